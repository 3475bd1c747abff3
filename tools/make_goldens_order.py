#!/opt/conda/bin/python3.9
"""Goldens for the hexatic order and the neighbour correlations (`Tissue.find_nearest_neighbors_using_voroni_tesselation`,
`calc_psin`, `find_second_order_neighbors` as calc_psin's other input, `calculate_neighbors_correlation_function`; ti.py:803-843,
2513-2583), from the REFERENCE's own methods.

    /opt/conda/bin/python3.9 tools/make_goldens_order.py     -> tests/golden/order_features.npz

Run with the interpreter and the stubs of tools/make_goldens_graph.py, whose frame builders are imported.  Tables:
  A (96 x 96, 80 sites), B (64 x 80, 50 sites)   the graph goldens' frames: segmented, tabulated and typed by the reference; the
                                                  query rows are its get_valid_non_edge_cells
  H   one centre point inside a ring of 72 points at seeded radii 40 +- RING_JITTER: the centre's row is longer than a wavefront
  L   the integer 5 x 4 lattice (cocircular quadruples: exact ties)
  C   two clusters of 20 points 400 px apart and one lone point (ring growth, the whole-grid case)
The hand-made tables H, L and C are all valid; their `neighbors` column is the reference's own Voronoi sets, so that
find_second_order_neighbors and the correlations run on them too.  Every table gets a seeded type byte ("HC" = bit 0, "X" = bit 1)
and a seeded mean_intensity_HC column.

Recorded per table: the columns, the query rows, the Voronoi sets and the second-order sets as sorted CSR, calc_psin for n = 6 and
n = 4 over both, the correlation for every CORR case, and for the RAISING cases the exception's class.

The generator checks its own inputs: every pair's interval is evaluated in exact rational arithmetic on the float coordinates;
the exact edges must equal scipy's on every table, and the smallest relative gap |hi - lo| / max(|hi|, |lo|) over all pairs of A, B,
H and C must be at least 1e-9 (L's ties are exact in float64 and are exempt).  Only data is written."""
import os
import sys
import tempfile
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens_graph as mg  # noqa: E402  (stubs, reference imports, frame builders)

np, pandas, ti = mg.np, mg.pandas, mg.ti

RING_JITTER = 0.1
CORR = [("type", "HC"), ("type", "X"), ("intensity", "HC")]
METHODS = ["neighbors", "neighbors average"]
RAISING = [("type", "neighbors", "nope"), ("type", "neighbors_average", "HC"), ("intensity", "neighbours", "HC")]


def exact_edges(px, py):
    """(edges, smallest relative gap) of the interval rule in rational arithmetic"""
    n = len(px)
    X, Y = [Fraction(float(v)) for v in px], [Fraction(float(v)) for v in py]
    edges, gap = set(), None
    for i in range(n):
        for j in range(i + 1, n):
            ax, ay = X[j] - X[i], Y[j] - Y[i]
            lo = hi = None
            blocked = False
            for k in range(n):
                if k == i or k == j:
                    continue
                bx, by = X[k] - X[i], Y[k] - Y[i]
                s = ax * by - ay * bx
                num = bx * bx + by * by - (ax * bx + ay * by)
                if s == 0:
                    blocked = blocked or num < 0
                    continue
                t = num / (2 * s)
                if s > 0:
                    hi = t if hi is None else min(hi, t)
                else:
                    lo = t if lo is None else max(lo, t)
            if lo is not None and hi is not None:
                scale = max(abs(lo), abs(hi))
                rel = abs(hi - lo) / scale if scale else Fraction(0)
                gap = rel if gap is None else min(gap, rel)
            if not blocked and (lo is None or hi is None or lo < hi):
                edges.add((i, j))
    return edges, (float(gap) if gap is not None else float("inf"))


def point_table(tmp, tag, px, py, rng):
    n = len(px)
    df = pandas.DataFrame({"area": np.full(n, 100), "perimeter": np.full(n, 40.0), "label": np.arange(1, n + 1), "cx": np.asarray(px, float),
                           "cy": np.asarray(py, float), "n_neighbors": 0, "valid": 1, "empty_cell": 0})
    df["type"] = np.zeros(n, np.uint8)
    df["neighbors"] = [set() for _ in range(n)]
    t = ti.Tissue(1, os.path.join(tmp, "movie_" + tag), ["zo", "atoh"], load_to_memory=True)
    t.type_names = ["HC", "X"]
    t.cell_info_list[0] = df
    t.set_cells_info(1, df)
    sets = ti.Tissue.find_nearest_neighbors_using_voroni_tesselation(df)
    df["neighbors"] = [set(int(v) for v in s) for s in sets]
    df["n_neighbors"] = [len(s) for s in sets]
    return t


def main():
    tmp = tempfile.mkdtemp(prefix="tipgold_order_")
    tables = {}
    for tag, ny, nx, nsites, seed in (("A", 96, 96, 80, 51), ("B", 64, 80, 50, 52)):
        labels, rng = mg.voronoi_labels(ny, nx, nsites, seed)
        t = mg.tabulate(tmp, tag, labels, rng)
        tables[tag] = (t, t.get_valid_non_edge_cells(1, t.get_cells_info(1)), rng)
    rng = np.random.default_rng(61)
    ang = 2 * np.pi * np.arange(72) / 72
    rad = 40.0 + rng.uniform(-RING_JITTER, RING_JITTER, 72)
    tables["H"] = (point_table(tmp, "H", np.concatenate([[50.0], 50.0 + rad * np.cos(ang)]), np.concatenate([[50.0], 50.0 + rad * np.sin(ang)]), rng),
                   None, rng)
    gy, gx = np.mgrid[0:4, 0:5]
    tables["L"] = (point_table(tmp, "L", gx.ravel().astype(float), gy.ravel().astype(float), rng), None, np.random.default_rng(62))
    rng = np.random.default_rng(63)
    cx = np.concatenate([rng.uniform(0, 30, 20), rng.uniform(400, 430, 20), [215.0]])
    cy = np.concatenate([rng.uniform(0, 30, 20), rng.uniform(0, 30, 20), [160.0]])
    tables["C"] = (point_table(tmp, "C", cx, cy, rng), None, rng)

    out = {"frames": np.asarray(list(tables)), "corr_state": np.asarray([c[0] for c in CORR]), "corr_type": np.asarray([c[1] for c in CORR]),
           "corr_methods": np.asarray(METHODS), "raise_state": np.asarray([r[0] for r in RAISING]),
           "raise_method": np.asarray([r[1] for r in RAISING]), "raise_type": np.asarray([r[2] for r in RAISING]),
           "ring_jitter": np.float64(RING_JITTER)}
    for tag, (t, cells, rng) in tables.items():
        ci = t.get_cells_info(1)
        n = ci.shape[0]
        if tag in "HLC":
            draw = rng.random(n)
            ci["type"] = np.select([draw < 0.3, draw < 0.4, draw < 0.5], [1, 3, 2], 0).astype(np.uint8)
        ci["mean_intensity_HC"] = rng.uniform(0.0, 2.0, n)
        cells = ci if cells is None else ci.loc[cells.index]
        rows = cells.index.to_numpy()
        px, py = cells.cx.to_numpy(), cells.cy.to_numpy()
        sets = t.find_nearest_neighbors_using_voroni_tesselation(cells)
        exact, gap = exact_edges(px, py)
        scipy_edges = {(min(q, int(np.flatnonzero(rows == v - 1)[0])), max(q, int(np.flatnonzero(rows == v - 1)[0]))) for q, s in enumerate(sets) for v in s}
        assert exact == scipy_edges, tag
        assert tag == "L" or gap >= 1e-9, (tag, gap)
        son = t.find_second_order_neighbors(1, cells)
        for name, dtype in (("cx", np.float64), ("cy", np.float64), ("valid", np.uint8), ("type", np.uint8), ("empty_cell", np.uint8),
                            ("mean_intensity_HC", np.float64)):
            out["ci_%s_%s" % (tag, name)] = np.asarray(ci[name].to_numpy(), dtype=dtype)
        out["nb_off_" + tag], out["nb_adj_" + tag] = mg.csr(ci["neighbors"])
        out["cells_" + tag] = rows.astype(np.int64)
        out["vor_off_" + tag], out["vor_mem_" + tag] = mg.csr(sets)
        out["son_off_" + tag], out["son_mem_" + tag] = mg.csr(son)
        out["gap_" + tag] = np.float64(gap)
        for order in (6, 4):
            for kind, lists in (("vor", sets), ("son", son)):
                a = np.asarray(t.calc_psin(1, cells, lists, n=order), dtype=np.float64)
                b = np.asarray(t.calc_psin(1, cells, lists, n=order, for_histogram=True), dtype=np.float64)
                assert np.array_equal(a, b)
                out["psi_%s_%d_%s" % (tag, order, kind)] = a
        corr = np.zeros((len(CORR), len(METHODS)))
        for a, (state, type_name) in enumerate(CORR):
            for b, method in enumerate(METHODS):
                with np.errstate(all="ignore"):
                    corr[a, b] = t.calculate_neighbors_correlation_function(1, cells, set_state_by=state, method=method, type_name=type_name)
        out["corr_" + tag] = corr
        excs = []
        for state, method, type_name in RAISING:
            try:
                t.calculate_neighbors_correlation_function(1, cells, set_state_by=state, method=method, type_name=type_name)
                excs.append("")
            except Exception as e:       # noqa: BLE001  (the golden records the exception's type)
                excs.append(type(e).__name__)
        out["raise_exc_" + tag] = np.asarray(excs)
        deg = max(len(s) for s in sets)
        print(tag, "rows", n, "cells", rows.size, "max degree", deg, "gap %.3g" % gap, "corr", corr.round(4).tolist(), excs)
        assert tag != "H" or deg > 64
    import scipy
    path = os.path.join(mg.OUT, "order_features.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, pandas.__version__, scipy.__version__]), **out)
    print("wrote order_features.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
