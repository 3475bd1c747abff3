#!/opt/conda/bin/python3.9
"""Goldens for the sensory-region filter (`Tissue.detect_non_sensory_region_cells`, ti.py:614-620, and
`Tissue.remove_cells_outside_of_sensory_region`, ti.py:2781-2792), from the REFERENCE's own two methods.

    /opt/conda/bin/python3.9 tools/make_goldens_sensory.py     -> tests/golden/sensory_region.npz

Run with the interpreter and the stubs of tools/make_goldens_graph.py, whose frame builders are imported.  Cases:
  A   a 128 x 96 Voronoi label map (about 60 cells) tabulated by the reference, 12 of its valid rows HC; no type map
  B   A's frame with rows of type 3, invalid hair cells, empty rows -- none of which may span the hull -- and a type map
  C   two hair cells: the reference raises; the exception's class name is recorded
  D   a 10 x 10 lattice of centroids spaced 7.5 (block label map, type map): every other row HC and the four corners, so that the
      hull is the square, its edges carry collinear hair cells and 36 rows lie exactly on the boundary
  E   11 500 rows, 3 000 of them HC, centroids uniform over 2048 x 2048: table only (detect_non_sensory_region_cells)

Recorded per case: the input columns (cx, cy, type, valid, empty_cell), the label map and the type map where there is one, the
reference's outside rows as flags, `valid` and the type map after the call, and each row's distance to the hull's boundary.

The generator checks its own fixtures (tests/hull_restate.py, exact rational arithmetic): every row must be a hull vertex or lie
farther from the hull's boundary than 1e-9 x the hull's diameter -- D's rows that lie EXACTLY on the boundary are exempt and
listed -- and the reference's flags must equal the exact strict-outside test on every row, D's boundary rows counting as inside.
A fixture whose answer rests on Qhull's rounding cannot be written.  The reference's time on case E is recorded with the machine's
name.  Only data is written."""
import os
import platform
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens_graph as mg  # noqa: E402  (stubs, reference imports, frame builders)

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
import hull_restate as hr  # noqa: E402

np, pandas, ti = mg.np, mg.pandas, mg.ti
BAND = 1e-9


def hand_tissue(tmp, tag, cx, cy, type, valid, empty, labels=None, type_map=None):
    n = len(cx)
    df = pandas.DataFrame({"area": np.full(n, 100), "perimeter": np.full(n, 40.0), "label": np.arange(1, n + 1),
                           "cx": np.asarray(cx, float), "cy": np.asarray(cy, float), "n_neighbors": 0,
                           "valid": np.asarray(valid, int), "type": np.asarray(type, int), "empty_cell": np.asarray(empty, int)})
    return with_table(tmp, tag, df, labels, type_map)


def with_table(tmp, tag, df, labels, type_map):
    t = ti.Tissue(1, os.path.join(tmp, "movie_" + tag), ["zo", "atoh"], load_to_memory=True)
    t.type_names = ["HC"]
    if labels is not None:
        t.labels_list[0] = labels
        t.set_labels(1, labels, reset_data=False)
    t.cell_info_list[0] = df
    t.set_cells_info(1, df)
    if type_map is not None:
        t.cells_type_list[0] = type_map
        t.set_cell_types(1, type_map)
    return t


def type_map_of(labels, type, valid):
    lut = np.full(int(labels.max()) + 1, 255, np.uint8)
    ok = np.asarray(valid) == 1
    lut[1:len(type) + 1][ok] = np.asarray(type, np.uint8)[ok]
    return lut[labels]


def record(out, tag, t, with_frame):
    ci = t.get_cells_info(1)
    cols = {k: ci[k].to_numpy().copy() for k in ("cx", "cy", "type", "valid", "empty_cell")}
    labels = t.get_labels(1) if with_frame else None
    types_in = None if not with_frame or t.get_cell_types(1) is None else np.array(t.get_cell_types(1), copy=True)
    try:
        rows = np.asarray(ti.Tissue.detect_non_sensory_region_cells(ci))
    except Exception as e:      # noqa: BLE001  (the golden records the exception's type)
        out["raises_" + tag] = np.asarray(type(e).__name__)
        for k, v in cols.items():
            out["%s_%s" % (k, tag)] = np.asarray(v, np.float64 if k in ("cx", "cy") else np.uint8)
        print(tag, "raises", type(e).__name__)
        return
    flags = np.zeros(len(ci), np.uint8)
    flags[rows] = 1
    if with_frame:
        assert t.remove_cells_outside_of_sensory_region(1) == 0
        assert np.array_equal(np.flatnonzero(ci["valid"].to_numpy() == 0), np.flatnonzero((cols["valid"] == 0) | (flags == 1)))
    # the band condition and the exact answer
    pts = hr.exact_points(cols["cx"], cols["cy"])
    hull = hr.convex_hull(pts, hr.hair_rows(cols["type"], cols["valid"], cols["empty_cell"]))
    exact = np.array([1 if hr.outside(pts, hull, p) else 0 for p in pts], np.uint8)
    margin = hr.margins(cols["cx"], cols["cy"], hull)
    hx, hy = cols["cx"][hull], cols["cy"][hull]
    diameter = float(np.sqrt((hx[:, None] - hx[None]) ** 2 + (hy[:, None] - hy[None]) ** 2).max())
    on_boundary = np.array([exact[r] == 0 and any(hr.orient(pts[hull[k]], pts[hull[(k + 1) % len(hull)]], pts[r]) == 0
                                                  for k in range(len(hull))) for r in range(len(pts))])
    vertex = np.isin(np.arange(len(pts)), hull)
    in_band = ~vertex & (margin <= BAND * diameter)
    if tag == "D":
        assert np.array_equal(in_band, on_boundary & ~vertex), "D: a row in the band that is not exactly on the boundary"
        assert int(on_boundary.sum()) == 36, int(on_boundary.sum())
        out["boundary_rows_D"] = np.flatnonzero(on_boundary).astype(np.int64)
    else:
        assert not in_band.any(), (tag, np.flatnonzero(in_band), margin[in_band])
    assert np.array_equal(flags, exact), (tag, np.flatnonzero(flags != exact))
    for k, v in cols.items():
        out["%s_%s" % (k, tag)] = np.asarray(v, np.float64 if k in ("cx", "cy") else np.uint8)
    out["outside_" + tag] = flags
    out["hull_" + tag] = np.asarray(hull, np.int32)
    out["margin_" + tag] = margin
    out["diameter_" + tag] = np.float64(diameter)
    if with_frame:
        out["labels_" + tag] = np.asarray(labels, np.int32)
        out["valid_out_" + tag] = ci["valid"].to_numpy().astype(np.uint8)
        if types_in is not None:
            out["types_in_" + tag] = types_in.astype(np.uint8)
            out["types_out_" + tag] = np.asarray(t.get_cell_types(1), np.uint8)
            print(tag, "type-map pixels repainted:", int((out["types_out_" + tag] != out["types_in_" + tag]).sum()))
    print(tag, "rows", len(pts), "hair cells", len(hr.hair_rows(cols["type"], cols["valid"], cols["empty_cell"])), "hull", len(hull),
          "outside", int(flags.sum()), "smallest non-vertex margin %.3g" % margin[~vertex & ~on_boundary].min(), "diameter %.4g" % diameter)


def main():
    tmp = tempfile.mkdtemp(prefix="tipgold_sensory_")
    out = {"band": np.float64(BAND)}

    labels, rng = mg.voronoi_labels(96, 128, 34, 71)
    base = mg.tabulate(tmp, "A0", labels, rng).get_cells_info(1).copy()
    n = base.shape[0]
    ok = np.flatnonzero((base["valid"].to_numpy() == 1) & (base["area"].to_numpy() > 0))
    hc = rng.choice(ok, 12, replace=False)
    a = base.copy()
    a["type"] = 0
    a.loc[hc, "type"] = 1
    a["neighbors"] = [set() for _ in range(n)]
    record(out, "A", with_table(tmp, "A", a.copy(), labels.copy(), None), True)

    b = a.copy()
    b["neighbors"] = [set() for _ in range(n)]
    rest = np.setdiff1d(ok, hc)
    picks = rng.choice(rest, 9, replace=False)
    b.loc[picks[:3], "type"] = 3                                   # bit 0 set, but not == 1
    b.loc[picks[3:6], "type"] = 1
    b.loc[picks[3:6], "valid"] = 0                                 # invalid hair cells
    b.loc[picks[6:9], "type"] = 1
    b.loc[picks[6:9], "empty_cell"] = 1                            # empty hair cells
    tmap = type_map_of(labels, b["type"].to_numpy(), b["valid"].to_numpy())
    record(out, "B", with_table(tmp, "B", b, labels.copy(), tmap), True)

    record(out, "C", hand_tissue(tmp, "C", [3.0, 40.0, 20.0, 8.0], [5.0, 30.0, 11.0, 25.0], [1, 1, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0]), False)

    gi, gj = np.mgrid[0:10, 0:10]
    gi, gj = gi.ravel(), gj.ravel()
    corner = np.isin(gi, (0, 9)) & np.isin(gj, (0, 9))
    dtype = (((gi + gj) % 2 == 0) | corner).astype(int)
    dlabels = (np.arange(80)[:, None] // 8 * 10 + np.arange(80)[None, :] // 8 + 1).astype(np.int32)
    dvalid = np.ones(100, int)
    record(out, "D", hand_tissue(tmp, "D", gj * 7.5, gi * 7.5, dtype, dvalid, np.zeros(100, int), dlabels,
                                 type_map_of(dlabels, dtype, dvalid)), True)

    rng = np.random.default_rng(76)
    ne = 11500
    etype = np.zeros(ne, int)
    etype[rng.choice(ne, 3000, replace=False)] = 1
    evalid = (rng.random(ne) > 0.05).astype(int)
    te = hand_tissue(tmp, "E", rng.uniform(0, 2048, ne), rng.uniform(0, 2048, ne), etype, evalid, np.zeros(ne, int))
    record(out, "E", te, False)
    times = []
    for _ in range(7):
        t0 = time.perf_counter()
        ti.Tissue.detect_non_sensory_region_cells(te.get_cells_info(1))
        times.append(time.perf_counter() - t0)
    out["reference_seconds_E"] = np.asarray(sorted(times))
    out["reference_machine"] = np.asarray("%s, %d CPUs" % (platform.processor() or platform.machine(), os.cpu_count()))
    print("E: the reference's detect_non_sensory_region_cells, median %.2f ms of 7" % (1e3 * float(np.median(times))))

    import scipy
    path = os.path.join(mg.OUT, "sensory_region.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, pandas.__version__, scipy.__version__]), **out)
    print("wrote sensory_region.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
