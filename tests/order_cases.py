"""The goldens of the order features (tests/golden/order_features.npz, tools/make_goldens_order.py) as test cases: per table the
columns, the query rows, the reference's Voronoi and second-order sets and its psi and correlation values, and the derived
tolerances."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "order_features.npz")
FRAMES = ("A", "B", "H", "L", "C")
TYPE_BITS = {"HC": 0, "X": 1}
PSI_TOL = 1e-13          # atan2 within 2 ulp of pi (9e-16), times n = 6, plus an ulp of the product and of sincos: 1e-14 per
#                          unit term; the mean adds count * 2^-53 for the order of the sum; five times that bound
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(GOLDEN))
    return _cache["g"]


def frame(tag):
    if tag not in _cache:
        g = golden()
        col = lambda name: g["ci_%s_%s" % (tag, name)]      # noqa: E731
        f = dict(cy=col("cy"), cx=col("cx"), valid=col("valid"), type=col("type"), empty=col("empty_cell"),
                 intensity=col("mean_intensity_HC"), offsets=g["nb_off_" + tag].astype(np.int32), adj=g["nb_adj_" + tag].astype(np.int32),
                 cells=g["cells_" + tag].astype(np.int32), vor=(g["vor_off_" + tag], g["vor_mem_" + tag].astype(np.int32)),
                 son=(g["son_off_" + tag], g["son_mem_" + tag].astype(np.int32)), corr=g["corr_" + tag],
                 psi={(o, k): g["psi_%s_%d_%s" % (tag, o, k)] for o in (6, 4) for k in ("vor", "son")})
        f["n"] = f["cy"].size
        _cache[tag] = f
    return _cache[tag]


def sets_of(off, mem):
    return [set(int(v) for v in mem[off[q]:off[q + 1]]) for q in range(len(off) - 1)]


def label_sets(f, rows):
    """rows of 0-based positions among the query points -> sets of table labels, the reference's form"""
    return [set(int(f["cells"][v]) + 1 for v in r) for r in rows]


def corr_cases():
    g = golden()
    return [(a, b, str(s), str(t), str(m)) for a, (s, t) in enumerate(zip(g["corr_state"], g["corr_type"]))
            for b, m in enumerate(g["corr_methods"])]


def raising_cases(tag):
    g = golden()
    return [(str(s), str(m), str(t), str(e)) for s, m, t, e in zip(g["raise_state"], g["raise_method"], g["raise_type"], g["raise_exc_" + tag])]


def state_of(f, state_by, type_name):
    """the state of the query rows: 0 / 1 for "type" (positive for the type bit, 255 never), the intensity column otherwise"""
    if state_by == "intensity":
        return f["intensity"][f["cells"]].astype(np.float64)
    t = f["type"][f["cells"]]
    return (((t >> TYPE_BITS[type_name]) & 1).astype(bool) & (t != 255)).astype(np.float64)


def state_columns(f, state):
    """(member bytes, state over the whole table) for graph_neighbor_state"""
    member, full = np.zeros(f["n"], np.uint8), np.zeros(f["n"], np.float64)
    member[f["cells"]] = 1
    full[f["cells"]] = state
    return member, full


def corr_tol(state, state_by, contacts):
    """the value differs from upstream's by the order of its sums only: contacts * 2^-52 / var, scaled by max|state - mean|^2 for
    intensity states (type states: the products are at most 1)"""
    scale = 1.0 if state_by == "type" else float(np.max(np.abs(state - state.mean())) ** 2)
    return contacts * 2.0 ** -52 / float(np.var(state)) * scale
