"""The goldens of the neighbour-graph features (tests/golden/graph_features.npz, tools/make_goldens_graph.py) as test cases: the
frames' tables, the case list, what the reference returned, and the evaluation of a case on a set of kernels -- the numpy
restatement (tests/graph_restate.py) or the device entries behind the same signatures."""
import os

import numpy as np

import graph_restate as gr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_features.npz")
FRAMES = ("A", "B", "H")
TYPE_BITS = {"HC": 0, "X": 1}
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(GOLDEN))
    return _cache["g"]


def frame(tag):
    """the frame's label map, table columns as the kernels take them, CSR of its neighbour sets and the contact triples"""
    if tag not in _cache:
        g = golden()
        col = lambda name, dtype: g["ci_%s_%s" % (tag, name)].astype(dtype)      # noqa: E731
        f = dict(labels=g["labels_" + tag].astype(np.int32), offsets=g["nb_off_" + tag].astype(np.int32),
                 adj=g["nb_adj_" + tag].astype(np.int32), valid=col("valid", np.uint8), empty=col("empty_cell", np.uint8),
                 type=col("type", np.uint8), working=g["working_" + tag].astype(np.uint8),
                 all_offsets=g["all_off_" + tag].astype(np.int32), all_adj=g["all_adj_" + tag].astype(np.int32),
                 cells=(g["cells_full_" + tag].astype(np.int32), g["cells_nz_" + tag].astype(np.int32)))
        f["n"] = f["valid"].size
        f["triples"] = gr.contact_triples(f["labels"])
        _cache[tag] = f
    return _cache[tag]


def cases(tag=None):
    g = golden()
    out = []
    for k in range(g["case_frame"].size):
        c = dict(k=k, frame=str(g["case_frame"][k]), method=str(g["case_method"][k]), cell_type=str(g["case_cell_type"][k]),
                 positive=bool(g["case_positive"][k]), second=bool(g["case_second"][k]), status=int(g["case_status"][k]),
                 exc=str(g["case_exc"][k]), cells_kind=int(g["case_cells"][k]))
        if tag is None or c["frame"] == tag:
            out.append(c)
    return out


def expected(c):
    """the reference's return value in comparable form, or None for a case it raised on"""
    if c["status"] != 0:
        return None
    g, key = golden(), "res_%03d" % c["k"]
    if c["method"] in ("son", "son0"):
        return [set(g[key][a:b].tolist()) for a, b in zip(g[key + "_off"][:-1], g[key + "_off"][1:])]
    if c["method"] == "ccl":
        off = g[key + "_off"]
        return [(g[key + "_labels"][a:b].tolist(), g[key][a:b].tolist()) for a, b in zip(off[:-1], off[1:])]
    return g[key]


def query_rows(c):
    f = frame(c["frame"])
    if c["method"] == "son0":
        return np.flatnonzero(f["valid"] == 1).astype(np.int32)
    return f["cells"][c["cells_kind"]]


def _selector(cell_type, positive):
    if cell_type in ("all", "valid", "invalid"):
        return {"all": gr.ALL, "valid": gr.VALID, "invalid": gr.INVALID}[cell_type], -1, True
    return gr.TYPE, TYPE_BITS[cell_type], positive


def on_kernels(ops, c):
    """case c through the kernels `ops` (graph_restate's signatures), in expected()'s form; None when the case is not a kernel's
    business (the raising cases and the all-zero column are the Python layer's)"""
    if c["status"] != 0:
        return None
    f = frame(c["frame"])
    q = query_rows(c)
    graph = (f["offsets"], f["adj"])
    if c["method"] == "nnt":
        if c["second"]:
            if c["cell_type"] != "all":
                return None
            return np.asarray([len(s) for s in ops.graph_second(*graph, f["valid"], f["type"], q, -1, True)], dtype=np.int64)
        mode, bit, positive = _selector(c["cell_type"], c["positive"])
        return ops.graph_counts(*graph, f["valid"], f["empty"], f["type"], q, mode, bit, positive)
    if c["method"] == "nbt":
        if not c["cell_type"]:
            return None              # type_list=None: upstream's pos / neg type lists, outside the device selector
        return np.stack([ops.graph_counts(*graph, f["valid"], f["empty"], f["type"], q, gr.TYPE, TYPE_BITS[name], True)
                         for name in ("HC", "X")], axis=1)
    if c["method"] in ("son", "son0"):
        bit = -1 if c["cell_type"] == "all" else TYPE_BITS[c["cell_type"]]
        return ops.graph_second(*graph, f["valid"], f["type"], q, bit, c["positive"])
    feature = {"contact length": ("all", True), "HC contact length": ("HC", True), "SC contact length": ("HC", False)}
    cell_type, positive = feature[c["cell_type"]] if c["method"] == "gfd" else (c["cell_type"], c["positive"])
    mode, bit, positive = _selector(cell_type, positive)
    sums, labels, values = ops.contact_sums(*f["triples"], *graph, f["valid"], f["type"], q, mode, bit, positive)
    if c["method"] == "gfd":
        return sums
    return [(l.tolist(), v.tolist()) for l, v in zip(labels, values)]


def assert_same(got, want):
    if isinstance(want, list):
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, "row %d: %r != %r" % (i, a, b)
    else:
        np.testing.assert_array_equal(np.asarray(got), want)
