#!/opt/conda/bin/python3.9
"""Goldens for the neighbour-graph feature columns (`Tissue.calculate_n_neighbors_from_type`, `calculate_n_neighbors_by_type`,
`find_second_order_neighbors`, `calculate_contact_length` and the contact-length loop of `get_frame_data`, ti.py:1065-1096,
1752-1799, 1844-1872, 2513-2543), from the REFERENCE's own methods on small frames.

    /opt/conda/bin/python3.9 tools/make_goldens_graph.py     -> tests/golden/graph_features.npz

Frames A (96 x 96) and B (64 x 80): dense Voronoi tessellations from the repo's synthetic generator, segmented with the reference's
`watershed_segmentation` and tabulated with its `calculate_frame_cellinfo` (which also runs its `find_neighbors` for the valid
rows); types by a seeded draw over two type names ("HC" = bit 0, "X" = bit 1) with a few invalid (255) bytes; afterwards a few
rows are made invalid and one row an `empty_cell`, the neighbour sets staying as they are.  Frame H (96 x 96) is hand-made: a hub
disc carrying the LARGEST label (so that upstream's find_neighbors, which finds a pair from its larger label, sees all of them from
the hub) inside a ring of thin radial cells -- the hub's row is longer than a wavefront --, and one blob in a corner that touches
label 0 only (degree 0).

Recorded per frame: the label map, the table columns, the neighbour sets as CSR, `find_neighbors(only_for_labels=None)` on a copy
as CSR, and for every (method, arguments) case what the reference returned or the class of the exception it raised.  Lists of sets
and per-contact arrays are recorded as CSR, SORTED per cell (upstream's order is Python's set iteration order).

The degree-0 row: where the reference fails on a case only because of a row without neighbours (it indexes the table with an empty
float array), the case is recorded with those rows kept out of `cells` (case_cells = 1); a case that raises either way is recorded
as raising, with the rows it was last run on.  Only data is written."""
import os
import sys
import tempfile
import types
import warnings

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub("aicsimageio", AICSImage=object)
_stub("aicsimageio.readers", czi_reader=None, bioformats_reader=None)
_stub("aicsimageio.writers", ome_tiff_writer=None)
_stub("trackpy")
sys.path.insert(0, os.path.join(REF, "tissue_analyzing_tool"))

import numpy as np  # noqa: E402
import pandas  # noqa: E402
import basic_image_manipulations as bim  # noqa: E402  (reference)
import tissue_info as ti  # noqa: E402  (reference)
from tissue_image_processing_amd import synthetic  # noqa: E402

if not hasattr(np, "bool"):          # ti.py:155 uses the alias numpy 1.24 removed
    np.bool = bool

COLUMNS = ["area", "perimeter", "label", "cx", "cy", "n_neighbors", "valid", "type", "empty_cell", "bounding_box_min_row",
           "bounding_box_min_col", "bounding_box_max_row", "bounding_box_max_col"]

# (method, cell_type, positive_for_type, second_neighbors)
#   nnt: calculate_n_neighbors_from_type      nbt: calculate_n_neighbors_by_type (cell_type: "HC,X" or "" for type_list=None)
#   son: find_second_order_neighbors (son0: cells=None)      ccl: calculate_contact_length row by row (ti.py:1087-1096)
#   gfd: get_frame_data(feature=cell_type, for_histogram=False), the contact-length features
CASES = [
    ("nnt", "all", True, False), ("nnt", "valid", True, False), ("nnt", "invalid", True, False),
    ("nnt", "HC", True, False), ("nnt", "HC", False, False), ("nnt", "X", True, False), ("nnt", "X", False, False),
    ("nnt", "all", True, True), ("nnt", "HC", True, True), ("nnt", "HC", False, True),
    ("nnt", "valid", True, True), ("nnt", "invalid", True, True),
    ("nnt", "same", True, False), ("nnt", "same", True, True), ("nnt", "nope", True, False),
    ("nbt", "HC,X", True, False), ("nbt", "", True, False),
    ("son0", "all", True, False),
    ("son", "all", True, False), ("son", "HC", True, False), ("son", "HC", False, False), ("son", "X", True, False),
    ("ccl", "all", True, False), ("ccl", "valid", True, False), ("ccl", "HC", True, False), ("ccl", "HC", False, False),
    ("ccl", "X", False, False),
    ("gfd", "contact length", True, False), ("gfd", "HC contact length", True, False), ("gfd", "SC contact length", True, False),
]


def tabulate(tmp, tag, labels, rng):
    t = ti.Tissue(1, os.path.join(tmp, "movie_" + tag), ["zo", "atoh"], load_to_memory=True)
    t.labels_list[0] = labels.copy()
    t.set_labels(1, labels.copy(), reset_data=False)
    t.calculate_frame_cellinfo(1)
    ci = t.cells_info.copy()
    draw = rng.random(ci.shape[0])
    ci["type"] = np.select([draw < 0.3, draw < 0.4, draw < 0.5, draw < 0.56], [1, 3, 2, 255], 0).astype(np.uint8)
    t.cell_info_list[0] = ci
    t.set_cells_info(1, ci)
    t.type_names = ["HC", "X"]
    return t


def voronoi_labels(ny, nx, nsites, seed):
    rng = np.random.default_rng(seed)
    sites = np.stack([rng.uniform(0, ny, nsites), rng.uniform(0, nx, nsites)], axis=1)
    d1, d2, _ = synthetic._two_nearest(sites, ny, nx)
    membrane = np.exp(-((d2 - d1) ** 2) / 4.0)
    return np.asarray(bim.watershed_segmentation(membrane.copy(), 0.03, 1, 3)).astype(np.int32), rng


def hub_labels(n_rays=72, r_hub=15.0, r_out=46.0):
    yy, xx = np.mgrid[0:96, 0:96]
    dy, dx = yy - 47.5, xx - 47.5
    r = np.sqrt(dy * dy + dx * dx)
    sector = np.floor((np.arctan2(dy, dx) + np.pi) / (2 * np.pi) * n_rays).astype(np.int64) % n_rays
    labels = np.zeros((96, 96), np.int32)
    ring = (r >= r_hub) & (r < r_out)
    labels[ring] = (sector[ring] + 1).astype(np.int32)          # rays 1 .. n_rays
    labels[3:7, 3:7] = n_rays + 1                                # the blob that touches label 0 only
    labels[r < r_hub] = n_rays + 2                               # the hub: the largest label
    return labels


def spoil(t, rng, invalid_rows, empty_row):
    """a few rows invalid, one an empty cell; neighbour sets stay"""
    ci = t.get_cells_info(1)
    for r in invalid_rows:
        ci.at[r, "valid"] = 0
    ci.at[empty_row, "empty_cell"] = 1


def csr(list_of_iterables, dtype=np.int64, sort=True):
    rows = [sorted(int(v) for v in s) if sort else [int(v) for v in s] for s in list_of_iterables]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.asarray([v for r in rows for v in r], dtype=dtype)


def run_case(t, case, cells):
    method, cell_type, positive, second = case
    if method == "nnt":
        return {"": np.asarray(t.calculate_n_neighbors_from_type(1, cells, cell_type=cell_type, positive_for_type=positive,
                                                                  second_neighbors=second), dtype=np.int64)}
    if method == "nbt":
        df = t.calculate_n_neighbors_by_type(1, cells, type_list=cell_type.split(",") if cell_type else None)
        return {"": np.asarray(df.to_numpy(), dtype=np.int64), "_columns": np.asarray(list(df.columns))}
    if method in ("son", "son0"):
        sets = t.find_second_order_neighbors(1, cells=None if method == "son0" else cells, cell_type=cell_type, positive_for_type=positive)
        off, members = csr(sets)
        return {"_off": off, "": members}
    if method == "ccl":
        labels = t.get_labels(1)
        from scipy.ndimage import maximum_filter, minimum_filter
        cross = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]])
        mx = maximum_filter(labels, footprint=cross, mode="constant")
        filled = labels.copy()
        filled[filled == 0] = np.max(filled) + 1
        mn = minimum_filter(filled, footprint=cross, mode="constant")
        labs, vals = [], []
        for _, cell in cells.iterrows():
            nl, cl = t.calculate_contact_length(1, cell, mx, mn, cell_type=cell_type, positive_for_type=positive)
            order = np.argsort(np.asarray(nl, dtype=np.int64), kind="stable")
            labs.append(np.asarray(nl, dtype=np.int64)[order])
            vals.append(np.asarray(cl, dtype=np.int64).reshape(-1)[order])
        off, lab = csr(labs, sort=False)
        _, val = csr(vals, sort=False)
        return {"_off": off, "_labels": lab, "": val}
    if method == "gfd":
        data, msg = t.get_frame_data(1, cell_type, cells, special_features=t.SPECIAL_FEATURES, global_features=t.GLOBAL_FEATURES,
                                     spatial_features=t.SPATIAL_FEATURES, for_histogram=False)
        assert msg == ""
        return {"": np.asarray(data, dtype=np.int64)}
    raise ValueError(method)


def main():
    tmp = tempfile.mkdtemp(prefix="tipgold_graph_")
    out = {}
    frames = {}
    for tag, ny, nx, nsites, seed in (("A", 96, 96, 80, 51), ("B", 64, 80, 50, 52)):
        labels, rng = voronoi_labels(ny, nx, nsites, seed)
        frames[tag] = (tabulate(tmp, tag, labels, rng), labels, rng)
    labels = hub_labels()
    frames["H"] = (tabulate(tmp, "H", labels, np.random.default_rng(53)), labels, np.random.default_rng(54))
    status, excs, cells_kind, case_frame = [], [], [], []
    k = 0
    for tag, (t, labels, rng) in frames.items():
        ci = t.get_cells_info(1)
        n = ci.shape[0]
        # CSR of find_neighbors(only_for_labels=None) on a copy of the table, before rows are spoilt
        keep = ci.copy(deep=True)
        keep["neighbors"] = [set(s) for s in ci["neighbors"]]
        t.find_neighbors(1, only_for_labels=None)
        off, adj = csr(t.get_cells_info(1)["neighbors"])
        out["all_off_" + tag], out["all_adj_" + tag] = off, adj
        t.cell_info_list[0] = keep
        t.set_cells_info(1, keep)
        ci = t.get_cells_info(1)
        out["working_" + tag] = np.asarray(ci["valid"].to_numpy() == 1, dtype=np.uint8)      # the rows calculate_frame_cellinfo worked on
        degree = np.asarray([len(s) for s in ci["neighbors"]])
        candidates = np.flatnonzero((ci["valid"].to_numpy() == 1) & (degree >= 3) & (degree <= 64))
        picks = rng.choice(candidates, size=4, replace=False)
        spoil(t, rng, picks[:3], picks[3])
        ci = t.get_cells_info(1)
        out["labels_" + tag] = labels
        for name in COLUMNS:
            out["ci_%s_%s" % (tag, name)] = np.asarray(ci[name].to_numpy(), dtype=np.float64)
        off, adj = csr(ci["neighbors"])
        out["nb_off_" + tag], out["nb_adj_" + tag] = off, adj
        full = ci[(ci["valid"].to_numpy() == 1) & (ci["empty_cell"].to_numpy() == 0)]
        nz = full[np.asarray([len(s) > 0 for s in full["neighbors"]])]
        out["cells_full_" + tag] = np.asarray(full.index.to_numpy(), dtype=np.int64)
        out["cells_nz_" + tag] = np.asarray(nz.index.to_numpy(), dtype=np.int64)
        print(tag, labels.shape, "rows", n, "cells", full.shape[0], "max degree", degree.max(), "degree 0 rows", int((degree == 0).sum()))
        for case in CASES:
            kind, res, exc = 0, None, ""
            try:
                res = run_case(t, case, full)
            except Exception as e:       # noqa: BLE001  (the golden records the exception's type)
                exc = type(e).__name__
                if nz.shape[0] != full.shape[0]:
                    kind = 1
                    try:
                        res, exc = run_case(t, case, nz), ""
                    except Exception as e2:       # noqa: BLE001
                        exc = type(e2).__name__
            for suffix, value in (res or {}).items():
                out["res_%03d%s" % (k, suffix)] = value
            status.append(0 if res is not None else 2)
            excs.append(exc)
            cells_kind.append(kind)
            case_frame.append(tag)
            print("%3d %s %-5s %-18s pos=%d second=%d cells=%s -> %s" % (k, tag, case[0], case[1], case[2], case[3], ("full", "nz")[kind],
                                                                       "ok" if res is not None else exc))
            k += 1
    ncase = len(CASES)
    out["case_frame"] = np.asarray(case_frame)
    out["case_method"] = np.asarray([c[0] for c in CASES] * len(frames))
    out["case_cell_type"] = np.asarray([c[1] for c in CASES] * len(frames))
    out["case_positive"] = np.asarray([c[2] for c in CASES] * len(frames), dtype=np.int64)
    out["case_second"] = np.asarray([c[3] for c in CASES] * len(frames), dtype=np.int64)
    out["case_status"] = np.asarray(status, dtype=np.int64)
    out["case_exc"] = np.asarray(excs)
    out["case_cells"] = np.asarray(cells_kind, dtype=np.int64)
    assert len(status) == ncase * len(frames)
    import scipy
    import skimage
    path = os.path.join(OUT, "graph_features.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, pandas.__version__, skimage.__version__, scipy.__version__]), **out)
    print("wrote graph_features.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
