#!/opt/conda/bin/python3.9
"""Goldens for the spatial feature maps and window statistics (`Tissue.calculate_spatial_data`, `calculate_data_around_a_given_cell`,
`get_frame_data`, ti.py:1035-1134, 1194-1266, 1610-1644), from the REFERENCE's own methods on small synthetic frames.

    /opt/conda/bin/python3.9 tools/make_goldens_spatial.py     -> tests/golden/spatial_maps.npz

Frames: a dense Voronoi tessellation from the repo's synthetic generator, segmented with the reference's `watershed_segmentation` and
tabulated with its `calculate_frame_cellinfo`; types by a seeded draw over two type names ("HC" = bit 0, "X" = bit 1) with a few
invalid (255) bytes.  Frame E is frame A with every row made invalid: no valid non-edge cell.  Only data is written: the label maps,
the table columns, the case list and what the reference returned for each case (a map, an error message, or the exception it raised)."""
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

COLUMNS = ["area", "perimeter", "label", "cx", "cy", "n_neighbors", "valid", "type", "empty_cell"]

# (frame, window_radius, step_size, feature, cells_type, positive_for_type)
CASES = [
    ("A", 25.5, 5, "HC density", "all", True),
    ("A", 25.5, 7, "HC type_fraction", "all", True),
    ("A", 25.5, 2, "HC type_fraction", "all", True),
    ("A", 10, 2, "HC density", "all", True),            # empty windows: density 0 there ...
    ("A", 10, 2, "area", "all", True),                  # ... and the error return for a mean
    ("A", 60, 16, "density", "all", True),
    ("A", 25.5, 16, "area", "all", True),
    ("A", 25.5, 7, "roundness", "all", True),
    ("A", 60, 5, "shape index", "all", True),
    ("A", 25.5, 5, "n_neighbors", "all", True),
    ("A", 25.5, 1, "HC density", "all", True),          # step 1: step // 2 == 0, every block is empty
    ("A", 25.5, 5, "density", "HC", False),
    ("A", 60, 7, "area", "HC", True),
    ("A", 25.5, 7, "type_fraction", "X", False),
    ("B", 25.5, 7, "HC density", "all", True),
    ("B", 60, 16, "HC type_fraction", "all", True),
    ("B", 10, 5, "density", "all", True),
    ("B", 60, 5, "roundness", "all", True),
    ("B", 25.5, 5, "shape index", "all", True),
    ("B", 60, 7, "n_neighbors", "HC", False),
    ("B", 25.5, 16, "type_fraction", "X", True),
    ("B", 25.5, 16, "area", "X", True),
    ("E", 25.5, 5, "HC density", "all", True),          # no valid non-edge cell
    ("E", 25.5, 5, "area", "all", True),
    ("A", 25.5, 5, "SC density", "all", True),          # "SC" is no type name: the reference raises
    ("A", 25.5, 5, "density", "nope", True),
]


def make_frame(tmp, tag, ny, nx, nsites, seed):
    rng = np.random.default_rng(seed)
    sites = np.stack([rng.uniform(0, ny, nsites), rng.uniform(0, nx, nsites)], axis=1)
    d1, d2, _ = synthetic._two_nearest(sites, ny, nx)
    membrane = np.exp(-((d2 - d1) ** 2) / 4.0)
    labels = np.asarray(bim.watershed_segmentation(membrane.copy(), 0.03, 1, 3)).astype(np.int32)
    t = ti.Tissue(1, os.path.join(tmp, "movie_" + tag), ["zo", "atoh"], load_to_memory=True)
    t.labels_list[0] = labels.copy()
    t.set_labels(1, labels.copy(), reset_data=False)
    t.calculate_frame_cellinfo(1)
    ci = t.cells_info.copy()
    draw = rng.random(ci.shape[0])
    typ = np.select([draw < 0.3, draw < 0.4, draw < 0.5, draw < 0.55], [1, 3, 2, 255], 0).astype(np.uint8)
    ci["type"] = typ
    t.cell_info_list[0] = ci
    t.set_cells_info(1, ci)
    t.type_names = ["HC", "X"]
    return t, labels


def table(t):
    ci = t.get_cells_info(1)
    return {k: np.asarray(ci[k].to_numpy(), dtype=np.float64) for k in COLUMNS}


def record(out, key, fn):
    """what fn() gives: status 0 = value, 1 = (None, message), 2 = raises"""
    try:
        data, msg = fn()
    except Exception as e:       # noqa: BLE001  (the golden records the exception's type)
        return 2, type(e).__name__
    if data is None:
        return 1, msg
    out[key] = np.asarray(data, dtype=np.float64)
    return 0, msg


def main():
    tmp = tempfile.mkdtemp(prefix="tipgold_sp_")
    out = {}
    tissues = {}
    for tag, ny, nx, nsites, seed in (("A", 96, 80, 70, 41), ("B", 128, 128, 100, 42)):
        t, labels = make_frame(tmp, tag, ny, nx, nsites, seed)
        tissues[tag] = t
        out["labels_" + tag] = labels
        for k, v in table(t).items():
            out["ci_%s_%s" % (tag, k)] = v
        valid = t.get_valid_non_edge_cells(1, t.get_cells_info(1))
        out["valid_rows_" + tag] = np.asarray(valid.index.to_numpy(), dtype=np.int64)
        print(tag, labels.shape, "rows", t.get_cells_info(1).shape[0], "valid non-edge", valid.shape[0])
    t, labels = make_frame(tmp, "E", 96, 80, 70, 41)
    t.get_cells_info(1)["valid"] = 0
    tissues["E"] = t
    assert t.get_valid_non_edge_cells(1, t.get_cells_info(1)).shape[0] == 0
    # ---- maps -------------------------------------------------------------------------------------------------------------------------
    status, msgs = [], []
    for k, (tag, radius, step, feature, cells_type, positive) in enumerate(CASES):
        t = tissues[tag]
        s, m = record(out, "case%02d_map" % k,
                      lambda: t.calculate_spatial_data(1, radius, step, feature, cells_type=cells_type, positive_for_type=positive))
        status.append(s)
        msgs.append(m)
        print(k, tag, radius, step, feature, cells_type, positive, "->", s, m)
    out["case_frame"] = np.asarray([c[0] for c in CASES])
    out["case_radius"] = np.asarray([c[1] for c in CASES], dtype=np.float64)
    out["case_step"] = np.asarray([c[2] for c in CASES], dtype=np.int64)
    out["case_feature"] = np.asarray([c[3] for c in CASES])
    out["case_cells_type"] = np.asarray([c[4] for c in CASES])
    out["case_positive"] = np.asarray([c[5] for c in CASES], dtype=np.int64)
    out["case_status"] = np.asarray(status, dtype=np.int64)
    out["case_msg"] = np.asarray(msgs)
    # ---- per-cell windows and get_frame_data ---------------------------------------------------------------------------------------------
    for tag in ("A", "B"):
        t = tissues[tag]
        info = t.get_cells_info(1)
        valid = t.get_valid_non_edge_cells(1, info)
        kw = dict(special_features=t.SPECIAL_FEATURES, global_features=t.GLOBAL_FEATURES, spatial_features=t.SPATIAL_FEATURES)
        st = []
        for feature in t.SPATIAL_FEATURES:
            for hist in (False, True):
                s, m = record(out, "gfd_%s_%s_%d" % (tag, feature, hist),
                              lambda: t.get_frame_data(1, feature, valid, for_histogram=hist, window_radius=25.5, **kw))
                st.append(s if s != 2 else {"KeyError": 2}.get(m, 3))
        out["gfd_%s_spatial_status" % tag] = np.asarray(st, dtype=np.int64)       # SPATIAL_FEATURES x (False, True); 2 = KeyError
        for feature in ("shape index", "roundness", "area", "perimeter", "n_neighbors", "density", "type_fraction", "total_area",
                        "number_of_cells"):
            s, m = record(out, "gfd_%s_%s" % (tag, feature), lambda: t.get_frame_data(1, feature, valid, **kw))
            assert s == 0
        hc = valid.loc[ti.is_positive_for_type(valid.type.to_numpy(), 0)]
        out["hc_rows_" + tag] = np.asarray(hc.index.to_numpy(), dtype=np.int64)
        for feature in ("density", "type_fraction", "total_area", "number_of_cells"):
            s, m = record(out, "gfd_hc_%s_%s" % (tag, feature), lambda: t.get_frame_data(1, feature, hc, **kw))
            assert s == 0
        # windows around single cells: a scalar for the two ratio features, the selected cells' values for the others
        picks = [0, valid.shape[0] // 2, valid.shape[0] - 1]
        out["around_rows_" + tag] = np.asarray(valid.index.to_numpy()[picks], dtype=np.int64)
        for j, p in enumerate(picks):
            cell = valid.iloc[p]
            for feature, cells_type, positive in (("HC density", "all", True), ("type_fraction", "HC", False), ("area", "HC", True),
                                                  ("roundness", "all", True)):
                s, m = record(out, "around_%s_%d_%s_%s_%d" % (tag, j, feature, cells_type, positive),
                              lambda: t.calculate_data_around_a_given_cell(1, cell, valid, 25.5, feature, cells_type,
                                                                           positive_for_type=positive))
                assert s == 0, (s, m)
        s, m = record(out, "around_%s_tiny" % tag,
                      lambda: t.calculate_data_around_a_given_point(1, 0.25, 0.75, valid, 0.5, "area", "all"))
        assert s == 1 and m == "No matching cells"
    import skimage
    np.savez_compressed(os.path.join(OUT, "spatial_maps.npz"),
                        versions=np.array([np.__version__, pandas.__version__, skimage.__version__]), **out)
    print("wrote spatial_maps.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(OUT, "spatial_maps.npz"))))


if __name__ == "__main__":
    main()
