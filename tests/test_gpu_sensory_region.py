"""GPU: the sensory-region filter (csrc/tip_hull.hip) -- hull, outside flags and invalidation against tip_sensory_region_host and the
goldens the reference's own methods wrote; the two Tissue methods against the goldens; GpuFrameBackend(sensory_region=True)
against the Tissue methods on the unfiltered run's frames."""
import ctypes
import warnings

import numpy as np
import pytest

import _gpu_movie_sensory_worker as w
import hull_cases as hc
from gloo_launch import run_ranks
from gpu_util import GuardedBuffer

pytestmark = pytest.mark.gpu

POINT_SETS = sorted(hc.CASES) + sorted(hc.BIG)


def _case(name):
    return hc.case(name)


def _selected(c):
    """the case's hull points as plain arrays, and their row positions"""
    rows = np.arange(c["cx"].size) if c["type"] is None else np.flatnonzero((c["type"] == 1) & (c["valid"] == 1) & (c["empty"] == 0))
    return c["cx"][rows], c["cy"][rows], rows


# ---- hull ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POINT_SETS)
def test_hull_equals_the_host_entry(name):
    from tissue_image_processing_amd import _segmentation as seg
    c = _case(name)
    px, py, rows = _selected(c)
    hull = seg.convex_hull(px, py)
    assert hull.dtype == np.int32
    np.testing.assert_array_equal(rows[hull], hc.host(name)[1])        # index for index: same start vertex, same orientation


def test_hull_survivors_pass_through_the_compaction():
    """70 000 points: more than one workgroup and more than 65 536 rows in the filter, and far fewer survivors than points"""
    from tissue_image_processing_amd import _lib, _segmentation as seg
    from gpu_util import launches
    c = hc.case("random70000")
    with launches() as ran:
        hull = seg.convex_hull(c["cx"], c["cy"])
    assert ran.get("hull_filter") == 1 and ran.get("hull_tangent") == 1 and ran.get("hull_sort_chunk", 0) >= 1
    assert 3 <= hull.size < 100
    lib, n = _lib.lib(), c["cx"].size
    big, n_hull = np.zeros(n, np.int32), ctypes.c_int64(0)
    assert lib.tip_convex_hull_f64(_lib.ptr(c["cx"]), _lib.ptr(c["cy"]), n, _lib.ptr(big), n, ctypes.byref(n_hull)) == 0
    np.testing.assert_array_equal(big[:n_hull.value], hull)


def test_hull_of_many_survivors_takes_the_multi_chunk_paths():
    """circle5000: every point survives the octagon, so the sort runs its steps between LDS chunks, and tangent and emit cross
    their 256-entry tiles; index for index the host entry's hull"""
    from tissue_image_processing_amd import _segmentation as seg
    from gpu_util import launches
    c = hc.case("circle5000")
    with launches() as ran:
        hull = seg.convex_hull(c["cx"], c["cy"])
    # 5 000 survivors pad to 8192 = 4 chunks of 2048: k = 4096 and 8192 need 1 + 2 steps between chunks and one chunk pass each
    assert ran.get("hull_sort_step") == 3 and ran.get("hull_sort_chunk") == 3 and ran.get("hull_pad") == 1
    want = hc.host("circle5000")[1]
    assert want.size > 2048
    np.testing.assert_array_equal(hull, want)


def test_hull_refuses_more_survivors_than_its_limit():
    """the tangent test is quadratic in the survivors: above 65 536 of them the entry says so instead of running for seconds"""
    from tissue_image_processing_amd import _lib
    c = hc.circle70000()
    assert np.unique(np.stack([c["cx"], c["cy"]], axis=1), axis=0).shape[0] == 70000
    hull, n_hull = np.zeros(70000, np.int32), ctypes.c_int64(0)
    rc = _lib.lib().tip_convex_hull_f64(_lib.ptr(c["cx"]), _lib.ptr(c["cy"]), 70000, _lib.ptr(hull), 70000, ctypes.byref(n_hull))
    assert rc == _lib.TIP_ERR_UNSUPPORTED and "65536" in _lib.last_error()


def test_hull_capacity_one_too_small_reports_the_size_needed():
    from tissue_image_processing_amd import _lib
    c = hc.case("circle200")
    want = hc.host("circle200")[1]
    lib, n = _lib.lib(), c["cx"].size
    hull, n_hull = np.full(want.size, -1, np.int32), ctypes.c_int64(0)
    rc = lib.tip_convex_hull_f64(_lib.ptr(c["cx"]), _lib.ptr(c["cy"]), n, _lib.ptr(hull), want.size - 1, ctypes.byref(n_hull))
    assert rc == _lib.TIP_ERR_OVERFLOW and n_hull.value == want.size and (hull == -1).all()
    rc = lib.tip_convex_hull_f64(_lib.ptr(c["cx"]), _lib.ptr(c["cy"]), n, _lib.ptr(hull), want.size, ctypes.byref(n_hull))
    assert rc == 0 and n_hull.value == want.size
    np.testing.assert_array_equal(hull, want)


def test_hull_dev_form_keeps_inside_its_buffers():
    from tissue_image_processing_amd import _lib
    c = hc.case("duplicates")
    want = hc.host("duplicates")[1]
    n = c["cx"].size
    dx, dy = GuardedBuffer((n,), np.float64, c["cx"]), GuardedBuffer((n,), np.float64, c["cy"])
    dh = GuardedBuffer((want.size,), np.float32)                        # (4-byte slots with NaN bands; read back as int32)
    n_hull = ctypes.c_int64(0)
    _lib.check(_lib.lib().tip_convex_hull_f64_dev(_lib.dptr(dx.ptr), _lib.dptr(dy.ptr), n, _lib.dptr(dh.ptr), want.size, ctypes.byref(n_hull)))
    got, bands_ok = dh.download()
    assert bands_ok and n_hull.value == want.size
    np.testing.assert_array_equal(got.view(np.int32), want)
    for b in (dx, dy, dh):
        b.buf.free()


@pytest.mark.parametrize("name", sorted(hc.DEGENERATE))
def test_hull_reports_no_hull(name):
    from tissue_image_processing_amd import _segmentation as seg
    c = hc.DEGENERATE[name]
    with pytest.raises(seg.NoHullError):
        seg.convex_hull(c["cx"], c["cy"])


# ---- outside flags ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POINT_SETS)
def test_outside_flags_equal_the_host_entry(name):
    from tissue_image_processing_amd import _segmentation as seg
    c = _case(name)
    want_outside, want_hull = hc.host(name)
    got = seg.points_outside_hull(c["cx"], c["cy"], want_hull, c["cx"], c["cy"])
    np.testing.assert_array_equal(got, want_outside)
    outside, hull = seg.sensory_region_dev(None, None, 0, c["cx"], c["cy"], c["type"], c["valid"], c["empty"])     # the driver's call
    np.testing.assert_array_equal(hull, want_hull)
    np.testing.assert_array_equal(outside, want_outside)


@pytest.mark.parametrize("tag", hc.GOLDEN_CASES)
def test_outside_flags_equal_the_reference(tag):
    from tissue_image_processing_amd import _segmentation as seg
    c = hc.golden_case(tag)
    outside, hull = seg.sensory_region_dev(None, None, 0, c["cx"], c["cy"], c["type"], c["valid"], c["empty"])
    np.testing.assert_array_equal(outside, hc.golden()["outside_" + tag])
    np.testing.assert_array_equal(hull, hc.golden()["hull_" + tag])


def test_outside_flags_of_no_queries():
    from tissue_image_processing_amd import _segmentation as seg
    c = hc.case("query_vertices")
    assert seg.points_outside_hull(c["cx"], c["cy"], hc.host("query_vertices")[1], np.zeros(0), np.zeros(0)).size == 0


# ---- invalidate ------------------------------------------------------------------------------------------------------------------
def test_invalidate_paints_the_selection_and_nothing_else():
    """64 x 96, every row starting off a multiple of 64 (the map sits 4 bytes into its buffer's alignment), label 0 and labels
    above n in the map"""
    from tissue_image_processing_amd import _lib, _segmentation as seg
    rng = np.random.default_rng(3)
    n = 40
    labels = rng.integers(0, n + 9, (64, 96)).astype(np.int32)
    assert (labels == 0).any() and (labels > n).any() and 96 % 64 != 0
    types = rng.integers(0, 4, (64, 96)).astype(np.uint8)
    outside = (rng.random(n) < 0.4).astype(np.uint8)
    want = types.copy()
    want[np.isin(labels, np.flatnonzero(outside) + 1)] = 255
    assert (want != types).any()
    d_lab, d_out = _lib.DeviceBuffer(labels.nbytes).upload(labels), _lib.DeviceBuffer(n).upload(outside)
    guard = np.full(types.size + 128, 77, np.uint8)
    guard[4:4 + types.size] = types.ravel()
    d_types = _lib.DeviceBuffer(guard.nbytes).upload(guard)
    seg.invalidate_cells_dev(d_lab.ptr, d_types.ptr + 4, labels.size, d_out.ptr, n)
    got = d_types.download(guard.shape, np.uint8)
    np.testing.assert_array_equal(got[4:4 + types.size].reshape(types.shape), want)
    assert (got[:4] == 77).all() and (got[4 + types.size:] == 77).all()
    for b in (d_lab, d_out, d_types):
        b.free()


# ---- Tissue ----------------------------------------------------------------------------------------------------------------------
def _tissue(tag, with_types=True, with_labels=True):
    import pandas as pd
    from tissue_image_processing_amd.tissue_info import Tissue
    g = hc.golden()
    n = g["cx_" + tag].size
    info = pd.DataFrame({"label": np.arange(1, n + 1), "cx": g["cx_" + tag], "cy": g["cy_" + tag], "type": g["type_" + tag].astype(np.int64),
                         "valid": g["valid_" + tag].astype(np.int64), "empty_cell": g["empty_cell_" + tag].astype(np.int64)})
    tissue = Tissue(1)
    if with_labels and "labels_" + tag in g.files:
        tissue.set_labels(1, g["labels_" + tag].copy())
    tissue.set_cells_info(1, info)
    if with_types and "types_in_" + tag in g.files:
        tissue.set_cell_types(1, g["types_in_" + tag].copy())
    return tissue


@pytest.mark.parametrize("tag", ("A", "B", "D"))
def test_tissue_methods_equal_the_reference(tag):
    from tissue_image_processing_amd.tissue_info import Tissue
    g = hc.golden()
    tissue = _tissue(tag)
    rows = Tissue.detect_non_sensory_region_cells(tissue.get_cells_info(1))
    np.testing.assert_array_equal(rows, np.flatnonzero(g["outside_" + tag]))
    assert tissue.remove_cells_outside_of_sensory_region(1) == 0
    np.testing.assert_array_equal(tissue.get_cells_info(1)["valid"].to_numpy(), g["valid_out_" + tag])
    if "types_out_" + tag in g.files:
        np.testing.assert_array_equal(tissue.get_cell_types(1), g["types_out_" + tag])
    else:
        assert tissue.get_cell_types(1) is None


def test_tissue_methods_on_a_frame_that_lacks_a_part():
    g = hc.golden()
    no_map = _tissue("B", with_types=False)                            # a table, labels, no type map: valid alone
    assert no_map.remove_cells_outside_of_sensory_region(1) == 0 and no_map.get_cell_types(1) is None
    np.testing.assert_array_equal(no_map.get_cells_info(1)["valid"].to_numpy(), g["valid_out_B"])
    no_labels = _tissue("B", with_labels=False)                        # no labels: 0, and nothing changes
    assert no_labels.remove_cells_outside_of_sensory_region(1) == 0
    np.testing.assert_array_equal(no_labels.get_cells_info(1)["valid"].to_numpy(), g["valid_B"])
    np.testing.assert_array_equal(no_labels.get_cell_types(1), g["types_in_B"])


def test_tissue_raises_where_the_reference_does():
    from tissue_image_processing_amd.tissue_info import Tissue
    assert str(hc.golden()["raises_C"]) == "QhullError"
    with pytest.raises(ValueError):
        Tissue.detect_non_sensory_region_cells(_tissue("C").get_cells_info(1))
    bad = _tissue("A").get_cells_info(1)
    bad.loc[5, "cx"] = np.inf
    with pytest.raises(ValueError):
        Tissue.detect_non_sensory_region_cells(bad)


# ---- the movie driver ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def movie_frames():
    return w.stacks()


def _run(tmp, name, frames, sensory):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        backend, tabs, ids, path = w.run_movie(str(tmp / name), 0, 1, None, sensory, frames=frames)
    try:
        labels = [backend.labels[t].download((w.Y, w.X), np.int32) for t in range(w.T)]
        types = [backend.fetch_cell_types(t) for t in range(w.T)]
        run = dict(path=path, tabs=tabs, ids=ids, labels=labels, types=types, columns=[name for name, _ in backend.extra_columns],
                   hulls=dict(backend.sensory_hulls), skipped=list(backend.sensory_skipped),
                   archive={t: backend.archive_frames[t]["types"] for t in range(w.T)},
                   warnings=[c for c in caught if issubclass(c.category, RuntimeWarning) and "sensory" in str(c.message)])
    finally:
        backend.close()
    return run


@pytest.fixture(scope="module")
def unfiltered(tmp_path_factory, movie_frames):
    return _run(tmp_path_factory.mktemp("sensory"), "plain", movie_frames, False)


@pytest.fixture(scope="module")
def filtered(tmp_path_factory, movie_frames):
    return _run(tmp_path_factory.mktemp("sensory"), "filtered", movie_frames, True)


def _tissue_of(run, t):
    import pandas as pd
    from tissue_image_processing_amd.tissue_info import Tissue
    tab = run["tabs"][t]
    n = tab["area"].size
    info = pd.DataFrame({"label": np.arange(1, n + 1), "cx": tab["cx"], "cy": tab["cy"], "type": tab["type"].astype(np.int64),
                         "valid": tab["valid"].astype(np.int64), "empty_cell": (tab["area"] <= 0).astype(np.int64)})
    tissue = Tissue(1)
    tissue.set_labels(1, run["labels"][t].copy())
    tissue.set_cells_info(1, info)
    tissue.set_cell_types(1, run["types"][t].copy())
    return tissue


def test_movie_filter_equals_the_tissue_method(unfiltered, filtered):
    from tissue_image_processing_amd.tissue_info import Tissue
    assert sorted(filtered["hulls"]) == [t for t in range(w.T) if t != w.TWO_HC_FRAME]
    for t in sorted(filtered["hulls"]):
        tissue = _tissue_of(unfiltered, t)
        outside = Tissue.detect_non_sensory_region_cells(tissue.get_cells_info(1))
        assert 0 < outside.size < tissue.get_cells_info(1).shape[0], "frame %d: the filter has nothing to do" % t
        tissue.remove_cells_outside_of_sensory_region(1)
        got = filtered["tabs"][t]
        assert got["in_sensory_region"].dtype == np.uint8 and got["valid"].dtype == np.uint8
        np.testing.assert_array_equal(got["in_sensory_region"], 1 - np.isin(np.arange(got["area"].size), outside), err_msg="frame %d" % t)
        np.testing.assert_array_equal(got["valid"], tissue.get_cells_info(1)["valid"].to_numpy(), err_msg="frame %d" % t)
        np.testing.assert_array_equal(filtered["types"][t], tissue.get_cell_types(1), err_msg="frame %d" % t)
        assert (filtered["types"][t] != unfiltered["types"][t]).any()
        hair = np.flatnonzero((unfiltered["tabs"][t]["type"] == 1) & (unfiltered["tabs"][t]["valid"] == 1) & (got["area"] > 0))
        assert np.isin(filtered["hulls"][t], hair).all() and filtered["hulls"][t].size >= 3
        for k in ("area", "cy", "cx", "type", "mean_intensity"):       # the filter changes valid and the map, nothing else of the typing
            np.testing.assert_array_equal(got[k], unfiltered["tabs"][t][k])
    # one frame against the rational restatement as well: the geometry, independent of the device entry
    import hull_restate as hr
    plain, got = unfiltered["tabs"][0], filtered["tabs"][0]
    want_outside, want_hull = hr.sensory_region(plain["cx"], plain["cy"], plain["type"], plain["valid"], plain["area"] <= 0)
    np.testing.assert_array_equal(got["in_sensory_region"], 1 - want_outside)
    np.testing.assert_array_equal(filtered["hulls"][0], want_hull)


def test_movie_neighbour_columns_follow_the_filtered_valid(filtered, movie_frames):
    from tissue_image_processing_amd.pipeline import FramePipeline
    pipe = FramePipeline(2, w.Z, w.Y, w.X)
    t = 1
    d = pipe.upload_stack(movie_frames[t])
    pipe.project(d)
    pipe.segment(0)
    tab = pipe.cell_tables()
    d.free()
    got = filtered["tabs"][t]
    np.testing.assert_array_equal(tab["area"], got["area"])
    want = pipe.neighbor_features(got["area"].size, got["valid"], got["type"])
    for name in FramePipeline.NEIGHBOR_COLUMNS + FramePipeline.TYPED_NEIGHBOR_COLUMNS:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    assert (got["valid_neighbors"] != got["n_neighbors"]).any()


def test_movie_archive_shows_the_filtered_frame(filtered):
    from tissue_image_processing_amd.tissue_info import Tissue
    tissue = Tissue(w.T)
    for _ in tissue.load(filtered["path"]):
        pass
    for t in range(w.T):
        np.testing.assert_array_equal(tissue.get_cells_info(t + 1)["valid"].to_numpy(), filtered["tabs"][t]["valid"])
        np.testing.assert_array_equal(tissue.get_cell_types(t + 1), filtered["types"][t])
        np.testing.assert_array_equal(tissue.get_labels(t + 1), filtered["labels"][t])


def test_movie_frame_without_a_hull_is_left_unfiltered(unfiltered, filtered):
    t = w.TWO_HC_FRAME
    plain = unfiltered["tabs"][t]
    assert int(((plain["type"] == 1) & (plain["valid"] == 1) & (plain["area"] > 0)).sum()) == 2
    assert filtered["skipped"] == [t] and t not in filtered["hulls"]
    assert len(filtered["warnings"]) == 1 and "frame %d" % t in str(filtered["warnings"][0].message)
    assert (filtered["tabs"][t]["in_sensory_region"] == 1).all()
    np.testing.assert_array_equal(filtered["tabs"][t]["valid"], plain["valid"])
    np.testing.assert_array_equal(filtered["types"][t], unfiltered["types"][t])
    assert not unfiltered["warnings"] and not unfiltered["skipped"] and not unfiltered["hulls"]


def test_movie_option_off_is_the_code_path_it_was(unfiltered, movie_frames):
    """same columns, same values: the typing call and the neighbour columns recomputed stage by stage on a pipeline"""
    from tissue_image_processing_amd import movie
    from tissue_image_processing_amd.pipeline import FramePipeline
    names = [name for name, _ in movie.GpuFrameBackend.CELL_TYPE_COLUMNS] + list(FramePipeline.NEIGHBOR_COLUMNS + FramePipeline.TYPED_NEIGHBOR_COLUMNS)
    assert unfiltered["columns"] == names
    assert set(names) <= set(unfiltered["tabs"][0]) and "in_sensory_region" not in unfiltered["tabs"][0]
    pipe = FramePipeline(2, w.Z, w.Y, w.X)
    t = 2
    d = pipe.upload_stack(movie_frames[t])
    pipe.project(d)
    pipe.segment(0)
    tab = pipe.cell_tables()
    d.free()
    rows = pipe.cell_types(n=tab["area"].size, **w.CELL_TYPES)
    got = unfiltered["tabs"][t]
    for k in ("type", "valid"):
        np.testing.assert_array_equal(got[k], rows[k])
    np.testing.assert_array_equal(got["mean_intensity"], rows["mean_intensity"])
    np.testing.assert_array_equal(unfiltered["types"][t], pipe.fetch_cell_types())
    want = pipe.neighbor_features(tab["area"].size, rows["valid"], rows["type"])
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def test_movie_option_needs_the_cell_types():
    from tissue_image_processing_amd import movie
    with pytest.raises(ValueError):
        movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0, sensory_region=True)
    with pytest.raises(ValueError):
        movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0, cell_types=dict(w.CELL_TYPES, type_index=1), sensory_region=True)


def test_movie_column_reaches_rank_0_of_two(tmp_path, filtered):
    out = str(tmp_path / "w2")
    run_ranks("_gpu_movie_sensory_worker.py", 2, (out, "1"), timeout=600, local_rank="0")
    a = np.load(out + ".npz")
    assert list(a["columns"]) == filtered["columns"] and "in_sensory_region" in filtered["columns"]
    for t in range(w.T):
        for k in ("valid", "in_sensory_region", "hc_neighbors", "valid_neighbors"):
            np.testing.assert_array_equal(a["%s_%d" % (k, t)], filtered["tabs"][t][k], err_msg="%s, frame %d" % (k, t))
