"""GPU: track linking on the device (csrc/tip_link.hip, linking.DeviceFrameLinker, process_movie(stitcher="device_linker")).
The reference is the host linker, linking.FrameLinker, on the same input; particle numbers are compared exactly in every
frame.  test_link_cases_host.py shows that the cases' optima have a margin far above rounding, so an exact solver with another
order of operations must find the same links."""
import numpy as np
import pytest

import link_cases as lc
from gpu_util import launches
from tissue_image_processing_amd import linking

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -2, -5


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _device_run(frames, **kw):
    lk = linking.DeviceFrameLinker(**kw)
    ids, stats = [], []
    for f in frames:
        ids.append(lk.link(f))
        stats.append(lk.last_stats)
    return ids, stats


def _call(lib_fn, tracks, points, search_range=100.0, stop=10.0, step=0.95, max_subnet=30):
    """The host-pointer entry on (n_tracks, 3) and (n, 3) arrays -> (status, track_of_feature, stats)."""
    from tissue_image_processing_amd import _lib
    tracks, points = np.ascontiguousarray(tracks, np.float64), np.ascontiguousarray(points, np.float64)
    out, stats = np.full(points.shape[0], -7, np.int32), np.full(6, -7, np.int64)
    rc = lib_fn(_lib.ptr(tracks), tracks.shape[0], _lib.ptr(points), points.shape[0], search_range, stop, step, max_subnet,
                _lib.ptr(out), _lib.ptr(stats))
    return rc, out, stats


# ---- movies ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.MOVIES))
def test_movie_ids_equal_the_host_linkers(name):
    ids, stats = _device_run(lc.frames_of(name))
    assert stats[0] is None and all(s is not None and s["oversize"] == 0 and s["links"] > 0 for s in stats[1:])
    print(name, stats[1:])
    assert _same(ids, lc.host_ids(name))
    if name == "B":
        assert max(s["rounds"] for s in stats[1:]) > 1


def test_shifted_coordinates():
    """Negative and large coordinates (cumulative drift): movie A moved by (-250.5, +1.0e5)."""
    frames = lc.shifted(lc.frames_of("A"), -250.5, 1.0e5)
    assert _same(_device_run(frames)[0], lc.run(linking.FrameLinker(), frames))


def _grid_doublings(points, h):
    """How often the grid kernel doubles the cell side h for these features (its own loop, on the CPU), and the final side."""
    fin = points[np.isfinite(points).all(axis=1)]
    H, W = np.ptp(fin[:, 0]), np.ptp(fin[:, 1])
    doublings = 0
    while (np.floor(H / h) + 1.0) * (np.floor(W / h) + 1.0) > points.shape[0] + 4:
        h, doublings = 2.0 * h, doublings + 1
    return doublings, h


def test_far_apart_copies_double_the_grid_cell():
    """Movie B next to a copy of itself 3.0e6 / 2.0e6 away: cells of side search_range would outnumber the features, so the grid
    kernel doubles h twelve times (no other link test doubles it at all); the host linker is the reference as everywhere."""
    frames = [np.concatenate([f, f + np.array([3.0e6, -2.0e6, 0.0])]) for f in lc.frames_of("B")]
    assert all(_grid_doublings(f, 100.0) == (12, 409600.0) for f in frames)
    assert all(_grid_doublings(f, 100.0)[0] == 0 for name in ("A", "B") for f in lc.frames_of(name))
    ids, stats = _device_run(frames)
    assert stats[0] is None and all(s is not None and s["oversize"] == 0 and s["links"] > 0 for s in stats[1:])
    assert _same(ids, lc.run(linking.FrameLinker(), frames))


# ---- edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [1, 4], ids=["inside_memory", "outside_memory"])
def test_empty_frames_between_points(gap):
    a = lc.frames_of("A")
    frames = [a[0]] + [np.zeros((0, 3))] * gap + [a[1]]
    ref = lc.run(linking.FrameLinker(), frames)
    assert (ref[-1].min() < a[0].shape[0]) == (gap == 1)        # the tracks are remembered over 1 empty frame, forgotten over 4
    assert _same(_device_run(frames)[0], ref)


def test_no_tracks_and_no_features():
    from tissue_image_processing_amd import _lib
    lib = _lib.lib()
    pts = lc.frames_of("B")[0]
    rc, out, stats = _call(lib.tip_link_frame_f64, np.zeros((0, 3)), pts)
    assert rc == 0 and (out == -1).all() and stats[:4].tolist() == [0, 0, 0, 0] and stats[5] == 0
    rc, out, stats = _call(lib.tip_link_frame_f64, pts, np.zeros((0, 3)))
    assert rc == 0 and out.size == 0 and stats[0] == 0
    # ... also with null pointers for the empty side
    out = np.full(pts.shape[0], -7, np.int32)
    assert lib.tip_link_frame_f64(None, 0, _lib.ptr(pts), pts.shape[0], 100.0, 10.0, 0.95, 30, _lib.ptr(out), None) == 0
    assert (out == -1).all()
    assert lib.tip_link_frame_f64(_lib.ptr(pts), pts.shape[0], None, 0, 100.0, 10.0, 0.95, 30, None, None) == 0


def test_subnet_assignment_is_globally_optimal_not_greedy():
    # test_linking.py's case: the greedy nearest link (a->x) forces b->y (sum d^2 = 82); the optimum is a->y, b->x (50)
    lk = linking.DeviceFrameLinker(search_range=50, adaptive_stop=None)
    ids0 = lk.link(linking.embed([0.0, 0.0], [0.0, 6.0], [800, 800]))
    ids1 = lk.link(linking.embed([0.0, 0.0], [1.0, -5.0], [800, 800]))
    assert ids1[0] == ids0[1] and ids1[1] == ids0[0]
    assert lk.last_stats["subnets"] == 1 and lk.last_stats["largest_subnet"] == 2 and lk.last_stats["rounds"] == 1


def test_memory_relinks_after_a_gap_and_forgets_after_it():
    base = np.array([[10.0, 10.0, 800.0], [200.0, 200.0, 900.0]])
    both = linking.embed(base[:, 0], base[:, 1], base[:, 2])
    only_first = linking.embed(base[:1, 0], base[:1, 1], base[:1, 2])
    moved = linking.embed(base[:, 0] + 1, base[:, 1], base[:, 2])
    for memory, frames in ((2, [both, only_first, only_first, moved]), (1, [both, only_first, only_first, both])):
        ref = lc.run(linking.FrameLinker(search_range=20, memory=memory), frames)
        assert (ref[-1][1] == ref[0][1]) == (memory == 2)
        assert _same(_device_run(frames, search_range=20, memory=memory)[0], ref)


def test_range_is_inclusive():
    """A track at (0, 0) and a feature at (60, 80) with equal areas: d == 100 == search_range is a link; 80.000001 is not."""
    first = linking.embed([0.0], [0.0], [900.0])
    lk = linking.DeviceFrameLinker(search_range=100)
    assert lk.link(first).tolist() == [0]
    assert lk.link(linking.embed([60.0], [80.0], [900.0])).tolist() == [0]
    assert lk.last_stats["links"] == 1
    lk = linking.DeviceFrameLinker(search_range=100)
    lk.link(first)
    assert lk.link(linking.embed([60.0], [80.000001], [900.0])).tolist() == [1]
    assert lk.last_stats["links"] == 0


# ---- subnet size -----------------------------------------------------------------------------------------------------------------
def test_cluster_of_30_is_solved_in_the_first_round():
    lk = linking.DeviceFrameLinker()
    alone = lc.cluster_frames(30, with_a=False)
    ids = lc.run(lk, alone)
    assert lk.last_stats == dict(links=900, rounds=1, subnets=1, largest_subnet=30, final_range=100.0, oversize=0)
    assert _same(ids, lc.run(linking.FrameLinker(), alone))
    assert _same(_device_run(lc.cluster_frames(30))[0], lc.cluster_host_ids(30))      # with movie A's cells far away from it


def test_cluster_of_31_needs_the_adaptive_search():
    lk = linking.DeviceFrameLinker()
    alone = lc.cluster_frames(31, with_a=False)
    ids = lc.run(lk, alone)
    assert lk.last_stats["links"] == 961 and lk.last_stats["rounds"] > 1 and lk.last_stats["final_range"] < 100.0
    assert lk.last_stats["largest_subnet"] <= 30
    assert _same(ids, lc.run(linking.FrameLinker(), alone))
    assert _same(_device_run(lc.cluster_frames(31))[0], lc.cluster_host_ids(31))


# ---- oversize --------------------------------------------------------------------------------------------------------------------
def _host_error(frames, **kw):
    lk = linking.FrameLinker(**kw)
    lk.link(frames[0])
    with pytest.raises(linking.SubnetOversizeError) as e:
        lk.link(frames[1])
    return str(e.value)


@pytest.mark.parametrize("stop", [None, 90], ids=["no_adaptive_search", "stop_reached"])
def test_oversize_is_the_host_linkers_error_and_leaves_no_state(stop):
    frames = lc.oversize_frames()
    lk = linking.DeviceFrameLinker(search_range=100, adaptive_stop=stop)
    lk.link(frames[0])
    with pytest.raises(linking.SubnetOversizeError) as e:
        lk.link(frames[1])
    assert str(e.value) == _host_error(frames, search_range=100, adaptive_stop=stop)
    assert lk.last_stats["oversize"] == (1 if stop is None else 2)
    a = lc.frames_of("A")[:2]
    assert _same(_device_run(a)[0], lc.host_ids("A")[:2])        # an ordinary call on the same thread afterwards


def test_oversize_subnets_shrink_the_range():
    frames = lc.oversize_frames()
    ids, stats = _device_run(frames, search_range=100, adaptive_stop=2)
    assert np.array_equal(ids[0], ids[1])
    assert stats[1]["rounds"] > 1
    assert _same(ids, lc.run(linking.FrameLinker(search_range=100, adaptive_stop=2), frames))


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def _second_frame_of_a():
    lk = linking.FrameLinker()
    a = lc.frames_of("A")
    lk.link(a[0])
    return np.ascontiguousarray(lk.track_pos), np.ascontiguousarray(a[1])


def _call_dev(tracks, points):
    """The device-pointer entry on (n_tracks, 3) and (n, 3) arrays -> (track_of_feature, stats)."""
    from tissue_image_processing_amd import _lib
    lib = _lib.lib()
    n = points.shape[0]
    d_t, d_p = _lib.DeviceBuffer(tracks.nbytes).upload(tracks), _lib.DeviceBuffer(points.nbytes).upload(points)
    d_out, d_stats = _lib.DeviceBuffer(n * 4), _lib.DeviceBuffer(6 * 8)
    try:
        _lib.check(lib.tip_link_frame_f64_dev(_lib.dptr(d_t.ptr), tracks.shape[0], _lib.dptr(d_p.ptr), n, 100.0, 10.0, 0.95, 30,
                                              _lib.dptr(d_out.ptr), _lib.dptr(d_stats.ptr)))
        _lib.check(lib.tip_sync())
        return d_out.download((n,), np.int32), d_stats.download((6,), np.int64)
    finally:
        for b in (d_t, d_p, d_out, d_stats):
            b.free()


def test_device_pointer_form_equals_the_host_pointer_form():
    from tissue_image_processing_amd import _lib
    tracks, points = _second_frame_of_a()
    rc, ref, ref_stats = _call(_lib.lib().tip_link_frame_f64, tracks, points)
    assert rc == 0 and ref.max() >= 0 and ref.min() >= -1
    out, stats = _call_dev(tracks, points)
    assert np.array_equal(out, ref)
    assert np.array_equal(stats, ref_stats)


def test_device_pointer_form_leaves_non_finite_rows_out():
    """The host form refuses non-finite rows; the device-pointer form cannot look, so its kernels skip them: a NaN feature gets
    no track, a track at cx = +inf gets no feature, and everything else is the call without those two rows."""
    tracks, points = _second_frame_of_a()
    clean, _ = _call_dev(tracks, points)
    linked = np.flatnonzero(clean >= 0)
    bad_f, bad_t = int(linked[0]), int(clean[linked[1]])                       # (both rows take part in the untouched call)
    bad_tracks, bad_points = tracks.copy(), points.copy()
    bad_points[bad_f] = np.nan
    bad_tracks[bad_t, 1] = np.inf
    out, stats = _call_dev(bad_tracks, bad_points)
    ref, ref_stats = _call_dev(np.delete(tracks, bad_t, axis=0), np.delete(points, bad_f, axis=0))
    ref = np.where(ref >= bad_t, ref + 1, ref)                                 # track numbers of the full table
    assert out[bad_f] == -1
    assert np.array_equal(np.delete(out, bad_f), ref)
    assert stats[0] == ref_stats[0] and stats[0] > 0


def test_argument_errors_come_back_without_a_launch():
    from tissue_image_processing_amd import _lib
    lib = _lib.lib()
    tracks, points = _second_frame_of_a()
    out = np.zeros(points.shape[0], np.int32)
    with launches() as ran:
        for fn in (lib.tip_link_frame_f64, lib.tip_link_frame_f64_dev):
            assert fn(None, tracks.shape[0], _lib.ptr(points), points.shape[0], 100.0, 10.0, 0.95, 30, _lib.ptr(out), None) == ERR_ARG
            assert fn(_lib.ptr(tracks), tracks.shape[0], _lib.ptr(points), points.shape[0], 100.0, 10.0, 0.95, 30, None, None) == ERR_ARG
            assert fn(_lib.ptr(tracks), -1, _lib.ptr(points), points.shape[0], 100.0, 10.0, 0.95, 30, _lib.ptr(out), None) == ERR_ARG
            assert _call(fn, tracks, points, search_range=0.0)[0] == ERR_ARG
            assert _call(fn, tracks, points, step=1.0)[0] == ERR_ARG
            assert _call(fn, tracks, points, step=0.0)[0] == ERR_ARG
            assert _call(fn, tracks, points, max_subnet=31)[0] == ERR_UNSUPPORTED
            assert _call(fn, tracks, points, max_subnet=0)[0] == ERR_UNSUPPORTED
        bad = points.copy()
        bad[3, 1] = np.nan
        assert _call(lib.tip_link_frame_f64, tracks, bad)[0] == ERR_ARG
        assert "feature 3" in _lib.last_error()
    assert not [k for k in ran if k.startswith("link_")], ran


def test_smaller_max_subnet_is_honoured():
    """max_subnet below 30: the 30-cluster is then too large for one round."""
    from tissue_image_processing_amd import _lib
    tracks, points = lc.cluster_frames(30, with_a=False)
    rc, out, stats = _call(_lib.lib().tip_link_frame_f64, tracks, points, max_subnet=29)
    assert rc == 0 and stats[1] > 1 and stats[3] <= 29 and stats[5] == 0


# ---- callers ---------------------------------------------------------------------------------------------------------------------
def test_process_movie_device_linker_equals_linker():
    from tissue_image_processing_amd import synthetic, movie
    Z, Y, X, T = 8, 256, 256, 6
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    stacks = [synthetic.make_stack(Z, Y, X, seed=50 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]
    drifts = np.zeros((T, 2))
    drifts[1:] = (0.5, -0.3)
    results = {}
    for stitcher in ("linker", "device_linker"):
        for block in (1, None):
            backend = movie.GpuFrameBackend(2, Z, Y, X, device=0)
            try:
                with launches() as ran:
                    results[stitcher, block] = movie.process_movie(T, lambda t: stacks[t], backend, drifts=drifts, stitcher=stitcher,
                                                                   block_frames=block)
            finally:
                backend.close()
            assert ("link_solve" in ran) == (stitcher == "device_linker")
    ref_tabs, ref_ids = results["linker", None]
    assert len(ref_ids) == T and max(i.max() for i in ref_ids) > 0
    for key, (tabs, ids) in results.items():
        assert _same(ids, ref_ids), key
        for t in range(T):
            assert sorted(tabs[t]) == sorted(ref_tabs[t])
            for col in ref_tabs[t]:
                np.testing.assert_array_equal(tabs[t][col], ref_tabs[t][col], err_msg="%s frame %d %s" % (key, t, col))


def _tracked_tissue():
    """The small movie of test_linking.py::test_tissue_method_labels_tracks_across_frames, tracked; the labels per frame."""
    from tissue_image_processing_amd.tissue_info import Tissue, make_df, CELL_INFO_SPECS
    rng = np.random.default_rng(5)
    n, T = 150, 4
    pts, area = rng.uniform(0, 500.0, (n, 2)), rng.uniform(500, 1500, n)
    tis = Tissue(T)
    tis.drifts[1:] = np.array([0.5, -0.3])
    for t in range(T):
        if t:
            perm = rng.permutation(n)
            pts = pts[perm] + rng.normal(0, 0.7, pts.shape) - np.array([0.5, -0.3])
            area = area[perm]
        df = make_df(n, CELL_INFO_SPECS).astype({"cy": float, "cx": float, "area": float})
        df.loc[:, "cy"], df.loc[:, "cx"], df.loc[:, "area"] = pts[:, 0], pts[:, 1], area
        df.loc[:, "valid"], df.loc[:, "empty_cell"] = 1, 0
        df.loc[:, "label"] = np.arange(1, n + 1)
        tis.set_cells_info(t + 1, df)
    assert tis.track_cells_with_trackpy() == T
    return [tis.get_cells_info(t + 1).label.to_numpy().copy() for t in range(T)]


def test_tissue_method_tracks_on_the_device_when_asked(monkeypatch):
    monkeypatch.setenv("TISSUE_HIP_LINKER", "host")
    with launches() as ran_host:
        ref = _tracked_tissue()
    monkeypatch.setenv("TISSUE_HIP_LINKER", "device")
    with launches() as ran_device:
        got = _tracked_tissue()
    assert "link_solve" not in ran_host and "link_solve" in ran_device
    assert np.array_equal(ref[0], np.arange(1, 151))
    assert _same(got, ref)
