"""movie.process_movie(local_drifts=...) on CPU: the sharded driver's local-drift mode with a numpy / oracle stand-in for the
device step (tests/_movie_local_worker.py) -- against a direct restatement of the tracker frame by frame, in one process
and gloo worlds of 2 and 4; the single whole-frame window against estimate_drift; the rejected argument combinations."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gloo_launch import run_ranks  # noqa: E402


@pytest.fixture(scope="module")
def frames():
    from _movie_worker import drifting_movie
    return drifting_movie(5)


@pytest.fixture(scope="module")
def restated_ids(frames):
    """The multi-window tracker written out: frame 0's ids as calculate_frame_cellinfo leaves them, then per frame the
    local-drift hits of the previous table against this frame and one assign_track_ids step."""
    from _movie_local_worker import MULTI, local_hits
    from oracle import oracle as orc
    from tissue_image_processing_amd.movie import assign_track_ids
    tabs = []
    for lab, _ in frames:
        rp = orc.regionprops(lab)
        area = rp["area"]
        tabs.append(dict(area=area, cy=np.where(area > 0, rp["cy"], 0.0), cx=np.where(area > 0, rp["cx"], 0.0)))
    n0 = tabs[0]["area"].size
    ids = [assign_track_ids(None, None, n0, start_ids=np.where(tabs[0]["area"] > 0, np.arange(1, n0 + 1), 0))]
    for t in range(1, len(frames)):
        hits, shifts = local_hits(frames[t - 1][1], frames[t][1], frames[t][0], tabs[t - 1], **MULTI)
        assert len(shifts) == 48
        ids.append(assign_track_ids(ids[-1], np.where(tabs[t - 1]["area"] > 0, hits, -1), tabs[t]["area"].size))
    return ids


def test_window_sets_of_the_two_cases(frames):
    from _movie_local_worker import MULTI, SINGLE, windows_of
    from tissue_image_processing_amd._registration import local_drift_windows
    shape = frames[0][0].shape
    assert shape == (144, 168)
    multi = local_drift_windows(shape, **MULTI)
    assert multi == windows_of(shape, **MULTI) and len(multi) == 48
    assert len(set((r1 - r0, c1 - c0) for r0, r1, c0, c1 in multi)) == 2
    assert local_drift_windows(shape, **SINGLE) == [(0, 144, 0, 168)]


def test_local_drift_hits_is_the_mean_and_lookup_rule():
    """movie.local_drift_hits on hand-made window shifts: sums in loop order and one division, round(cy - d_row) /
    round(cx - d_col), -1 for a point no window contains."""
    from tissue_image_processing_amd.movie import local_drift_hits
    drifts = [((0, 10, 0, 10), 1.0, -2.0), ((5, 15, 0, 10), 2.0, 0.5), ((0, 10, 5, 20), 0.25, 0.25)]
    tab = dict(area=np.array([4, 4, 4, 4]), cy=np.array([2.4, 7.0, 7.5, 17.0]), cx=np.array([3.0, 7.0, 2.0, 3.0]))
    seen = {}

    def lookup(qy, qx):
        seen["q"] = (qy.copy(), qx.copy())
        return np.arange(10, 10 + qy.size).astype(np.int32)

    hits = local_drift_hits(drifts, tab, lookup)
    # row 0: window 0 only; row 1 (7, 7): all three; row 2: round(7.5) = 8, (8, 2): windows 0 and 1; row 3: none
    d_row = [1.0, ((1.0 + 2.0) + 0.25) / 3, (1.0 + 2.0) / 2]
    d_col = [-2.0, ((-2.0 + 0.5) + 0.25) / 3, (-2.0 + 0.5) / 2]
    np.testing.assert_array_equal(seen["q"][0][:3], np.round(tab["cy"][:3] - d_row).astype(np.int64))
    np.testing.assert_array_equal(seen["q"][1][:3], np.round(tab["cx"][:3] - d_col).astype(np.int64))
    np.testing.assert_array_equal(hits, [10, 11, 12, -1])
    assert hits.dtype == np.int32


def test_single_process_matches_the_restatement(frames, restated_ids):
    from _movie_local_worker import MULTI, LocalOracleBackend
    from tissue_image_processing_amd import movie
    drifts = np.zeros((len(frames), 2))
    drifts[1:] = (0.25, -0.5)                 # the local-drift mode ignores them and leaves them in the tables
    backend = LocalOracleBackend(144, 168)
    tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], backend, 0, 1, None, "cpu", drifts, local_drifts=MULTI)
    for t in range(len(frames)):
        np.testing.assert_array_equal(ids[t], restated_ids[t])
        np.testing.assert_array_equal(tabs[t]["drift"], drifts[t])
    assert sorted(backend.local_drifts) == [1, 2, 3, 4] and all(len(v) == 48 for v in backend.local_drifts.values())


@pytest.mark.parametrize("world,block", [(2, 0), (2, 1), (4, 0), (4, 1)])
def test_gloo_worlds_match_the_restatement(tmp_path, restated_ids, world, block):
    out = str(tmp_path / "w.npz")
    run_ranks("_movie_local_worker.py", world, (out, "multi", block), timeout=300)
    a = np.load(out)
    assert int(a["n"]) == 5
    np.testing.assert_array_equal(a["drifts"], np.zeros((5, 2)))
    for t in range(5):
        np.testing.assert_array_equal(a["ids_%d" % t], restated_ids[t])


def test_single_whole_frame_window_equals_estimate_drift(frames):
    """One window that is the whole frame: the mean of one shift is the shift, every centroid lies in the window -- the ids
    and the tables' columns are those of estimate_drift=True.  The "drift" entry is the one difference the mode defines: it
    keeps the given rows, and the estimate stays on the owner, where it equals estimate_drift's."""
    from _movie_local_worker import SINGLE, LocalOracleBackend
    from tissue_image_processing_amd import movie
    T = len(frames)
    etabs, eids = movie.process_movie(T, lambda t: frames[t], LocalOracleBackend(144, 168), 0, 1, None, "cpu", estimate_drift=True)
    backend = LocalOracleBackend(144, 168)
    tabs, ids = movie.process_movie(T, lambda t: frames[t], backend, 0, 1, None, "cpu", local_drifts=SINGLE)
    for t in range(T):
        np.testing.assert_array_equal(ids[t], eids[t])
        assert sorted(tabs[t]) == sorted(etabs[t])
        for col in ("area", "cy", "cx"):
            np.testing.assert_array_equal(tabs[t][col], etabs[t][col])
        np.testing.assert_array_equal(tabs[t]["drift"], [0.0, 0.0])
        if t >= 1:
            assert backend.local_drifts[t] == [tuple(etabs[t]["drift"])]


class _NoPlanes(object):
    keep_planes = False
    Y, X = 144, 168

    def local_drift_lookup(self, t, prev_plane, prev_table, step_size=100, window_size=700):   # pragma: no cover
        raise AssertionError


class _NoExtents(object):
    def local_drift_lookup(self, t, prev_plane, prev_table, step_size=100, window_size=700):   # pragma: no cover
        raise AssertionError


def _backend(kind):
    from _movie_local_worker import LocalOracleBackend
    from _movie_worker import OracleBackend
    return {"local": lambda: LocalOracleBackend(144, 168), "oracle": OracleBackend, "no_planes": _NoPlanes,
            "no_extents": _NoExtents}[kind]()


@pytest.mark.parametrize("kw,backend", [
    (dict(local_drifts=True, estimate_drift=True), "local"),
    (dict(local_drifts=True, use_piv=True), "local"),
    (dict(local_drifts=dict(window_size=48), stitcher="linker"), "local"),
    (dict(local_drifts=dict(window_size=48)), "oracle"),                     # no local_drift_lookup
    (dict(local_drifts=dict(window_size=48)), "no_planes"),                  # keep_planes=False
    (dict(local_drifts=dict(window_size=48)), "no_extents"),
    (dict(local_drifts=dict(window_size=48, step=16)), "local"),             # unknown key
    (dict(local_drifts="yes"), "local"),
    (dict(local_drifts=True), "local"),                                      # 144 x 168 does not exceed 700
    (dict(local_drifts=dict(window_size=144)), "local"),                     # rows do not exceed the window
    (dict(local_drifts=dict(window_size=150)), "local"),
])
def test_rejected_combinations(kw, backend):
    from tissue_image_processing_amd import movie
    calls = []

    def source(t):
        calls.append(t)
        raise AssertionError("no frame may be computed")

    with pytest.raises(ValueError):
        movie.process_movie(3, source, _backend(backend), 0, 1, None, "cpu", **kw)
    assert calls == []


def test_local_drifts_none_is_unchanged(golden):
    """local_drifts=None (the default) is the drift path, exactly as before."""
    from _movie_worker import OracleBackend
    from tissue_image_processing_amd import movie
    g = golden("tracking")
    labs = list(g["labels"])
    drifts = np.zeros((3, 2))
    drifts[1:] = (0.5, -0.3)
    _, ids = movie.process_movie(3, lambda t: labs[t], OracleBackend(), 0, 1, None, "cpu", drifts, local_drifts=None)
    for t in range(3):
        np.testing.assert_array_equal(ids[t], g["ids_%d" % t])
