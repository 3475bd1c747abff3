"""GPU: the sharded movie driver's local-drift mode.  GpuFrameBackend.local_drift_lookup against hits assembled from the
per-window comparator (tip_memcpy2d_d2d + phase_cross_correlation_dev), the mean rule in numpy and backend.lookup; the single
whole-frame window against estimate_drift; two processes (both on GPU 0, gloo collectives) against one."""
import numpy as np
import pytest

from gloo_launch import run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    from _movie_worker import drifting_movie
    return drifting_movie(4)


def _backend(frames):
    from _gpu_movie_piv_worker import installed_backend_class
    return installed_backend_class()(*frames[0][0].shape)


def test_local_drift_lookup_equals_the_assembled_hits(frames):
    from _gpu_movie_local_worker import MULTI
    from test_gpu_local_drift_batch import _Frames, loop_shifts
    from tissue_image_processing_amd._registration import local_drift_windows
    backend = _backend(frames)
    try:
        tab0 = backend.process_frame(0, frames[0])
        backend.process_frame(1, frames[1])
        hits = backend.local_drift_lookup(1, backend.plane(0), tab0, **MULTI)
        # the comparator's shift per window, then the mean of the windows that contain the rounded centroid
        windows = local_drift_windows(frames[0][1].shape, **MULTI)
        assert len(windows) == 48
        with _Frames(frames[0][1], frames[1][1]) as fr:
            shifts = [loop_shifts(fr, [(r0, c0, r0, c0)], r1 - r0, c1 - c0)[0] for r0, r1, c0, c1 in windows]
        assert backend.local_drifts[1] == [(w, float(s[0]), float(s[1])) for w, s in zip(windows, shifts)]
        cy, cx = tab0["cy"], tab0["cx"]
        rows, cols = np.round(cy).astype(np.int64), np.round(cx).astype(np.int64)
        s_row, s_col, cnt = np.zeros(cy.shape), np.zeros(cy.shape), np.zeros(cy.shape)
        for (r0, r1, c0, c1), sh in zip(windows, shifts):
            inside = (rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1)
            s_row[inside] += sh[0]
            s_col[inside] += sh[1]
            cnt[inside] += 1
        assert cnt.min() >= 1                      # (the windows cover this frame)
        want = backend.lookup(1, np.round(cy - s_row / cnt).astype(np.int64), np.round(cx - s_col / cnt).astype(np.int64))
        assert hits.dtype == np.int32
        np.testing.assert_array_equal(hits, want)
        assert (hits > 0).any()
    finally:
        backend.close()


def test_single_window_equals_estimate_drift(frames):
    from _gpu_movie_local_worker import SINGLE
    from tissue_image_processing_amd import movie
    T = len(frames)
    be, bl = _backend(frames), _backend(frames)
    try:
        etabs, eids = movie.process_movie(T, lambda t: frames[t], be, 0, 1, None, "cpu", estimate_drift=True)
        tabs, ids = movie.process_movie(T, lambda t: frames[t], bl, 0, 1, None, "cpu", local_drifts=SINGLE)
        for t in range(T):
            np.testing.assert_array_equal(ids[t], eids[t])
            np.testing.assert_array_equal(tabs[t]["drift"], [0.0, 0.0])
            if t >= 1:
                assert bl.local_drifts[t] == [((0, 144, 0, 168), etabs[t]["drift"][0], etabs[t]["drift"][1])]
    finally:
        be.close()
        bl.close()


def test_world2_equals_world1(tmp_path):
    o1, o2 = str(tmp_path / "w1.npz"), str(tmp_path / "w2.npz")
    run_ranks("_gpu_movie_local_worker.py", 1, (o1,), timeout=300, local_rank="0")
    run_ranks("_gpu_movie_local_worker.py", 2, (o2,), timeout=300, local_rank="0")
    a, b = np.load(o1), np.load(o2)
    assert int(a["n"]) == int(b["n"]) == 4
    for t in range(4):
        np.testing.assert_array_equal(a["ids_%d" % t], b["ids_%d" % t])
