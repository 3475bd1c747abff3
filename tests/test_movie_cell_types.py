"""CPU (gloo): process_movie carries a backend's per-row cell-type columns (type, valid, mean_intensity) through the per-round
all-gather, so rank 0's tables hold them at any world size; without them the tables are what they were."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gloo_launch import run_ranks  # noqa: E402

BASE_KEYS = ["area", "cx", "cy", "drift"]
TYPE_KEYS = ["mean_intensity", "type", "valid"]


def _run(world, out, n_frames, block=0, typed=1):
    run_ranks("_movie_celltypes_worker.py", world, (out, n_frames, block, typed), timeout=300)
    return np.load(out)


def _assert_same(a, b, n, keys):
    for t in range(n):
        np.testing.assert_array_equal(a["ids_%d" % t], b["ids_%d" % t])
        assert list(a["keys_%d" % t]) == list(b["keys_%d" % t]) == keys
        for k in keys:
            x, y = a["%s_%d" % (k, t)], b["%s_%d" % (k, t)]
            assert x.dtype == y.dtype, (k, t, x.dtype, y.dtype)
            np.testing.assert_array_equal(x, y)          # (NaN == NaN here: absent rows' mean_intensity)


def test_world1_tables_hold_the_numpy_types():
    from _movie_worker import TypingBackend, numpy_cell_types, typed_movie
    from tissue_image_processing_amd import movie
    frames = typed_movie(4)
    tabs, _ = movie.process_movie(4, lambda t: frames[t], TypingBackend(True), 0, 1, None, "cpu")
    for t, (lab, marker) in enumerate(frames):
        typ, valid, mean = numpy_cell_types(lab, marker, threshold=0.4)
        np.testing.assert_array_equal(tabs[t]["type"], typ)
        np.testing.assert_array_equal(tabs[t]["valid"], valid)
        np.testing.assert_array_equal(tabs[t]["mean_intensity"], mean)
    # the movie exercises both outcomes, absent rows and the single-pixel label
    allt = np.concatenate([tb["type"] for tb in tabs])
    assert (allt == 1).any() and (allt == 0).any()
    assert np.isnan(tabs[0]["mean_intensity"][4]) and tabs[0]["area"][-1] == 1


def test_type_columns_survive_the_gather(tmp_path):
    """world 2 and 4 equal world 1 for every column, with uneven shards (7 frames) and rounds of 1 and 2 frames per rank
    (world 4, block 1: the second round leaves rank 3 without a frame)."""
    n = 7
    ref = _run(1, str(tmp_path / "w1.npz"), n)
    for world, block in ((2, 0), (2, 1), (4, 1), (4, 2)):
        got = _run(world, str(tmp_path / ("w%d_b%d.npz" % (world, block))), n, block)
        assert int(got["n"]) == n
        _assert_same(ref, got, n, BASE_KEYS + TYPE_KEYS)


def test_fewer_frames_than_ranks(tmp_path):
    ref = _run(1, str(tmp_path / "w1.npz"), 3)
    got = _run(4, str(tmp_path / "w4.npz"), 3, 1)
    _assert_same(ref, got, 3, BASE_KEYS + TYPE_KEYS)


def test_untyped_tables_are_unchanged(tmp_path):
    """A backend without extra columns: rank 0's tables have exactly the keys and values they had, and the track ids are
    those of the typed run (typing does not touch the tracker)."""
    n = 7
    plain1 = _run(1, str(tmp_path / "p1.npz"), n, typed=0)
    plain2 = _run(2, str(tmp_path / "p2.npz"), n, 1, typed=0)
    _assert_same(plain1, plain2, n, BASE_KEYS)
    typed2 = _run(2, str(tmp_path / "t2.npz"), n, 1)
    for t in range(n):
        np.testing.assert_array_equal(plain2["ids_%d" % t], typed2["ids_%d" % t])
        for k in BASE_KEYS:
            np.testing.assert_array_equal(plain2["%s_%d" % (k, t)], typed2["%s_%d" % (k, t)])


def test_backend_rejects_unknown_typing_options():
    """Misspelt options fail when the backend is made (before any device work), not on the first frame."""
    from tissue_image_processing_amd import movie
    with pytest.raises(ValueError, match="percentage_above"):
        movie.GpuFrameBackend(2, 1, 8, 8, cell_types=dict(percentage_above=3))
