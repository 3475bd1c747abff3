"""GPU: the frame-sharded movie driver with TWO processes (gloo collectives, both on GPU 0) equals the one-process run;
and the watershed's fallback machinery (wide tile pass + global-minimum commits) gives the same labels as the endgame."""
import numpy as np
import pytest

from gloo_launch import run_ranks

pytestmark = pytest.mark.gpu


def _run(world, out):
    run_ranks("_gpu_movie_worker.py", world, (out,), timeout=600, local_rank="0")


def test_world2_equals_world1(tmp_path):
    o1, o2 = str(tmp_path / "w1.npz"), str(tmp_path / "w2.npz")
    _run(1, o1)
    _run(2, o2)
    a, b = np.load(o1), np.load(o2)
    for t in range(int(a["n"])):
        np.testing.assert_array_equal(a["ids_%d" % t], b["ids_%d" % t])
        np.testing.assert_array_equal(a["area_%d" % t], b["area_%d" % t])
        np.testing.assert_array_equal(a["eids_%d" % t], b["eids_%d" % t])
    # drift estimated by each frame's owner from the neighbour rank's plane: identical in both runs, and close to the
    # synthetic movie's global motion (0.5, -0.3) px/frame undone (the sites also random-walk, so only roughly)
    np.testing.assert_array_equal(a["est"], b["est"])
    print("estimated drifts:", a["est"].tolist())
    assert np.all(np.abs(a["est"][1:] - np.array([-0.5, 0.3])) < 1.0)


def test_watershed_fallback_paths_agree():
    from tissue_image_processing_amd import _segmentation as seg, _lib
    rng = np.random.default_rng(4)
    img = rng.random((150, 170))          # white noise: many lines, many stuck pockets
    ref, f0 = seg.watershed(img, return_flags=True)
    with _lib.tuning(TIP_WS_NO_ENDGAME="1"):
        out, f1 = seg.watershed(img, return_flags=True)
    np.testing.assert_array_equal(out, ref)
    print("pixels finished serially with the endgame disabled:", f1 >> _lib.WS_FLAG_COUNT_SHIFT)


def _groove_image(K=14, H=24, W=41):
    """Two basins left/right of a ridge at the middle column; the ridge column carries a slowly rising GROOVE whose
    flanks rise fast.  The lowest groove pixel becomes a watershed line, every groove pixel above it has that line (or
    a stuck pixel) as its only lower neighbour: a K-cell staircase pocket that is released only when a flank is labelled."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    mid = W // 2
    img = 100.0 - np.abs(x - mid) + 0.001 * y + 0.00037 * x
    img[:, mid - 1] = 99.0 + 2.0 * np.arange(H)
    img[:, mid + 1] = 99.0005 + 2.0 * np.arange(H)
    img[:, mid] = 200.0 + np.arange(H)
    img[0, mid] = 99.5
    img[1:K + 1, mid] = 99.5 + 0.1 * np.arange(1, K + 1)
    return img


def test_watershed_serial_finish():
    """With the endgame and the wide pass disabled a long stuck pocket is a serial dependency chain the tile rounds cannot
    release: the rest of the flood is finished by the host stage (one pass, same pop-time rule) -- same labels, equal to the
    serial oracle, and `flags` says so."""
    from oracle import oracle as orc
    from tissue_image_processing_amd import _segmentation as seg, _lib
    img = _groove_image()
    ref = seg.watershed(img)
    np.testing.assert_array_equal(ref, orc.watershed(img))
    with _lib.tuning(TIP_WS_NO_ENDGAME="1"):
        out_w, flags_w = seg.watershed(img, return_flags=True)           # wide pass available
        np.testing.assert_array_equal(out_w, ref)
        with _lib.tuning(TIP_WS_NO_WIDE="1"):
            out, flags = seg.watershed(img, return_flags=True)            # only the serial finish is left
    np.testing.assert_array_equal(out, ref)
    assert flags & _lib.WS_FLAG_SERIAL_FINISH and flags >> _lib.WS_FLAG_COUNT_SHIFT > 0
    print("pixels finished serially:", flags >> _lib.WS_FLAG_COUNT_SHIFT, "(with the wide pass:", flags_w >> _lib.WS_FLAG_COUNT_SHIFT, ")")
