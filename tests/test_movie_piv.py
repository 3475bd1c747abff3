"""movie.process_movie(use_piv=True) on CPU: the sharded driver's PIV mode with a numpy stand-in for the device step
(tests/_movie_worker.py), against the reference's own use_piv run (tests/golden/piv_tracking.npz), one process and
gloo worlds of 2 and 4, the IndexError protocol and the rejected argument combinations."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gloo_launch import run_ranks  # noqa: E402


def _run(world, out, mode="golden", block=0, timeout=300):
    """`world` gloo ranks of _movie_piv_worker.py (an IndexError is written to out.rank<r>.err, not raised out of the process)."""
    run_ranks("_movie_piv_worker.py", world, (out, mode, block), timeout=timeout)


def test_piv_hits_restatement_pins_the_transposed_sampling():
    """The numpy statement the stand-in and the GPU tests use: the ROW flow is read at (round(cx), round(cy)) and moves cx,
    the column flow moves cy; the moved point is looked up at (round(cy), round(cx)); absent rows give -1."""
    from _movie_worker import piv_hits
    flow = np.zeros((2, 8, 8), np.float32)
    flow[0, 2, 5] = -4.0            # at (row = round(cx) = 2, col = round(cy) = 5): cx 2 -> 6
    flow[1, 2, 5] = 4.0             # cy 5 -> 1
    tab = dict(area=np.array([3, 0]), cy=np.array([5.0, 5.0]), cx=np.array([2.0, 2.0]))
    lab = np.zeros((8, 8), np.int32)
    lab[1, 6] = 7                   # (cy, cx) = (1, 6)
    np.testing.assert_array_equal(piv_hits(flow, lab, tab), [7, -1])
    lab = lab.T.copy()              # (6, 1): where an untransposed sampling would land
    np.testing.assert_array_equal(piv_hits(flow, lab, tab), [0, -1])


def test_single_process_matches_reference_use_piv(golden):
    from _movie_worker import PivOracleBackend, golden_frames
    from tissue_image_processing_amd import movie
    g = golden("piv_tracking")
    frames = golden_frames()
    drifts = np.zeros((len(frames), 2))
    drifts[1:] = (0.25, -0.5)                 # the PIV branch ignores them and leaves them in the tables
    tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], PivOracleBackend(), 0, 1, None, "cpu", drifts,
                                    use_piv=True)
    for t in range(len(frames)):
        np.testing.assert_array_equal(ids[t], g["flow_ids_%d" % t])
        np.testing.assert_array_equal(tabs[t]["drift"], drifts[t])


@pytest.mark.parametrize("world,block", [(2, 0), (2, 1), (4, 0), (4, 1)])
def test_gloo_worlds_match_reference_use_piv(tmp_path, golden, world, block):
    g = golden("piv_tracking")
    out = str(tmp_path / "w.npz")
    _run(world, out, block=block)
    a = np.load(out)
    assert int(a["n"]) == 4
    np.testing.assert_array_equal(a["drifts"], np.zeros((4, 2)))
    for t in range(4):
        np.testing.assert_array_equal(a["ids_%d" % t], g["flow_ids_%d" % t])


def test_single_process_non_square_raises_index_error():
    from _movie_worker import PivOracleBackend, golden_frames
    from tissue_image_processing_amd import movie
    frames = golden_frames(crop=True)
    with pytest.raises(IndexError, match="out of bounds for axis 0 with size 64"):
        movie.process_movie(len(frames), lambda t: frames[t], PivOracleBackend(), 0, 1, None, "cpu", use_piv=True)


def test_world2_non_square_raises_on_every_rank(tmp_path):
    """Rank 1 owns the failing frame 1; rank 0 has nothing to sample but must raise too, and neither may hang."""
    out = str(tmp_path / "crop.npz")
    _run(2, out, mode="crop", timeout=120)
    assert not os.path.exists(out)
    msgs = [open("%s.rank%d.err" % (out, r)).read() for r in range(2)]
    assert "out of bounds for axis 0 with size 64" in msgs[1]
    assert "frame 1" in msgs[0] and "rank 1" in msgs[0]


class _NoPlanes(object):
    keep_planes = False

    def piv_lookup(self, t, prev_plane, prev_table):      # pragma: no cover - never reached
        raise AssertionError


@pytest.mark.parametrize("kw,backend", [
    (dict(estimate_drift=True), "piv"),
    (dict(stitcher="linker"), "piv"),
    (dict(), "oracle"),             # no piv_lookup
    (dict(), "no_planes"),          # keep_planes=False
])
def test_rejected_combinations(kw, backend):
    from _movie_worker import OracleBackend, PivOracleBackend
    from tissue_image_processing_amd import movie
    b = {"piv": PivOracleBackend, "oracle": OracleBackend, "no_planes": _NoPlanes}[backend]()
    calls = []

    def source(t):
        calls.append(t)
        raise AssertionError("no frame may be computed")

    with pytest.raises(ValueError):
        movie.process_movie(3, source, b, 0, 1, None, "cpu", use_piv=True, **kw)
    assert calls == []


def test_use_piv_false_is_unchanged(golden):
    """use_piv=False (the default) is the drift path, exactly as before."""
    from _movie_worker import OracleBackend
    from tissue_image_processing_amd import movie
    g = golden("tracking")
    labs = list(g["labels"])
    drifts = np.zeros((3, 2))
    drifts[1:] = (0.5, -0.3)
    _, ids = movie.process_movie(3, lambda t: labs[t], OracleBackend(), 0, 1, None, "cpu", drifts, use_piv=False)
    for t in range(3):
        np.testing.assert_array_equal(ids[t], g["ids_%d" % t])
