"""GPU: the PIV step of the sharded movie tracker (csrc/tip_piv.hip, movie.process_movie(use_piv=True)).

The sampling-and-lookup kernel against the numpy statement of upstream's steps (tests/_movie_worker.piv_hits), the flow
inside the new entry against tip_optical_flow_tvl1 on the uint16-truncated planes (bit-identical), the driver on the
reference's own use_piv run, on a synthetic square movie against Tissue.track_cells_iterator(use_piv=True), and two
processes on one GPU against one."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gloo_launch import run_ranks  # noqa: E402


@pytest.fixture(scope="module")
def reg():
    from tissue_image_processing_amd import _lib, _registration
    _lib.init(0)
    return _registration


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _rows(rng, Y, X, n):
    """Previous-frame rows that exercise every rule: continuous points, exact .5 ties, negative indices that wrap, points
    that the flow moves out of the frame, and absent rows (area 0, at (0, 0) or elsewhere)."""
    cy = rng.uniform(0, X - 1, n)
    cx = rng.uniform(0, Y - 1, n)
    k = n // 5
    cx[:k] = rng.integers(0, Y - 1, k) + 0.5                      # ties on both axes
    cy[:k] = rng.integers(0, X - 1, k) + 0.5
    cx[k:2 * k] = -rng.integers(1, Y + 1, k) + rng.uniform(-0.49, 0.49, k)   # round(cx) in [-Y, -1]: wraps
    cy[2 * k:3 * k] = -rng.integers(1, X + 1, k) + rng.uniform(-0.49, 0.49, k)
    cx[3 * k:3 * k + 20] = Y - 0.6                                 # near the last row / column: the flow moves some out
    cy[3 * k + 20:3 * k + 40] = X - 0.6
    area = rng.integers(1, 50, n)
    area[rng.random(n) < 0.1] = 0
    absent = np.flatnonzero(area == 0)
    cy[absent[::2]] = 0.0
    cx[absent[::2]] = 0.0
    return dict(area=area, cy=cy, cx=cx)


@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("shape", [(64, 64), (48, 80), (80, 48)])
def test_sample_kernel_matches_numpy(reg, quantized, shape):
    from _movie_worker import piv_hits
    Y, X = shape
    rng = np.random.default_rng(5 + Y)
    flow = rng.uniform(-8, 8, (2, Y, X)).astype(np.float32)
    if quantized:                  # quarter steps: .5 ties also AFTER the shift
        flow = (np.round(flow * 4) / 4).astype(np.float32)
    lab = rng.integers(0, 200, (Y, X)).astype(np.int32)
    tab = _rows(rng, Y, X, 3000)
    tab["cx"] = np.clip(tab["cx"], -Y, Y - 0.6)                   # every index in bounds
    tab["cy"] = np.clip(tab["cy"], -X, X - 0.6)
    want = piv_hits(flow, lab, tab)
    assert (want == -1).sum() > 100 and (want >= 0).sum() > 500
    d_flow, d_lab = _dev(flow), _dev(lab)          # (held: a temporary's memory could be handed to the next tensor)
    got = reg.piv_sample_dev(d_flow.data_ptr(), d_lab.data_ptr(), Y, X, tab)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("bad", [
    [(7, "cy", 64.2), (12, "cx", 70.0)],          # axis 0 is checked over every row before axis 1
    [(7, "cy", 64.2), (30, "cy", -65.0)],         # axis 1 only: the first failing row
    [(3, "cx", -64.6), (9, "cx", 99.0)],          # round(-64.6) = -65
    [(40, "cx", 63.5)],                            # a tie that rounds up to 64
    [(41, "cy", -64.5)],                           # a tie that rounds to -64: wraps, no error
])
def test_sample_kernel_index_errors_as_numpy(reg, bad):
    from _movie_worker import piv_hits
    Y = X = 64
    rng = np.random.default_rng(2)
    flow = rng.uniform(-3, 3, (2, Y, X)).astype(np.float32)
    lab = rng.integers(0, 50, (Y, X)).astype(np.int32)
    tab = _rows(rng, Y, X, 100)
    tab["cx"] = np.clip(tab["cx"], -Y, Y - 0.6)
    tab["cy"] = np.clip(tab["cy"], -X, X - 0.6)
    for i, key, v in bad:
        tab[key][i] = v
    d_flow, d_lab = _dev(flow), _dev(lab)
    try:
        want = piv_hits(flow, lab, tab)
    except IndexError as e:
        with pytest.raises(IndexError) as got:
            reg.piv_sample_dev(d_flow.data_ptr(), d_lab.data_ptr(), Y, X, tab)
        assert str(got.value) == str(e)
    else:
        np.testing.assert_array_equal(reg.piv_sample_dev(d_flow.data_ptr(), d_lab.data_ptr(), Y, X, tab), want)


def test_entry_flow_is_tvl1_on_truncated_planes(reg):
    """The flow inside tip_piv_lookup_max3_i32_dev is tip_optical_flow_tvl1 on the uint16-truncated planes, bit for bit; the
    hits are the numpy statement on that flow; n == 0 computes nothing and returns."""
    import torch
    from _movie_worker import golden_frames, piv_hits
    from oracle import oracle as orc
    (lab0, p0), (lab1, p1) = golden_frames()[:2]
    assert np.any(p0 != np.floor(p0))
    Y, X = p0.shape
    want_flow = reg.optical_flow_tvl1(p0.astype(np.uint16), p1.astype(np.uint16))
    rp = orc.regionprops(lab0)
    tab = dict(area=rp["area"], cy=np.where(rp["area"] > 0, rp["cy"], 0.0), cx=np.where(rp["area"] > 0, rp["cx"], 0.0))
    d0, d1, dl = _dev(p0), _dev(p1), _dev(lab1.astype(np.int32))
    flow = torch.full((2, Y, X), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    hit = reg.piv_lookup_dev(d0.data_ptr(), d1.data_ptr(), dl.data_ptr(), Y, X, tab, flow_ptr=flow.data_ptr())
    np.testing.assert_array_equal(flow.cpu().numpy(), want_flow)
    np.testing.assert_array_equal(hit, piv_hits(want_flow, lab1, tab))
    hit2 = reg.piv_lookup_dev(d0.data_ptr(), d1.data_ptr(), dl.data_ptr(), Y, X, tab)      # flow in the workspace
    np.testing.assert_array_equal(hit2, hit)
    empty = dict(area=np.zeros(0, np.int64), cy=np.zeros(0), cx=np.zeros(0))
    assert reg.piv_lookup_dev(d0.data_ptr(), d1.data_ptr(), dl.data_ptr(), Y, X, empty).shape == (0,)


def test_public_flow_entries_reject_the_internal_dtype(reg):
    from tissue_image_processing_amd import _lib
    import ctypes
    a = np.zeros((8, 8), np.float64)
    f = np.zeros((2, 8, 8), np.float32)
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().tip_optical_flow_tvl1(_lib.ptr(a), _lib.ptr(a), 5, 8, 8, ctypes.c_float(15), ctypes.c_float(0.3),
                                                    5, 10, ctypes.c_double(1e-4), _lib.ptr(f), None, 0))


def test_installed_golden_through_gpu_backend(reg, golden):
    """The driver with the device step on the reference's own use_piv run (label maps and float64 planes installed on the
    device, one process, rounds of one frame)."""
    from _gpu_movie_piv_worker import installed_backend_class
    from _movie_worker import golden_frames
    from tissue_image_processing_amd import movie
    g = golden("piv_tracking")
    frames = golden_frames()
    backend = installed_backend_class()(*frames[0][0].shape)
    try:
        tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], backend, block_frames=1, use_piv=True)
    finally:
        backend.close()
    for t in range(len(frames)):
        np.testing.assert_array_equal(ids[t], g["flow_ids_%d" % t])
        np.testing.assert_array_equal(tabs[t]["drift"], [0.0, 0.0])


def test_synthetic_square_movie_equals_tissue_tracker(reg):
    """Full GpuFrameBackend (projection, segmentation, tables on the device) on a drifting 256^2 movie: the sharded driver's
    ids equal Tissue.track_cells_iterator(use_piv=True) on the backend's own label maps and uint16-truncated planes."""
    from _gpu_movie_piv_worker import synthetic_movie
    from tissue_image_processing_amd import movie
    from tissue_image_processing_amd import tissue_info as ti
    Z, Y, X, T = 6, 256, 256, 4
    stacks = synthetic_movie(Y, X, T, Z)
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, keep_planes=True)
    try:
        tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, use_piv=True)
        labs = [backend.labels[t].download((Y, X), np.int32) for t in range(T)]
        imgs = np.stack([backend.planes[t].cpu().numpy() for t in range(T)]).astype(np.uint16)
    finally:
        backend.close()
    assert all(lab.max() > 20 for lab in labs)
    tis = ti.Tissue(T)
    for f in range(T):
        tis.set_labels(f + 1, labs[f].copy(), reset_data=True)
        tis.calculate_frame_cellinfo(f + 1)
    assert list(tis.track_cells_iterator(1, T, images=imgs, image_in_memory=True, use_piv=True)) == list(range(2, T + 1))
    for f in range(T):
        np.testing.assert_array_equal(ids[f], tis.get_cells_info(f + 1).label.to_numpy())
    for f in range(1, T):                                     # most cells keep their track
        assert np.isin(ids[f], ids[f - 1]).mean() > 0.5


def _run(world, out, mode, timeout=600):
    run_ranks("_gpu_movie_piv_worker.py", world, (out, mode), timeout=timeout, local_rank="0")


def test_world2_equals_world1(tmp_path):
    o1, o2 = str(tmp_path / "w1.npz"), str(tmp_path / "w2.npz")
    _run(1, o1, "square")
    _run(2, o2, "square")
    a, b = np.load(o1), np.load(o2)
    for t in range(int(a["n"])):
        np.testing.assert_array_equal(a["ids_%d" % t], b["ids_%d" % t])
        np.testing.assert_array_equal(a["area_%d" % t], b["area_%d" % t])


def test_world2_non_square_raises_on_both_ranks(tmp_path):
    out = str(tmp_path / "ns.npz")
    _run(2, out, "nonsquare", timeout=300)
    assert not os.path.exists(out)
    msgs = [open("%s.rank%d.err" % (out, r)).read() for r in range(2)]
    assert any("out of bounds for axis 0 with size 128" in m for m in msgs)
    assert all("out of bounds" in m for m in msgs)
