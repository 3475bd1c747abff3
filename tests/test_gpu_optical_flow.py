"""GPU: skimage.registration.optical_flow_tvl1 on the device (tip_optflow.hip) against the scikit-image goldens and the
numpy restatement (tests/tvl1_restate.py), and Tissue.track_cells_iterator(use_piv=True) against the reference's own
tracker (tools/make_goldens_piv.py).  Numerical contract: max <= 2e-3 px, 99.9th percentile
<= 1e-4 px, mean <= 1e-5 px, equal warps per pyramid level."""
import os
import threading

import numpy as np
import pytest

import tvl1_restate as R
from test_optical_flow_host import GOLD, assert_contract, flow_errors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reg():
    from tissue_image_processing_amd import _lib, _registration
    _lib.init(0)
    return _registration


def scene(H, W, seed):
    """Smoothed noise in [0, 1]: texture everywhere, so the flow is determined everywhere."""
    from scipy import ndimage as ndi
    img = ndi.gaussian_filter(np.random.default_rng(seed).random((H, W)), 3.0)
    return (img - img.min()) / (img.max() - img.min())


def moved(img, dy, dx):
    """img sampled at (y - dy, x - dx) with bilinear interpolation (edges clamped): content moves by (dy, dx)."""
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return R.warp_nearest(img.astype(np.float32), np.stack([yy - dy, xx - dx])).astype(np.float64)


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[8:-4] for p in GOLD])
def test_device_flow_matches_golden(reg, path):
    g = np.load(path)
    flow, warps = reg.optical_flow_tvl1_levels(g["ref"], g["mov"], tol=float(g["tol"]))
    assert flow.dtype == np.float32 and flow.shape == g["flow"].shape
    assert warps == list(g["warps"])
    print("%s: max %.3g p99.9 %.3g mean %.3g" % ((os.path.basename(path),) + flow_errors(flow, g["flow"])))
    assert_contract(flow, g["flow"])
    np.testing.assert_array_equal(reg.optical_flow_tvl1(g["ref"], g["mov"], tol=float(g["tol"])), flow)


@pytest.mark.parametrize("shape", [(1023, 777), (33, 33), (17, 500), (1024, 1024)])
def test_device_flow_matches_restatement(reg, shape):
    H, W = shape
    a = scene(H, W, H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    b = moved(a, 0.9 + 0.4 * np.sin(xx / 50.0), -0.6 + 0.3 * np.cos(yy / 40.0))
    a16, b16 = (a * 60000).astype(np.uint16), (b * 60000).astype(np.uint16)
    want, wwarps = R.tvl1(a16, b16)
    flow, warps = reg.optical_flow_tvl1_levels(a16, b16)
    assert warps == wwarps
    print("%s: max %.3g p99.9 %.3g mean %.3g" % ((shape,) + flow_errors(flow, want)))
    assert_contract(flow, want)


def test_2048_shift_recovered(reg):
    a = scene(2048, 2048, 7)
    b = moved(a, 1.25, -0.75)
    flow, warps = reg.optical_flow_tvl1_levels(a, b)
    assert len(warps) == 7 and all(1 <= w <= 5 for w in warps)
    assert np.isfinite(flow).all()
    inner = flow[:, 64:-64, 64:-64]
    assert abs(float(np.median(inner[0])) - 1.25) < 0.01 and abs(float(np.median(inner[1])) + 0.75) < 0.01
    assert abs(float(inner[0].mean()) - 1.25) < 0.01 and abs(float(inner[1].mean()) + 0.75) < 0.01


def test_device_variant_writes_device_flow(reg):
    import torch
    g = np.load(GOLD[0])
    want = reg.optical_flow_tvl1(g["ref"], g["mov"], tol=float(g["tol"]))
    ta = torch.from_numpy(g["ref"].astype(np.float32)).cuda()
    tb = torch.from_numpy(g["mov"].astype(np.float32)).cuda()
    host = reg.optical_flow_tvl1(g["ref"].astype(np.float32), g["mov"].astype(np.float32), tol=float(g["tol"]))
    out = torch.empty((2,) + ta.shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    reg.optical_flow_tvl1_dev(ta.data_ptr(), tb.data_ptr(), ta.shape[0], ta.shape[1], out.data_ptr(), "float32",
                              tol=float(g["tol"]))
    from tissue_image_processing_amd import _lib
    _lib.check(_lib.lib().tip_sync())
    np.testing.assert_array_equal(out.cpu().numpy(), host)
    assert flow_errors(host, want)[0] < 1e-3


def _piv_tissue(g):
    from tissue_image_processing_amd import tissue_info as ti
    labs = g["labels"]
    t = ti.Tissue(labs.shape[0])
    for f in range(labs.shape[0]):
        t.set_labels(f + 1, labs[f].copy(), reset_data=True)
        t.calculate_frame_cellinfo(f + 1)
    return t


def test_piv_tracker_golden(reg):
    g = np.load(os.path.join(ROOT, "tests", "golden", "piv_tracking.npz"))
    t = _piv_tissue(g)
    drifts0 = t.drifts.copy()
    frames = list(t.track_cells_iterator(1, g["labels"].shape[0], images=g["images"], image_in_memory=True, use_piv=True))
    assert frames == [2, 3, 4]
    for f in range(g["labels"].shape[0]):
        np.testing.assert_array_equal(t.get_cells_info(f + 1).label.to_numpy(), g["flow_ids_%d" % f])
    np.testing.assert_array_equal(t.drifts, drifts0)
    np.testing.assert_array_equal(g["flow_drifts"], drifts0)


def test_piv_tracker_analytic_field(reg, monkeypatch):
    """The transposed sampling (row flow at row = round(cx), col = round(cy)) pinned on a fixed field."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "piv_tracking.npz"))

    def analytic(a, b):
        yy, xx = np.mgrid[0:a.shape[0], 0:a.shape[1]].astype(np.float32)
        return np.stack([0.6 + 0.01 * yy - 0.004 * xx, -0.9 + 0.007 * xx]).astype(np.float32)

    monkeypatch.setattr(reg, "optical_flow_tvl1", analytic)
    t = _piv_tissue(g)
    list(t.track_cells_iterator(1, g["labels"].shape[0], images=g["images"], image_in_memory=True, use_piv=True))
    for f in range(g["labels"].shape[0]):
        np.testing.assert_array_equal(t.get_cells_info(f + 1).label.to_numpy(), g["analytic_ids_%d" % f])


def test_piv_tracker_non_square_index_error(reg):
    """Upstream indexes the flow [round(cx), round(cy)]: on a frame wider than tall, a cell right of the last row index
    raises IndexError, as numpy does in the reference."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "piv_tracking.npz"))
    from tissue_image_processing_amd import tissue_info as ti
    labs, imgs = g["labels"][:2, :64, :], g["images"][:2, :64, :]          # 64 rows x 128 columns
    t = ti.Tissue(2)
    for f in range(2):
        t.set_labels(f + 1, labs[f].copy(), reset_data=True)
        t.calculate_frame_cellinfo(f + 1)
    assert t.get_cells_info(1).cx.max() > 64
    with pytest.raises(IndexError):
        list(t.track_cells_iterator(1, 2, images=imgs, image_in_memory=True, use_piv=True))


def test_piv_without_images_is_the_drift_path(reg):
    g = np.load(os.path.join(ROOT, "tests", "golden", "tracking.npz"))
    out = []
    for piv in (False, True):
        from tissue_image_processing_amd import tissue_info as ti
        labs = g["labels"]
        t = ti.Tissue(labs.shape[0])
        for f in range(labs.shape[0]):
            t.set_labels(f + 1, labs[f].copy(), reset_data=True)
            t.calculate_frame_cellinfo(f + 1)
        t.drifts[1] = (0.5, -0.3)
        t.drifts[2] = (0.5, -0.3)
        assert list(t.track_cells_iterator(1, labs.shape[0], use_piv=piv)) == [2, 3]
        out.append(([t.get_cells_info(f + 1).label.to_numpy() for f in range(labs.shape[0])], t.drifts.copy()))
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(out[0][1], out[1][1])
    for f in range(g["labels"].shape[0]):
        np.testing.assert_array_equal(out[1][0][f], g["ids_%d" % f])


def test_two_threads_give_serial_results(reg):
    from tissue_image_processing_amd import _lib
    pairs = []
    for k, path in enumerate(GOLD[:4]):
        g = np.load(path)
        pairs.append((g["ref"], g["mov"], float(g["tol"])))
    serial = [reg.optical_flow_tvl1_levels(a, b, tol=t) for a, b, t in pairs]
    got = [None] * len(pairs)
    errs = []

    def work(idx):
        try:
            _lib.init(0)
            for _ in range(2):
                for i in idx:
                    a, b, t = pairs[i]
                    got[i] = reg.optical_flow_tvl1_levels(a, b, tol=t)
            _lib.load().tip_shutdown()
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(ix,)) for ix in ([0, 2], [1, 3])]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for (f0, w0), (f1, w1) in zip(serial, got):
        assert w0 == w1
        np.testing.assert_array_equal(f0, f1)
