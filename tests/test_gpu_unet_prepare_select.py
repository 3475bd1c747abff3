"""GPU: the order statistics of prepare_image's fused pass (tip_unet_prepare_f64_dev: a radix select in five digit passes by a fixed
number of workgroups; the workgroup that finishes last picks the digit and re-arms the state) against the torch expressions the
pass replaces (sort + where + divide), bit for bit, and against normalize_channel on the host.

The inputs are the smallest on which each part of the select decides: keys that differ only in the last digits or only in the
first, ranks inside a run of equal keys and inside the run of the maximum, planes shorter than one workgroup's stripe and around
its edge, the largest channel count, planes that give every workgroup several trips and a ragged last one, and calls of different
shapes back to back on one context (counters and histograms must come back armed)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ulp_ladder(rng):
    return 1000.0 + np.spacing(1000.0) * rng.integers(0, 8192, (2, 61, 67))       # the keys differ in their lowest 13 bits only


def _zero_run(rng):
    img = rng.random((2, 97, 131)) * 3000
    img[rng.random(img.shape) < 0.6] = 0.0                                        # the 1st percentile lies inside the run of zeros
    return img


def _saturated(rng):
    img = rng.random((2, 64, 200)) * 4000 - 50
    u = rng.random(img.shape)
    img[u < 0.05] = 4095.0                                                        # the 99th percentile lies inside the run of the maximum
    img[(u >= 0.05) & (u < 0.10)] = -0.0
    return img


def _signed_pow2(rng):
    sign = np.where(rng.random((1, 50, 41)) < 0.5, -1.0, 1.0)
    return sign * np.ldexp(1.0, rng.integers(-300, 300, (1, 50, 41)))             # only the leading digits differ


def _length(n):
    def make(rng):
        return rng.random((1, 1, n)) * 100.0 - 20.0
    return make


CASES = {
    "ulp_ladder": _ulp_ladder,
    "zero_run": _zero_run,
    "saturated_top_signed_zero": _saturated,
    "signed_powers_of_two": _signed_pow2,
    "c8": lambda rng: rng.random((8, 33, 65)) * 500.0,
    "several_trips": lambda rng: rng.random((2, 1000, 1031)) * 4000.0 - 100.0,
    "several_trips_c4": lambda rng: rng.random((4, 1024, 1031)) * 4000.0 - 100.0,  # fewer workgroups per channel: two unrolled trips
    "uint16": lambda rng: rng.integers(0, 4000, (2, 200, 333)).astype(np.uint16),
}
for _n in (2, 3, 100, 101, 2047, 2048, 2049):
    CASES["n%d" % _n] = _length(_n)


def _make(case):
    return CASES[case](np.random.default_rng(7))


@pytest.fixture(scope="module")
def pred():
    """one predictor for the module: prepare_image takes every shape, and its select state lives with the calling thread"""
    from tissue_image_processing_amd import prediction_local as pl
    return pl.SegmentationPredictor(None, (2, 64, 64))


def _fused(pred, img, monkeypatch):
    monkeypatch.delenv("TISSUE_HIP_PREPARE_TORCH", raising=False)
    out, npad = pred.prepare_image(img)
    return out.clone(), npad


def _torch_path(pred, img, monkeypatch):
    monkeypatch.setenv("TISSUE_HIP_PREPARE_TORCH", "1")
    out, npad = pred.prepare_image(img)
    monkeypatch.delenv("TISSUE_HIP_PREPARE_TORCH", raising=False)
    return out, npad


def _check(pred, img, monkeypatch):
    """fused == torch path (bit for bit) and close to normalize_channel; returns the fused result"""
    import torch
    from tissue_image_processing_amd import prediction_local as pl
    fused, npad = _fused(pred, img, monkeypatch)
    ref, npad_ref = _torch_path(pred, img, monkeypatch)
    torch.cuda.synchronize()
    assert npad == npad_ref and fused.shape == ref.shape and fused.dtype == ref.dtype
    assert torch.equal(fused, ref)
    host = img.cpu().numpy() if isinstance(img, torch.Tensor) else img
    exp = np.stack([pl.normalize_channel(host[c]) for c in range(host.shape[0])])
    assert np.isfinite(exp).all()
    got = fused[0, :, npad[1][0]:, npad[2][0]:].cpu().numpy()
    np.testing.assert_allclose(got, np.transpose(exp, (0, 2, 1)), rtol=1e-6, atol=1e-7)
    return fused


@pytest.mark.parametrize("case", sorted(CASES))
def test_select_equals_sort(case, pred, monkeypatch):
    _check(pred, _make(case), monkeypatch)


def test_select_on_a_transposed_view(pred, monkeypatch):
    """the plane orientation whose second index has unit stride"""
    import torch
    base = torch.as_tensor(np.random.default_rng(7).random((2, 260, 517)) * 900.0, device="cuda")
    img = base.transpose(1, 2)
    _check(pred, img, monkeypatch)


def test_select_on_a_plane_off_the_16_byte_grid(pred, monkeypatch):
    """channel planes that start 8 bytes past a 16-byte boundary and have an odd length: the 16-byte loads start one key in"""
    import torch
    flat = torch.as_tensor(np.random.default_rng(7).random(1 + 2 * 45 * 71) * 50.0 - 3.0, device="cuda")
    img = flat[1:].view(2, 45, 71)
    assert img.data_ptr() % 16 == 8
    _check(pred, img, monkeypatch)


def test_state_is_rearmed_between_calls(pred, monkeypatch):
    """one predictor, one thread, one select state: ulp ladder, zero run, ulp ladder again -- the first and the third result are
    equal, and each equals the sort's"""
    import torch
    a, b = _make("ulp_ladder"), _make("zero_run")
    first = _check(pred, a, monkeypatch)
    _check(pred, b, monkeypatch)
    third = _check(pred, a, monkeypatch)
    assert torch.equal(first, third)


def test_eight_channels_then_one(pred, monkeypatch):
    import torch
    a, b = _make("c8"), _make("signed_powers_of_two")
    first = _check(pred, a, monkeypatch)
    _check(pred, b, monkeypatch)
    assert torch.equal(first, _check(pred, a, monkeypatch))
