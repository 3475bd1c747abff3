"""CPU: the host side of the U-Net's fp16 range guard -- the policy variable TISSUE_HIP_UNET_RANGE and the refusal of checkpoints
that hold a NaN or an infinity (the device side is tests/test_gpu_unet_range.py)."""
import numpy as np
import pytest

from tissue_image_processing_amd import _lib, _unet_hip, prediction_local as pl


def test_policy_values(monkeypatch):
    monkeypatch.delenv("TISSUE_HIP_UNET_RANGE", raising=False)
    assert _unet_hip.range_policy() == "fallback"
    for v in ("fallback", "raise", "off"):
        monkeypatch.setenv("TISSUE_HIP_UNET_RANGE", v)
        assert _unet_hip.range_policy() == v
    for v in ("", "Fallback", "1", "warn"):
        monkeypatch.setenv("TISSUE_HIP_UNET_RANGE", v)
        with pytest.raises(ValueError, match="TISSUE_HIP_UNET_RANGE"):
            _unet_hip.range_policy()


def test_range_error_is_a_library_error():
    assert issubclass(pl.UNetRangeError, _lib.TissueHipError) and pl.UNetRangeError is _unet_hip.UNetRangeError


def _narrow_weight_list(rng, filters=(4, 8, 16), bottleneck=32):
    """model.get_weights() order of the U-Net of pl.py:31-72 at small widths: 92 arrays, with the name _UNet gives each"""
    ws, names = [], []

    def conv(name, cin, cout, k=3):
        ws.extend([rng.normal(0, 0.1, (k, k, cin, cout)).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)])
        names.extend([name + " kernel", name + " bias"])

    def bn(name, c):
        ws.extend([rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.1, c).astype(np.float32),
                   rng.normal(0, 0.1, c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32)])
        names.extend([name + " statistics"] * 4)

    def double(name, cin, cout):
        conv(name + ".c1", cin, cout)
        bn(name + ".b1", cout)
        conv(name + ".c2", cout, cout)
        bn(name + ".b2", cout)

    c = 2
    for i, f in enumerate(filters):
        double("d%d" % i, c, f)
        c = f
    double("mid", c, bottleneck)
    c = bottleneck
    for i, f in enumerate(reversed(filters)):
        ws.extend([rng.normal(0, 0.1, (3, 3, f, c)).astype(np.float32), rng.normal(0, 0.1, f).astype(np.float32)])
        names.extend(["u%d.t kernel" % i, "u%d.t bias" % i])
        double("u%d" % i, 2 * f, f)
        c = f
    conv("head", c, 2, 1)
    return ws, names


@pytest.mark.parametrize("index,bad", [(0, np.nan), (3, np.inf), (40, -np.inf), (48, np.nan), (49, np.nan), (91, np.nan)])
def test_non_finite_checkpoint_array_is_refused(index, bad):
    """One NaN / infinity anywhere in the 92 arrays: ValueError that names the array (a kernel, a bias, BatchNorm statistics, a
    transposed convolution's arrays, the head's bias).  Such a value used to reach the weight packing, which then scaled the layer
    by 1 without a word."""
    import torch
    ws, names = _narrow_weight_list(np.random.default_rng(5))
    assert len(ws) == 92
    net = pl._UNet(2, "cpu", dtype=torch.float64, weights=ws)         # the clean list loads
    assert net.filters == (4, 8, 16) and net.bottleneck == 32 and net.range_exceeded is False and net.last_mode is None
    ws[index] = ws[index].copy()
    ws[index].reshape(-1)[-1] = bad
    with pytest.raises(ValueError, match=r"%s holds a NaN or an infinity" % names[index].replace(".", r"\.")):
        pl._UNet(2, "cpu", dtype=torch.float64, weights=ws)


def test_reset_range_clears_the_sticky_state():
    import torch
    net = pl._UNet(2, "cpu", dtype=torch.float64, filters=(4, 8, 16), bottleneck=32)
    net.range_exceeded, net._range_warned = True, True
    net.reset_range()
    assert net.range_exceeded is False and net._range_warned is False
    net.range_exceeded, net._range_warned = True, True
    net.randomize_statistics(1)          # new parameters: the old verdict is void
    assert net.range_exceeded is False and net._range_warned is False
