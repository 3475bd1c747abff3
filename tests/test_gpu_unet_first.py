"""GPU: the U-Net's first layer on the matrix cores (csrc/tip_unet_first.h: k_unet_conv_first_mfma, mode f16x3) -- an implicit im2col
with K = 18 padded to 32 -- against the float32 vector kernel it replaces there (bit for bit on data both compute exactly), against
float64, its range flag, and the hook TIP_UNET_FIRST that selects between the two."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACT = 16.0                                                        # _unet_hip._F16_ACT_SCALE
F16_MAX = 65504.0


def _ctx():
    import torch
    from tissue_image_processing_amd import _lib
    dev = torch.device("cuda", 0)
    return dev, _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _status(lib, stream):
    from tissue_image_processing_amd import _lib
    flags = ctypes.c_int(-1)
    _lib.check(lib.tip_unet_range_read(stream, ctypes.byref(flags)))
    return flags.value


def _run(kernel, x, w, bias, scale, shift):
    """x (2, H, W), w (128, 2, 3, 3) as the network holds them, bias / scale / shift (128) in the layer's own units, all float32 on
    the host -> (the two fp16 planes (2, H, W, 128) on the host, status word).  kernel "mfma": tip_unet_conv_first_packed_dev with
    the weights packed as _unet_hip.weights() packs them; "valu": tip_unet_conv_first_dev, format 1."""
    import torch
    from tissue_image_processing_amd import _lib, _unet_hip
    dev, lib, stream = _ctx()
    H, W = x.shape[1:]
    xd = x.float().contiguous().to(dev)
    rows18 = w.float().permute(2, 3, 1, 0).reshape(18, 128).contiguous().to(dev)       # k = 2 (3 ky + kx) + channel
    fb, fs, ft = bias.float().to(dev), (scale.float() * ACT).to(dev), (shift.float() * ACT).to(dev)
    out = torch.zeros((2, H, W, 128), dtype=torch.float16, device=dev)
    _lib.check(lib.tip_unet_range_reset(stream))
    if kernel == "mfma":
        rows = torch.zeros((1, 32, 128), dtype=torch.float32, device=dev)
        rows[0, :18] = rows18
        wp, inv = _unet_hip._pack(rows, 2, 1)
        _lib.check(lib.tip_unet_conv_first_packed_dev(xd.data_ptr(), H, W, wp.data_ptr(), inv, fb.data_ptr(), fs.data_ptr(), ft.data_ptr(),
                                                      out.data_ptr(), stream))
    else:
        _lib.check(lib.tip_unet_conv_first_dev(xd.data_ptr(), H, W, rows18.data_ptr(), fb.data_ptr(), fs.data_ptr(), ft.data_ptr(),
                                               out.data_ptr(), 2, 1, stream))
    st = _status(lib, stream)
    return out.cpu(), st


@pytest.mark.parametrize("shape", [(24, 96), (8, 32)])
def test_exact_case_equals_the_vector_kernel_bit_for_bit(shape):
    """Inputs multiples of 1/16 in [0, 4), weights signed powers of two in [2^-3, 1], biases and shifts multiples of 1/16, BatchNorm
    scales powers of two: every piece split is exact (lo = 0), every product and every 18-term sum is exact in float32 in both
    kernels, so the two planes are equal bit for bit -- a wrong tap, channel, permutation or seam cannot pass.  24 x 96 is 3 x 3
    segments' worth of seams with all four borders; at 8 x 32 one segment row touches every border."""
    import torch
    H, W = shape
    g = torch.Generator().manual_seed(17 + H)
    x = torch.randint(0, 64, (2, H, W), generator=g).float() / 16
    w = 2.0 ** -torch.randint(0, 4, (128, 2, 3, 3), generator=g).float() * (torch.randint(0, 2, (128, 2, 3, 3), generator=g).float() * 2 - 1)
    bias = torch.randint(-64, 64, (128,), generator=g).float() / 16
    scale = 2.0 ** torch.randint(-1, 2, (128,), generator=g).float()
    shift = torch.randint(-64, 64, (128,), generator=g).float() / 16
    new, st_new = _run("mfma", x, w, bias, scale, shift)
    old, st_old = _run("valu", x, w, bias, scale, shift)
    assert st_new == 0 and st_old == 0
    ref = torch.nn.functional.conv2d(x.double()[None], w.double(), None, padding=1)[0].permute(1, 2, 0)
    ref = torch.relu(ref + bias.double()) * scale.double() + shift.double()
    assert torch.equal(old.float().sum(0).double() / ACT, ref)            # (the construction: the vector kernel is exact on it)
    diff = new.view(torch.int16) != old.view(torch.int16)
    print("%dx%d: %d of %d piece words differ" % (H, W, int(diff.sum()), diff.numel()))
    assert not bool(diff.any())


@pytest.mark.parametrize("shape", [(8, 32), (40, 96)])
def test_accuracy_against_float64(shape):
    """randn inputs, 0.1 randn weights, random bias / scale / shift as in test_gpu_unet_conv.py::test_single_layers_against_float64,
    against torch float64 on the unsplit values; bound: that test's f16x3 bound for a single layer, 2e-6 of the largest value."""
    import torch
    H, W = shape
    g = torch.Generator().manual_seed(11 + H)
    x = torch.randn((2, H, W), generator=g)
    w = torch.randn((128, 2, 3, 3), generator=g) * 0.1
    bias, scale, shift = torch.randn(128, generator=g), torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    out, st = _run("mfma", x, w, bias, scale, shift)
    got = out.float().sum(0).double() / ACT
    ref = torch.nn.functional.conv2d(x.double()[None], w.double(), None, padding=1)[0].permute(1, 2, 0)
    ref = torch.relu(ref + bias.double()) * scale.double() + shift.double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print("first layer on the matrix cores, %dx%d: max error / max |value| = %.2e" % (H, W, err))
    assert st == 0
    assert err < 2e-6


# Frames beyond one segment per wave.  The launch is min(h w / 128, 512) workgroups of four waves and a wave walks the 32-pixel
# segments wave, wave + 2048, ...: up to 65536 pixels (every size above) the loop body runs once and the prefetch of the next
# segment never.  264 x 256 is 2112 segments -- waves 0 .. 63 take two, the rest one (an uneven tail; a first iteration that does
# and one that does not prefetch); 136 x 1024 is 4352 -- two or three (the prefetch guard goes false on a LATER iteration, for some
# waves an iteration earlier than for others); 256 x 512 is 4096 -- exactly two.  TIP_UNET_FIRST=3 cuts the launch to 768 workgroups:
# 264 x 256 is then one segment per wave from 528 workgroups, the largest single-segment launch.
WALKS = [((264, 256), None), ((136, 1024), None), ((256, 512), None), ((264, 256), "3")]


@pytest.mark.parametrize("shape,first", WALKS)
def test_segment_walk(shape, first):
    """The construction of test_exact_case_equals_the_vector_kernel_bit_for_bit (bit for bit against the vector kernel, which equals
    float64) and the data and bound of test_accuracy_against_float64 (2e-6), on frames whose waves walk several segments; the
    status word stays 0."""
    import contextlib
    import torch
    from tissue_image_processing_amd import _lib
    H, W = shape
    hook = _lib.tuning(TIP_UNET_FIRST=first) if first else contextlib.nullcontext()
    g = torch.Generator().manual_seed(29 + H)
    x = torch.randint(0, 64, (2, H, W), generator=g).float() / 16
    w = 2.0 ** -torch.randint(0, 4, (128, 2, 3, 3), generator=g).float() * (torch.randint(0, 2, (128, 2, 3, 3), generator=g).float() * 2 - 1)
    bias = torch.randint(-64, 64, (128,), generator=g).float() / 16
    scale = 2.0 ** torch.randint(-1, 2, (128,), generator=g).float()
    shift = torch.randint(-64, 64, (128,), generator=g).float() / 16
    with hook:
        new, st_new = _run("mfma", x, w, bias, scale, shift)
    old, st_old = _run("valu", x, w, bias, scale, shift)
    assert st_new == 0 and st_old == 0
    ref = torch.nn.functional.conv2d(x.double()[None], w.double(), None, padding=1)[0].permute(1, 2, 0)
    ref = torch.relu(ref + bias.double()) * scale.double() + shift.double()
    assert torch.equal(old.float().sum(0).double() / ACT, ref)
    diff = (new.view(torch.int16) != old.view(torch.int16)).any(0).any(-1)          # (H, W): pixels with a differing piece word
    print("%dx%d: %d of %d pixels differ from the vector kernel; first: %s" % (H, W, int(diff.sum()), diff.numel(), diff.nonzero()[:4].tolist()))
    assert not bool(diff.any())
    assert torch.equal(new.float().sum(0).double() / ACT, ref)
    del new, old, diff

    x = torch.randn((2, H, W), generator=g)
    w = torch.randn((128, 2, 3, 3), generator=g) * 0.1
    bias, scale, shift = torch.randn(128, generator=g), torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    with hook:
        out, st = _run("mfma", x, w, bias, scale, shift)
    got = out.float().sum(0).double() / ACT
    ref = torch.nn.functional.conv2d(x.double()[None], w.double(), None, padding=1)[0].permute(1, 2, 0)
    ref = torch.relu(ref + bias.double()) * scale.double() + shift.double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print("first layer on the matrix cores, %dx%d%s: max error / max |value| = %.2e" % (H, W, ", TIP_UNET_FIRST=3" if first else "", err))
    assert st == 0
    assert err < 2e-6


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x6"])
def test_vector_kernel_bf16_pieces_against_float64(mode):
    """tip_unet_conv_first_dev with bf16 pieces (the first layer of modes bf16x3 and bf16x6, otherwise reached by whole-network runs
    only) at 24 x 96 against float64, at the per-layer bounds of the layer tests (unet_layers.TOL)."""
    import torch
    from tissue_image_processing_amd import _lib
    from unet_layers import MODES, TOL, Fenced
    planes, fmt = MODES[mode]
    dev, lib, stream = _ctx()
    H, W = 24, 96
    g = torch.Generator().manual_seed(53)
    x = torch.randn((2, H, W), generator=g)
    w = torch.randn((128, 2, 3, 3), generator=g) * 0.1
    bias, scale, shift = torch.randn(128, generator=g), torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    xd = x.contiguous().to(dev)
    rows18 = w.permute(2, 3, 1, 0).reshape(18, 128).contiguous().to(dev)
    fb, fs, ft = bias.to(dev), scale.to(dev), shift.to(dev)
    out = Fenced((planes, H, W, 128), torch.bfloat16, dev)
    _lib.check(lib.tip_unet_conv_first_dev(xd.data_ptr(), H, W, rows18.data_ptr(), fb.data_ptr(), fs.data_ptr(), ft.data_ptr(),
                                           out.t.data_ptr(), planes, fmt, stream))
    torch.cuda.synchronize()
    out.check("%s first layer" % mode)
    got = out.t.cpu().float().sum(0).double()
    ref = torch.nn.functional.conv2d(x.double()[None], w.double(), None, padding=1)[0].permute(1, 2, 0)
    ref = torch.relu(ref + bias.double()) * scale.double() + shift.double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print("%s first layer (vector kernel), %dx%d: max error / max |value| = %.2e" % (mode, H, W, err))
    assert err < TOL[mode]


def _one_channel(x_value, scale_value, pixel=None, channel=5):
    """8 x 32 pixels, input channel 0 = 1 everywhere (x_value at `pixel`), centre weight 2^-12 (input test) or 1 into `channel`, bias
    and shift 0, BatchNorm scale x activation scale = scale_value -> (status, hi and lo planes of the channel)"""
    import torch
    H, W = 8, 32
    x = torch.zeros((2, H, W))
    x[0] = 1.0
    w = torch.zeros((128, 2, 3, 3))
    w[channel, 0, 1, 1] = 1.0 if pixel is None else 2.0 ** -12
    if pixel is not None:
        x[0, pixel[0], pixel[1]] = x_value
    zero = torch.zeros(128)
    scale = torch.full((128,), float(scale_value) / ACT)
    out, st = _run("mfma", x, w, zero, scale, zero)
    o = out.float()
    assert float(o[..., [c for c in range(128) if c != channel]].abs().max()) == 0.0
    return st, o[0, :, :, channel], o[1, :, :, channel]


def test_range_flag_input():
    """an input pixel of 5000 (16 x 5000 is beyond fp16) raises TIP_UNET_RANGE_F16 instead of being silently saturated; 4094 -- stored
    as exactly 65504 -- does not"""
    st, hi, lo = _one_channel(5000.0, ACT, pixel=(3, 7))
    assert st == 1
    assert float(hi[3, 7]) + float(lo[3, 7]) == F16_MAX * 2.0 ** -12             # (the clamped input through the centre tap, stored times 16)
    st, hi, lo = _one_channel(4094.0, ACT, pixel=(3, 7))
    assert st == 0
    assert float(hi[3, 7]) + float(lo[3, 7]) == F16_MAX * 2.0 ** -12
    st, hi, lo = _one_channel(-4094.0, ACT, pixel=(0, 0))
    assert st == 0
    st, hi, lo = _one_channel(-5000.0, ACT, pixel=(7, 31))
    assert st == 1


def test_range_flag_output():
    """one channel pushed beyond the range by a large BatchNorm scale raises the flag and is stored as +-65504 (|v| = 65504 / 16);
    exactly 65504 is in range (the construction of test_gpu_unet_range.py::test_exact_limit_first_layer)"""
    over = np.nextafter(np.float32(F16_MAX), np.float32(np.inf))
    st, hi, lo = _one_channel(None, F16_MAX)
    assert st == 0
    assert float(hi.min()) == float(hi.max()) == F16_MAX and float(lo.abs().max()) == 0.0
    st, hi, lo = _one_channel(None, over)
    assert st == 1
    assert float(hi.min()) == float(hi.max()) == F16_MAX and float(lo.abs().max()) == 0.0
    st, hi, lo = _one_channel(None, -over)
    assert st == 1
    assert float(hi.min()) == float(hi.max()) == -F16_MAX and float(lo.abs().max()) == 0.0
    st, hi, lo = _one_channel(None, -F16_MAX)
    assert st == 0
    assert float(hi.min()) == float(hi.max()) == -F16_MAX
    st, hi, lo = _one_channel(None, F16_MAX)          # reset clears the word
    assert st == 0


def test_hook_selects_the_vector_kernel(monkeypatch):
    """The network at 64 x 256 in f16x3 with TIP_UNET_FIRST=valu and without it: probabilities within 5e-6 absolute, the spread
    DESIGN 5.7 records between float32-equivalent routes."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl, _lib
    for v in ("TISSUE_HIP_UNET_RANGE", "TISSUE_HIP_UNET_ARITH", "TISSUE_HIP_UNET_COMPOSE"):
        monkeypatch.delenv(v, raising=False)
    net = pl._UNet(2, torch.device("cuda", 0), dtype=torch.float32, seed=3)
    net.randomize_statistics(1)
    x = torch.from_numpy(np.random.default_rng(0).random((1, 2, 64, 256))).to("cuda").float()
    assert net.hip_path_ok(x)
    lib = _lib.lib()
    _lib.set_tuning("TIP_UNET_FIRST", None)
    assert lib.tip_unet_first_mfma() == 1
    p_new = net.forward(x)
    assert net.last_mode == "f16x3"
    with _lib.tuning(TIP_UNET_FIRST="valu"):
        assert lib.tip_unet_first_mfma() == 0
        p_old = net.forward(x)
        assert net.last_mode == "f16x3"
    assert lib.tip_unet_first_mfma() == 1
    d = float((p_new - p_old).abs().max())
    print("TIP_UNET_FIRST mfma vs valu, 64x256 network: max |dp| = %.2e" % d)
    assert d < 5e-6
