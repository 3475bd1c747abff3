"""GPU: a decoder level's transposed convolution folded into the convolution behind it (_unet_hip.compose, the raw-output
and accumulator-seed modes of csrc/tip_unet_conv.h and the border pass of csrc/tip_unet_planes.h) against float64 evaluations of the ORIGINAL, uncomposed layers
on the unsplit values.  Error measure and bounds are those of test_gpu_unet_conv.test_single_layers_against_float64: max error / max
|reference| (of the whole tensor) below 2e-6 / 4e-5 / 2e-6 for f16x3 / bf16x3 / bf16x6 -- asserted on the whole output and again on
every edge region alone, where a missing border term is an error of the values' own size."""
import ctypes

import numpy as np
import pytest

from unet_layers import ACT, MODES, TOL, _assert_regions, _join, _split

pytestmark = pytest.mark.gpu


def _stage(mode, h, w, x, tw, bt, skip, w1, b1, scale, shift):
    """One decoder stage through the composed route: (h, w, 2C) low-resolution input and (2h, 2w, Cs) skip tensor -> the joined
    float64 output (2h, 2w, Cout) of Conv2DTranspose + bias -> concatenate -> Conv2D 3x3 + bias -> ReLU -> scale / shift."""
    import torch
    from tissue_image_processing_amd import _unet_hip as uh, _lib
    planes, fmt = MODES[mode]
    A = ACT if fmt else 1.0
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    st = uh.compose_layers(tw.to(dev), bt.to(dev), w1.to(dev), b1.to(dev), planes, fmt)
    px, ps = _split(x, planes, fmt).to(dev), _split(skip, planes, fmt).to(dev)
    part = uh.composed_up(st, planes, fmt, px, h, w, stream)
    fs, ft = (scale * A).to(dev), (shift * A).to(dev)
    out = torch.empty((planes, 2 * h, 2 * w, w1.shape[0]), dtype=torch.float16 if fmt else torch.bfloat16, device=dev)
    d = uh._conv_desc(st["skip"], planes, fmt, ps, None, 2 * h, 2 * w, st["bias"], fs, ft, out=out, seed=part)
    _lib.check(lib.tip_unet_conv_dev(ctypes.byref(d), stream))
    torch.cuda.synchronize()
    return _join(out.cpu(), fmt).double()


def _stage_reference(x, tw, bt, skip, w1, b1, scale, shift):
    import torch
    F = torch.nn.functional
    h, w = x.shape[:2]
    up = F.conv_transpose2d(x.double().permute(2, 0, 1)[None], tw.double(), bt.double(), stride=2)[:, :, :2 * h, :2 * w]
    cat = torch.cat([up, skip.double().permute(2, 0, 1)[None]], 1)
    ref = F.conv2d(cat, w1.double(), None, padding=1)[0].permute(1, 2, 0)
    return torch.relu(ref + b1.double()) * scale.double() + shift.double()


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3", "bf16x6"])
@pytest.mark.parametrize("low", [(8, 32), (16, 32)])
def test_decoder_stage_against_float64(mode, low):
    """32 low-resolution channels -> 16 (the transposed convolution's output, which never exists) + 16 skip -> 128, asymmetric random
    data; low-resolution grids of 8 rows (8-row tile flavours for the composed stencils) and 16 rows (the 16-row flavours: four-step
    schedule for the 4- and 6-tap classes, three steps per barrier for the 9-tap class)."""
    import torch
    h, w = low
    g = torch.Generator().manual_seed(23 + h)
    x, skip = torch.randn((h, w, 32), generator=g), torch.randn((2 * h, 2 * w, 16), generator=g)
    tw, bt = torch.randn((32, 16, 3, 3), generator=g) * 0.1, torch.randn(16, generator=g)
    w1, b1 = torch.randn((128, 32, 3, 3), generator=g) * 0.1, torch.randn(128, generator=g)
    scale, shift = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    got = _stage(mode, h, w, x, tw, bt, skip, w1, b1, scale, shift)
    ref = _stage_reference(x, tw, bt, skip, w1, b1, scale, shift)
    _assert_regions(mode, "decoder stage %dx%d" % low, got, ref,
                    ["all", "last row", "last column", "bottom-right corner", "first row", "first column"])


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3", "bf16x6"])
def test_transposed_bias_reaches_every_edge_type(mode):
    """All-zero input and skip, non-zero transposed-convolution bias: the output is the bias through the taps that lie inside the
    up-sampled image -- one constant in the interior, another on each of the four edges and four corners."""
    import torch
    h, w = 8, 32
    g = torch.Generator().manual_seed(5)
    x, skip = torch.zeros((h, w, 32)), torch.zeros((2 * h, 2 * w, 16))
    tw, bt = torch.randn((32, 16, 3, 3), generator=g) * 0.1, torch.randn(16, generator=g)
    w1, b1 = torch.randn((128, 32, 3, 3), generator=g) * 0.1, torch.randn(128, generator=g) * 0.1
    scale, shift = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.1
    got = _stage(mode, h, w, x, tw, bt, skip, w1, b1, scale, shift)
    ref = _stage_reference(x, tw, bt, skip, w1, b1, scale, shift)
    assert float((ref[0, 5] - ref[3, 5]).abs().max()) > 0.1 * float(ref.abs().max())      # (the edges do differ from the interior)
    _assert_regions(mode, "bias-only stage", got, ref,
                    ["all", "interior", "first row", "last row", "first column", "last column", "top-left corner", "top-right corner",
                     "bottom-left corner", "bottom-right corner"])


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3", "bf16x6"])
@pytest.mark.parametrize("shape", [(8, 16), (16, 144)])
def test_raw_output_and_seed_round_trip(mode, shape):
    """A 3x3 layer over two concatenated inputs as two launches over the channel halves -- the first with raw float32 output, the second
    seeded with it -- equals the one-launch layer to the bound; a zero seed changes nothing, bit for bit.  8 rows x 16 channels per
    half: the 8-row flavour; 16 rows x 144: the 16-row three-steps-per-barrier flavour (two pieces) takes the seed."""
    import torch
    from tissue_image_processing_amd import _unet_hip as uh, _lib
    planes, fmt = MODES[mode]
    A = ACT if fmt else 1.0
    H, C = shape
    W, CO = 32, 128
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator().manual_seed(31 + C)
    a0, a1 = torch.randn((H, W, C), generator=g), torch.randn((H, W, C), generator=g)
    wt = torch.randn((CO, 2 * C, 3, 3), generator=g) * 0.1
    bias, scale, shift = torch.randn(CO, generator=g), torch.rand(CO, generator=g) + 0.5, torch.randn(CO, generator=g)
    offs = [ky - 1 for ky in range(3) for kx in range(3)], [kx - 1 for ky in range(3) for kx in range(3)]
    taps = lambda sel: torch.stack([wt[:, sel, ky, kx].t() for ky in range(3) for kx in range(3)], 0).to(dev)

    def layer(sel):
        wp, inv = uh._pack(taps(sel), planes, fmt)
        return (wp,) + offs + (inv,)

    whole, first, second = layer(slice(None)), layer(slice(0, C)), layer(slice(C, 2 * C))
    p0, p1 = _split(a0, planes, fmt).to(dev), _split(a1, planes, fmt).to(dev)
    fb, fs, ft = bias.to(dev), (scale * A).to(dev), (shift * A).to(dev)
    store = torch.float16 if fmt else torch.bfloat16

    def run(layer, src, skip, **kw):
        out = None if "raw" in kw else torch.empty((planes, H, W, CO), dtype=store, device=dev)
        d = uh._conv_desc(layer, planes, fmt, src, skip, H, W, None if "raw" in kw else fb, fs, ft, out=out, **kw)
        _lib.check(lib.tip_unet_conv_dev(ctypes.byref(d), stream))
        return out

    one = run(whole, p0, p1)
    part = torch.full((H, W, CO), float("nan"), dtype=torch.float32, device=dev)
    run(first, p0, None, raw=part)
    two = run(second, p1, None, seed=part)
    zero_seeded = run(whole, p0, p1, seed=torch.zeros((H, W, CO), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(zero_seeded.view(torch.int16), one.view(torch.int16))
    x64 = torch.cat([a0, a1], 2).double().permute(2, 0, 1)[None]
    raw_ref = torch.nn.functional.conv2d(x64[:, :C], wt[:, :C].double(), None, padding=1)[0].permute(1, 2, 0)
    ref = torch.nn.functional.conv2d(x64, wt.double(), None, padding=1)[0].permute(1, 2, 0)
    ref = torch.relu(ref + bias.double()) * scale.double() + shift.double()
    top = float(ref.abs().max())
    e_raw = float((part.cpu().double() - raw_ref).abs().max() / raw_ref.abs().max())
    e_two = float((_join(two.cpu(), fmt).double() - _join(one.cpu(), fmt).double()).abs().max()) / top
    e_ref = float((_join(two.cpu(), fmt).double() - ref).abs().max()) / top
    print("%s %dx%d, %d+%d channels: raw output vs float64 %.2e, two launches vs one %.2e, vs float64 %.2e" % (mode, H, W, C, C, e_raw, e_two, e_ref))
    assert e_raw < TOL[mode] and e_two < TOL[mode] and e_ref < TOL[mode]


def test_network_routes_report_and_agree_with_float64(monkeypatch):
    """64 x 256 network, f16x3: the composed route is the default and says so, TISSUE_HIP_UNET_COMPOSE=0 takes the four parity
    launches per level and says so; each within the network tolerance of test_network_hip_path_vs_float64 (4e-6) of the float64
    network."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl
    monkeypatch.setenv("TISSUE_HIP_UNET_ARITH", "f16x3")
    monkeypatch.delenv("TISSUE_HIP_UNET_COMPOSE", raising=False)
    gpu = pl._UNet(2, torch.device("cuda", 0), dtype=torch.float32, seed=3)
    ref = pl._UNet(2, "cpu", dtype=torch.float64, seed=3)
    gpu.randomize_statistics(4)
    ref.randomize_statistics(4)
    x = torch.from_numpy(np.random.default_rng(0).random((1, 2, 64, 256)))
    xg = x.to("cuda").float()
    assert gpu.hip_path_ok(xg)
    exp = ref.forward(x)
    composed = gpu.forward(xg).cpu().double()
    assert gpu.last_mode == "f16x3" and len(gpu.last_compose) > 0
    monkeypatch.setenv("TISSUE_HIP_UNET_COMPOSE", "0")
    plain = gpu.forward(xg).cpu().double()
    assert gpu.last_compose == ()
    monkeypatch.setenv("TISSUE_HIP_UNET_COMPOSE", "u0,u1,u2")
    every = gpu.forward(xg).cpu().double()
    assert gpu.last_compose == ("u0", "u1", "u2")
    e_c, e_p, e_e = (float((t - exp).abs().max()) for t in (composed, plain, every))
    print("f16x3 network 64x256: max |dp| composed (default levels %s) %.2e, uncomposed %.2e, every level composed %.2e"
          % (",".join(gpu.last_compose), e_c, e_p, e_e))
    assert e_c < 4e-6 and e_p < 4e-6 and e_e < 4e-6
