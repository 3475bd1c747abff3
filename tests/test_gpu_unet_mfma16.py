"""GPU: the K = 32 kernel behind the f16x3 convolutions on 16-row tiles with four and more taps (csrc/tip_unet_conv_k32.h:
v_mfma_f32_16x16x32_f16 on PAIRS of consecutive (chunk, tap) steps), one launch at a time against the float64 evaluation of the same
stencil (unet_layers.py).  The flavour code -- which the MFMA shape does not change -- and tip_unet_conv_mfma_k are asserted in front
of every launch.

The (taps, c0, c1) cases walk the pairing's edges: one chunk with an unpaired last step (9, 16, 0); one pair straddling a chunk
boundary (9, 32, 0); straddle and unpaired last step (9, 48, 0); the straddling pair reading in0 and in1 (9, 16, 16); longer loops that
wrap the three-pair weight ring and both activation buffers (9, 32, 16), (9, 144, 0), (6, 256, 0), (6, 272, 16); every tap count from
four to eight, of which four taps make the next chunk's activations due one pair after they are issued.  Grids 32 x 64 (2 x 2 tiles:
a seam in y and in x) and 32 x 128 (the XCD workgroup order, on and off), 256 output channels (two channel blocks).

The 8-row kernel (flavour 0) stays on 32x32x16, so the cases at h = 24 and under the default plan only assert that
tip_unet_conv_mfma_k says so.  EXACT and RANDOM data are unet_layers' exact_case and random_case: what test_gpu_unet_flavours.py
runs on, drawn once per process."""
import ctypes

import pytest

import unet_layers as ul
from unet_layers import HEAD_TOL, REGIONS, TOL, _assert_regions, _join, _split, bits, exact_case, random_case, run_case

pytestmark = pytest.mark.gpu

MODE, COUT = "f16x3", 256
T16 = {"TIP_UNET_TILE8": "0"}          # (nine taps on <= 128 input channels take 8-row tiles by default)
CASES = [(9, 16, 0), (9, 32, 0), (9, 48, 0), (9, 16, 16), (9, 32, 16), (9, 144, 0),
         (4, 16, 0), (5, 32, 0), (6, 256, 0), (6, 272, 16), (7, 48, 0), (8, 32, 0)]
GRIDS = [(32, 64), (32, 128)]
EPILOGUE_CASE = (9, 48, 0)             # straddling pairs and an unpaired last step


def _code(ntaps, c0, c1, spb=3):
    return 6 if spb > 1 and (ntaps == 9 or (ntaps == 6 and c0 + c1 >= 256)) else 2


def _mfma_k(ntaps, c0, c1, h, w, cout=COUT):
    from tissue_image_processing_amd import _lib
    dy, dx = ul.tap_offsets(ntaps)
    return _lib.lib().tip_unet_conv_mfma_k(ctypes.byref(ul.describe(MODE, (h, w, c0), (h, w, c1) if c1 else None, ntaps, dy, dx, cout, out_h=h, out_w=w)))


def _run(c, ntaps, c0, c1, h, w, want_k=32, spb=3, **kw):
    """one launch; the flavour code (run_layer) and the MFMA shape are asserted first"""
    assert _mfma_k(ntaps, c0, c1, h, w, c["taps"].shape[2]) == want_k
    return run_case(MODE, _code(ntaps, c0, c1, spb), c, **kw)


@pytest.mark.parametrize("h,w", GRIDS)
@pytest.mark.parametrize("ntaps,c0,c1", CASES)
def test_exact_data_equal_float64(ntaps, c0, c1, h, w):
    """EXACT data: raw output equal to float64, seeded output equal to seed + sum, identical bits twice in a row, with
    TIP_UNET_SPB=1 (another flavour code, the same kernel) and with the XCD order off; stored pieces equal to the split of the
    float64 result"""
    import torch
    from tissue_image_processing_amd import _lib
    c = exact_case(ntaps, c0, c1, COUT, h, w)
    bn = dict(bias=c["bias"], scale=c["scale"], shift=c["shift"])
    with _lib.tuning(**T16):
        raw = _run(c, ntaps, c0, c1, h, w, raw=True)["raw"]
        again = _run(c, ntaps, c0, c1, h, w, raw=True)["raw"]
        seeded = _run(c, ntaps, c0, c1, h, w, raw=True, seed=c["seed"])["raw"]
        stored = _run(c, ntaps, c0, c1, h, w, **bn)
        with _lib.tuning(TIP_UNET_SPB="1"):
            raw_spb1 = _run(c, ntaps, c0, c1, h, w, spb=1, raw=True)["raw"]
            stored_spb1 = _run(c, ntaps, c0, c1, h, w, spb=1, **bn)["out"]
        with _lib.tuning(TIP_UNET_XCD_MAP="0"):
            raw_plain = _run(c, ntaps, c0, c1, h, w, raw=True)["raw"]
            stored_plain = _run(c, ntaps, c0, c1, h, w, **bn)["out"]
    wrong = raw.double() != c["ref"]["sum"]
    print("%d of %d raw sums differ from float64" % (int(wrong.sum()), wrong.numel()))
    assert not bool(wrong.any()), "raw output differs from float64 at (y, x, channel) %s ..." % wrong.nonzero()[:4].tolist()
    assert torch.equal(seeded.double(), c["seeded"]), "seeded raw output differs from float64's seed + sum"
    assert torch.equal(bits(again), bits(raw)), "two identical launches differ"
    assert torch.equal(bits(raw_spb1), bits(raw)), "TIP_UNET_SPB=1 changes the raw output"
    assert torch.equal(bits(raw_plain), bits(raw)), "TIP_UNET_XCD_MAP=0 changes the raw output"
    assert stored["status"] == 0
    want = _split(c["ref"]["out"].float(), 2, 1)
    assert torch.equal(bits(stored["out"]), bits(want)), "stored pieces differ from the split of the float64 result"
    assert torch.equal(bits(stored_spb1), bits(stored["out"])) and torch.equal(bits(stored_plain), bits(stored["out"]))


@pytest.mark.parametrize("h,w", GRIDS)
@pytest.mark.parametrize("ntaps,c0,c1", CASES)
def test_random_data_within_layer_bounds(ntaps, c0, c1, h, w):
    """RANDOM data: unet_layers' per-layer bound for f16x3 on the tensor, every border region and every tile seam; the 32x32x16
    kernels (TIP_UNET_MFMA=16) and the K = 32 kernel, each within that bound of float64, differ by at most twice the bound"""
    from tissue_image_processing_amd import _lib
    c = random_case(ntaps, c0, c1, COUT, h, w)
    bn = dict(bias=c["bias"], scale=c["scale"], shift=c["shift"])
    with _lib.tuning(**T16):
        res = _run(c, ntaps, c0, c1, h, w, **bn)
        with _lib.tuning(TIP_UNET_MFMA="16"):
            old = _run(c, ntaps, c0, c1, h, w, want_k=16, **bn)
    assert res["status"] == 0 and old["status"] == 0
    got, was = _join(res["out"], 1).double(), _join(old["out"], 1).double()
    what = "K = 32, %d taps %d+%d, %dx%d" % (ntaps, c0, c1, h, w)
    _assert_regions(MODE, what, got, c["ref"]["out"], REGIONS)
    ul.assert_seams(MODE, what, got, c["ref"]["out"], 16)
    diff = float((got - was).abs().max()) / float(c["ref"]["out"].abs().max())
    print("%s: max |K = 32 - K = 16| / max |value| = %.2e" % (what, diff))
    assert diff <= 2 * TOL[MODE]


def test_eight_row_launches_keep_32x32x16():
    """flavour 0 is not converted: h = 24 (no multiple of 16), and the default plan's nine taps on <= 128 input channels"""
    from tissue_image_processing_amd import _lib
    assert _mfma_k(9, 32, 0, 24, 64) == 16
    assert _mfma_k(9, 128, 0, 32, 64) == 16
    with _lib.tuning(**T16):
        assert _mfma_k(9, 128, 0, 32, 64) == 32
        assert _mfma_k(3, 32, 0, 32, 64) == 16 and _mfma_k(2, 32, 0, 32, 64) == 16        # flavours 1 and 4
        with _lib.tuning(TIP_UNET_MFMA="16"):
            assert _mfma_k(9, 128, 0, 32, 64) == 16


# ---- the epilogue's forms on the K = 32 kernel's lane map, one case each ------------------------------------------------------------

def test_bias_only_epilogue():
    from tissue_image_processing_amd import _lib
    c = random_case(*EPILOGUE_CASE)
    with _lib.tuning(**T16):
        res = _run(c, *EPILOGUE_CASE, 32, 64, bias=c["bias"])
    assert res["status"] == 0
    got = _join(res["out"], 1).double()
    assert float(c["ref_bias"].min()) < -0.1 * float(c["ref_bias"].abs().max())
    _assert_regions(MODE, "bias-only epilogue", got, c["ref_bias"], REGIONS)
    ul.assert_seams(MODE, "bias-only epilogue", got, c["ref_bias"], 16)


def test_pooled_output():
    """the pooled planes are exactly max_pool2d of the joined stored output, which is the launch's without pool_out bit for bit"""
    import torch
    from tissue_image_processing_amd import _lib
    c = random_case(*EPILOGUE_CASE)
    bn = dict(bias=c["bias"], scale=c["scale"], shift=c["shift"])
    with _lib.tuning(**T16):
        res = _run(c, *EPILOGUE_CASE, 32, 64, pool=True, **bn)
        alone = _run(c, *EPILOGUE_CASE, 32, 64, **bn)["out"]
    assert torch.equal(bits(res["out"]), bits(alone))
    assert torch.equal(_join(res["pool"]), torch.nn.functional.max_pool2d(_join(res["out"]).permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0))
    _assert_regions(MODE, "pooled output", _join(res["pool"], 1).double(), c["ref"]["pool"], REGIONS)
    _assert_regions(MODE, "output next to the pooled one", _join(res["out"], 1).double(), c["ref"]["out"], ["all"])


@pytest.mark.parametrize("oy,ox", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_stride_two_mapping(oy, ox):
    """stored (bias only) and raw output through the stride-2 mapping: the class within the bound / equal to float64, the other three
    parity classes keep the sentinel (run_layer)"""
    import torch
    from tissue_image_processing_amd import _lib
    c, e = random_case(*EPILOGUE_CASE), exact_case(*EPILOGUE_CASE)
    with _lib.tuning(**T16):
        res = _run(c, *EPILOGUE_CASE, 32, 64, bias=c["bias"], stride=2, oy=oy, ox=ox)
        raw = _run(e, *EPILOGUE_CASE, 32, 64, raw=True, stride=2, oy=oy, ox=ox)["raw"]
    got = _join(res["out"][:, oy::2, ox::2], 1).double()
    _assert_regions(MODE, "stride 2, class (%d, %d)" % (oy, ox), got, c["ref_bias"], REGIONS)
    assert torch.equal(raw[oy::2, ox::2].double(), e["ref"]["sum"])


def test_fused_head():
    """head_out (128 output channels) against float64's softmax and against tip_unet_head_dev on the same layer's stored planes"""
    from tissue_image_processing_amd import _lib
    c = random_case(*EPILOGUE_CASE, 128)
    bn = dict(bias=c["bias"], scale=c["scale"], shift=c["shift"])
    with _lib.tuning(**T16):
        fused = _run(c, *EPILOGUE_CASE, 32, 64, head=(c["hw"], c["hb"]), **bn)
        stored = _run(c, *EPILOGUE_CASE, 32, 64, **bn)["out"]
    assert fused["status"] == 0
    ref = c["ref"]["head"]
    assert float((ref * (1 - ref) > 0.05).double().mean()) > 0.9
    separate = ul.head_dev(MODE, stored, c["hw"], c["hb"], 0)
    e_f, e_fs = float((fused["head"].double() - ref).abs().max()), float((fused["head"].double() - separate.double()).abs().max())
    print("fused head: max |dp| vs float64 %.2e, fused vs separate %.2e" % (e_f, e_fs))
    assert e_f < HEAD_TOL[MODE] and e_fs < HEAD_TOL[MODE]


def test_range_flag_fires():
    """the fp16 range word (test_gpu_unet_range.py's mechanism): BatchNorm scales that push values past 4094 set bit 0 and the stored
    pieces saturate; the same layer with its own scales does not"""
    from tissue_image_processing_amd import _lib
    c = random_case(*EPILOGUE_CASE)
    big = c["scale"] * (2.0 * 4094 / float(c["ref"]["out"].abs().max()))
    assert float((ul.reference(c["a0"], c["a1"], c["taps"], c["dy"], c["dx"], c["bias"], big, c["shift"])["out"]).abs().max()) > 4094 * 1.5
    with _lib.tuning(**T16):
        ok = _run(c, *EPILOGUE_CASE, 32, 64, bias=c["bias"], scale=c["scale"], shift=c["shift"])
        over = _run(c, *EPILOGUE_CASE, 32, 64, bias=c["bias"], scale=big, shift=c["shift"])
    assert ok["status"] == 0
    assert over["status"] & 1
    assert float(_join(over["out"], 1).abs().max()) <= 65504 / 16
