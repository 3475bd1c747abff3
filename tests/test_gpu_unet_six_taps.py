"""GPU: the six-tap classes of a composed decoder level on the three-steps-per-barrier schedule (flavour 6 of tip_unet_conv_flavour,
csrc/tip_unet_conv.h: a chunk's six taps in two iterations), which they take from 256 input channels on, and the fragment reads of
k_unet_conv's main loop, which no longer wait for the copies in flight: a tile read before its copy landed shows as a wrong sum.

One launch at a time through unet_layers.run_layer, which asserts the flavour code first and fences every output with sentinels.
Grids as in test_gpu_unet_flavours.py: 32 x 64 (2 x 2 sixteen-row tiles) and 32 x 128 (the XCD workgroup order), 256 output
channels (two channel blocks).  (taps, c0, c1) = (6, 256, 0): the threshold, sixteen chunks -- every LDS ring wraps; (6, 128, 128):
the second input from chunk 8 on, at a chunk boundary inside the loop; (6, 272, 0): seventeen chunks, an odd count (the loop ends
in the activation buffer it began in); (6, 272, 16): a first input of an odd chunk count and a second input of one chunk;
(6, 240, 0), one chunk below the threshold, keeps flavour 2.

EXACT data (unet_layers.exact_case, which asserts its construction: inputs multiples of 1/16 in [0, 4), weights signed powers of two
in [2^-3, 1], every product a multiple of 2^-7 and every sum below 2^9): the raw float32 sum must EQUAL float64 -- no tolerance.
RANDOM data (unet_layers.random_case): the per-layer bounds of the existing layer tests (unet_layers.TOL) on the tensor, its borders
and every tile seam."""
import pytest

import unet_layers as ul
from unet_layers import MODES, _assert_regions, _join, bits, exact_case, random_case, run_case

pytestmark = pytest.mark.gpu

COUT = 256
REGIONS = ["all", "interior", "first row", "last row", "first column", "last column", "top-left corner", "bottom-right corner"]
CASES = [(6, 256, 0, 6), (6, 128, 128, 6), (6, 272, 0, 6), (6, 272, 16, 6), (6, 240, 0, 2)]          # (taps, c0, c1, flavour)
PARAMS = [pytest.param(t, c0, c1, code, mode, id="%dtaps-%d+%d-flavour%d-%s" % (t, c0, c1, code, mode))
          for t, c0, c1, code in CASES for mode in ("f16x3", "bf16x3")]


@pytest.mark.parametrize("h,w", [(32, 64), (32, 128)])
@pytest.mark.parametrize("ntaps,c0,c1,code,mode", PARAMS)
def test_exact_data_equal_float64(ntaps, c0, c1, code, mode, h, w):
    """raw output equal to float64, twice with identical bits, seeded equal to float64's seed + sum, the same bits with the XCD order
    off and with one step per barrier (TIP_UNET_SPB=1: flavour 2, the schedule these launches ran on before)"""
    import torch
    from tissue_image_processing_amd import _lib
    c = exact_case(ntaps, c0, c1, COUT, h, w)
    raw = run_case(mode, code, c, raw=True)["raw"]
    again = run_case(mode, code, c, raw=True)["raw"]
    seeded = run_case(mode, code, c, raw=True, seed=c["seed"])["raw"]
    with _lib.tuning(TIP_UNET_XCD_MAP="0"):
        plain = run_case(mode, code, c, raw=True)["raw"]
    with _lib.tuning(TIP_UNET_SPB="1"):
        one = run_case(mode, 2, c, raw=True)["raw"]
    wrong = raw.double() != c["ref"]["sum"]
    assert not bool(wrong.any()), "raw output differs from float64 at (y, x, channel) %s ..." % wrong.nonzero()[:4].tolist()
    assert torch.equal(bits(again), bits(raw)) and torch.equal(bits(plain), bits(raw)) and torch.equal(bits(one), bits(raw))
    assert torch.equal(seeded.double(), c["seeded"])


@pytest.mark.parametrize("ntaps,c0,c1,code,mode", PARAMS)
def test_random_data_within_layer_bounds(ntaps, c0, c1, code, mode):
    """BatchNorm epilogue on random data: within TOL of float64 on the tensor, its borders and every tile seam, and the stored planes
    are those of the one-step schedule bit for bit (the same products in the same order per accumulator)"""
    import torch
    from tissue_image_processing_amd import _lib
    c = random_case(ntaps, c0, c1, COUT)
    res = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])
    with _lib.tuning(TIP_UNET_SPB="1"):
        one = run_case(mode, 2, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])
    assert res.get("status", 0) == 0
    assert torch.equal(bits(res["out"]), bits(one["out"]))
    got = _join(res["out"], MODES[mode][1]).double()
    what = "flavour %d, %d taps %d+%d" % (code, ntaps, c0, c1)
    _assert_regions(mode, what, got, c["ref"]["out"], REGIONS)
    ul.assert_seams(mode, what, got, c["ref"]["out"], 16)


def test_flavour_of_six_taps():
    """the dispatcher's answer without a launch: six taps take flavour 6 from 256 input channels on, on 16-row tiles, unless
    TIP_UNET_SPB=1; four, five and eight taps and shorter six-tap loops keep flavour 2"""
    import ctypes
    from tissue_image_processing_amd import _lib
    lib = _lib.lib()

    def flavour(taps, c0, c1=0, mode="f16x3", h=32):
        dy, dx = ul.tap_offsets(taps)
        a1 = (h, 64, c1) if c1 else None
        return lib.tip_unet_conv_flavour(ctypes.byref(ul.describe(mode, (h, 64, c0), a1, taps, dy, dx, COUT, out_h=h)))

    assert flavour(6, 256) == 6 and flavour(6, 1024) == 6 and flavour(6, 128, 128) == 6
    assert flavour(6, 240) == 2 and flavour(6, 32) == 2 and flavour(6, 128, 112) == 2
    assert flavour(4, 256) == 2 and flavour(5, 256) == 2 and flavour(8, 256) == 2
    assert flavour(6, 256, h=24) == 0 and flavour(6, 256, mode="bf16x6") == 3
    with _lib.tuning(TIP_UNET_SPB="1"):
        assert flavour(6, 256) == 2
    with _lib.tuning(TIP_UNET_TILE8="1"):
        assert flavour(6, 256) == 0
