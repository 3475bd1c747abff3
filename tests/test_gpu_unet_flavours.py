"""GPU: every flavour of k_unet_conv (csrc/tip_unet_conv.h; the codes of tip_unet_conv_flavour, include/tissue_hip.h) at the edges
of its own schedule, one launch at a time, against the float64 evaluation of the same stencil on the unsplit values (unet_layers.py).

Grids are 32 x 64 -- 2 x 2 sixteen-row tiles or 4 x 2 eight-row tiles: a seam in y and in x, every border -- and 256 output
channels: two channel blocks, so the weight offset's block term, the per-block constants, the output's channel offset and the
seed's are all exercised.  The (taps, c0, c1) cases put every flavour through its shortest loops (one chunk, fewer steps than the
weight prefetch distance, the switch to the second input at its first chunk) and through loops long enough to wrap every LDS
buffer ring.  Every launch first asserts, through tip_unet_conv_flavour, that the dispatcher picks the flavour the case is listed
under; every output lies between sentinel bands that must come back untouched.

Two kinds of data.  EXACT: inputs multiples of 1/16 in [0, 4), weights signed powers of two in [2^-3, 1] -- every piece split (one
piece holds such a value), every product (a multiple of 2^-7) and every partial sum (|sum| < 2^9: 16 significant bits) is exact in
float32 in any order, in all three modes, so the raw float32 output must EQUAL float64: a wrong tap, chunk, block, permutation or
seam, or a tile read before its copy landed, cannot pass, and no tolerance is involved.  RANDOM: randn inputs, 0.1 randn weights,
held to the per-layer bounds TOL of the existing layer tests on the whole tensor, every border region and every tile seam."""
import pytest

import unet_layers as ul
from unet_layers import HEAD_TOL, MODES, REGIONS, _assert_regions, _join, _split, bits, exact_case, random_case, run_case

pytestmark = pytest.mark.gpu

H, W, COUT = 32, 64, 256

# flavour code -> [(ntaps, c0, c1, tuning under which the dispatcher must pick the flavour)]
_T16, _SPB1 = {"TIP_UNET_TILE8": "0"}, {"TIP_UNET_SPB": "1"}
_CASES = {
    4: [(1, 16, 0, {}), (1, 32, 0, {}), (1, 48, 0, {}), (1, 16, 16, {}), (2, 16, 0, {}), (2, 48, 0, {})],
    1: [(3, 16, 0, {}), (3, 32, 0, {}), (3, 16, 32, {})],
    2: [(4, 16, 0, {}), (5, 16, 0, {}), (6, 32, 0, {}), (8, 16, 16, {}), (4, 144, 0, {}), (9, 16, 0, dict(_T16, **_SPB1)), (9, 144, 16, _SPB1)],
    6: [(9, 16, 0, _T16), (9, 32, 0, _T16), (9, 144, 16, {}), (9, 160, 0, {})],
    0: [(n, c0, c1, {"TIP_UNET_TILE8": "1"}) for n, c0, c1 in
        [(1, 16, 0), (2, 16, 0), (3, 32, 0), (4, 16, 32), (6, 16, 0), (9, 16, 0), (9, 32, 16)]],
}
_CASES[3] = _CASES[0]
_FLAVOUR_MODES = {0: ["f16x3", "bf16x3"], 1: ["f16x3", "bf16x3"], 2: ["f16x3", "bf16x3"], 4: ["f16x3", "bf16x3"], 6: ["f16x3", "bf16x3"],
                  3: ["bf16x6"]}
# one case per template shape for the epilogues (both piece formats of the two-piece shapes)
_SHAPE_CASE = {0: (9, 32, 16, {"TIP_UNET_TILE8": "1"}), 3: (9, 32, 16, {"TIP_UNET_TILE8": "1"}), 1: (3, 16, 32, {}), 2: (6, 32, 0, {}),
               4: (2, 48, 0, {}), 6: (9, 144, 16, {})}


def _params(table):
    out = []
    for code in (4, 1, 2, 6, 0, 3):
        entries = table[code] if isinstance(table[code], list) else [table[code]]
        for ntaps, c0, c1, tune in entries:
            for mode in _FLAVOUR_MODES[code]:
                spb = "-spb1" if tune.get("TIP_UNET_SPB") else ""
                out.append(pytest.param(code, ntaps, c0, c1, tune, mode, id="%s-%dtaps-%d+%d%s-%s" % ("%dx%dx%dx%dx%d" % ul.FLAVOURS[code], ntaps, c0, c1, spb, mode)))
    return out


ALL_CASES = _params(_CASES)
SHAPE_CASES = _params(_SHAPE_CASE)


def _xcd_active(code, h, w, cout):
    """whether a launch of this flavour on this grid uses the XCD workgroup order when TIP_UNET_XCD_MAP allows it (tip_unet.hip)"""
    return cout > 128 and ((h // ul.FLAVOURS[code][1]) * (w // 32)) % 8 == 0


@pytest.mark.parametrize("code,ntaps,c0,c1,tune,mode", ALL_CASES)
def test_exact_data_equal_float64(code, ntaps, c0, c1, tune, mode):
    """EXACT data, every case: the raw float32 output equals the float64 sum, twice into fresh sentinel buffers with identical bits,
    and again with the XCD workgroup order switched off; seeded with multiples of 2^-7 it equals float64's seed + sum, and a zero
    seed changes no bit.

    The stored planes of the BatchNorm epilogue (bias, shift multiples of 1/16, scales 1/2, 1, 2: v = relu(sum + bias) scale + shift
    is a multiple of 2^-8 below 2^11, exact in float32) equal the host's split of the float64 result piece for piece in every mode
    -- both split the same float32 by the same roundings.  Whether the pieces HOLD v: bf16x6, three 8-bit pieces: every float32.
    f16x3: 16 v is a multiple of 2^-4 below 2^15; the high piece's ulp is at most 16, so the remainder is at most 8 = 128 x 2^-4, an
    8-bit multiple of 2^-4 above fp16's subnormal range: held exactly.  bf16x3: the high piece's ulp reaches 8, the remainder 4 =
    1024 x 2^-8 -- up to 11 bits for an 8-bit piece: not held in general, so the joined value is held to TOL instead."""
    import torch
    from tissue_image_processing_amd import _lib
    c = exact_case(ntaps, c0, c1)
    planes, fmt = MODES[mode]
    th = ul.FLAVOURS[code][1]
    zero = torch.zeros((H, W, COUT))
    with _lib.tuning(**tune):
        raw = run_case(mode, code, c, raw=True)["raw"]
        again = run_case(mode, code, c, raw=True)["raw"]
        seeded = run_case(mode, code, c, raw=True, seed=c["seed"])["raw"]
        zero_seeded = run_case(mode, code, c, raw=True, seed=zero)["raw"]
        stored = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])
        with _lib.tuning(TIP_UNET_XCD_MAP="0"):
            raw_plain = run_case(mode, code, c, raw=True)["raw"]
            stored_plain = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])["out"]
    wrong = raw.double() != c["ref"]["sum"]
    print("%s: %d of %d raw sums differ from float64 (XCD order %s)" % (mode, int(wrong.sum()), wrong.numel(), "on" if _xcd_active(code, H, W, COUT) else "not applicable"))
    assert not bool(wrong.any()), "raw output differs from float64 at (y, x, channel) %s ..." % wrong.nonzero()[:4].tolist()
    assert torch.equal(bits(again), bits(raw)), "two identical launches differ"
    assert torch.equal(bits(raw_plain), bits(raw)), "TIP_UNET_XCD_MAP=0 changes the raw output"
    assert torch.equal(seeded.double(), c["seeded"]), "seeded raw output differs from float64's seed + sum"
    assert torch.equal(bits(zero_seeded), bits(raw)), "a zero seed changes the raw output"
    assert stored.get("status", 0) == 0
    want = _split(c["ref"]["out"].float(), planes, fmt)
    assert torch.equal(bits(stored["out"]), bits(want)), "stored pieces differ from the split of the float64 result"
    assert torch.equal(bits(stored_plain), bits(stored["out"])), "TIP_UNET_XCD_MAP=0 changes the stored planes"
    got = _join(stored["out"], fmt).double()
    if mode == "bf16x3":
        _assert_regions(mode, "exact data, stored", got, c["ref"]["out"], REGIONS)
        ul.assert_seams(mode, "exact data, stored", got, c["ref"]["out"], th)
    else:
        assert torch.equal(got, c["ref"]["out"])


@pytest.mark.parametrize("code,ntaps,c0,c1,tune,mode", ALL_CASES)
def test_random_data_within_layer_bounds(code, ntaps, c0, c1, tune, mode):
    """RANDOM data, every case, BatchNorm epilogue: max error / max |reference| below TOL on the whole tensor, every edge, every corner,
    the interior and the rows and columns either side of every tile seam; the XCD workgroup order changes no bit."""
    import torch
    from tissue_image_processing_amd import _lib
    c = random_case(ntaps, c0, c1)
    fmt = MODES[mode][1]
    what = "<%d,%d,%d,%d,%d> %d taps %d+%d" % (ul.FLAVOURS[code] + (ntaps, c0, c1))
    with _lib.tuning(**tune):
        res = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])
        with _lib.tuning(TIP_UNET_XCD_MAP="0"):
            plain = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])["out"]
    assert res.get("status", 0) == 0
    assert torch.equal(bits(plain), bits(res["out"]))
    got = _join(res["out"], fmt).double()
    _assert_regions(mode, what, got, c["ref"]["out"], REGIONS)
    ul.assert_seams(mode, what, got, c["ref"]["out"], ul.FLAVOURS[code][1])


@pytest.mark.parametrize("code,ntaps,c0,c1,tune,mode", [p for p in SHAPE_CASES if p.values[0] not in (0, 3)])
def test_xcd_order_on_sixteen_row_tiles(code, ntaps, c0, c1, tune, mode):
    """32 x 64 is four sixteen-row tiles, and the XCD workgroup order needs a multiple of eight: 32 x 128 (2 x 4 tiles, three seams
    in x) runs it.  EXACT data: raw output equal to float64 and stored planes equal to the split float64 result, bit-identical with
    the order off."""
    import torch
    from tissue_image_processing_amd import _lib
    h, w = 32, 128
    assert _xcd_active(code, h, w, COUT) and not _xcd_active(code, H, W, COUT)
    c = exact_case(ntaps, c0, c1, COUT, h, w)
    planes, fmt = MODES[mode]
    with _lib.tuning(**tune):
        raw = run_case(mode, code, c, raw=True)["raw"]
        stored = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])["out"]
        with _lib.tuning(TIP_UNET_XCD_MAP="0"):
            raw_plain = run_case(mode, code, c, raw=True)["raw"]
            stored_plain = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])["out"]
    assert torch.equal(raw.double(), c["ref"]["sum"])
    assert torch.equal(bits(stored), bits(_split(c["ref"]["out"].float(), planes, fmt)))
    assert torch.equal(bits(raw_plain), bits(raw)) and torch.equal(bits(stored_plain), bits(stored))


@pytest.mark.parametrize("code,ntaps,c0,c1,tune,mode", SHAPE_CASES)
def test_bias_only_epilogue(code, ntaps, c0, c1, tune, mode):
    """no scale / shift (the transposed convolution's layers): sum + bias, no ReLU -- negative values survive"""
    from tissue_image_processing_amd import _lib
    c = random_case(ntaps, c0, c1)
    with _lib.tuning(**tune):
        res = run_case(mode, code, c, bias=c["bias"])
    assert res.get("status", 0) == 0
    got = _join(res["out"], MODES[mode][1]).double()
    assert float(c["ref_bias"].min()) < -0.1 * float(c["ref_bias"].abs().max())
    _assert_regions(mode, "bias-only epilogue", got, c["ref_bias"], REGIONS)
    ul.assert_seams(mode, "bias-only epilogue", got, c["ref_bias"], ul.FLAVOURS[code][1])


@pytest.mark.parametrize("code,ntaps,c0,c1,tune,mode", SHAPE_CASES)
def test_pooled_output(code, ntaps, c0, c1, tune, mode):
    """pool_out: the pooled planes are exactly max_pool2d of the joined stored output (what test_single_layers_against_float64 demands
    of the 8-row flavour), the stored output is the launch's without pool_out bit for bit, and the pooled map is within TOL of
    float64's"""
    import torch
    from tissue_image_processing_amd import _lib
    c = random_case(ntaps, c0, c1)
    fmt = MODES[mode][1]
    with _lib.tuning(**tune):
        res = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"], pool=True)
        alone = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])["out"]
    assert torch.equal(bits(res["out"]), bits(alone))
    assert torch.equal(_join(res["pool"]), torch.nn.functional.max_pool2d(_join(res["out"]).permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0))
    _assert_regions(mode, "pooled output", _join(res["pool"], fmt).double(), c["ref"]["pool"], REGIONS)
    _assert_regions(mode, "output next to the pooled one", _join(res["out"], fmt).double(), c["ref"]["out"], ["all"])


@pytest.mark.parametrize("oy,ox", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("code,ntaps,c0,c1,tune,mode", SHAPE_CASES)
def test_stride_two_mapping(code, ntaps, c0, c1, tune, mode, oy, ox):
    """input-grid pixel (y, x) -> (2 y + oy, 2 x + ox) of a 64 x 128 output, stored (bias only, as the transposed convolution's parity
    classes) and raw: the class is within TOL / equal to float64, the other three parity classes keep the sentinel (run_layer)"""
    import torch
    from tissue_image_processing_amd import _lib
    c, e = random_case(ntaps, c0, c1), exact_case(ntaps, c0, c1)
    with _lib.tuning(**tune):
        res = run_case(mode, code, c, bias=c["bias"], stride=2, oy=oy, ox=ox)
        raw = run_case(mode, code, e, raw=True, stride=2, oy=oy, ox=ox)["raw"]
    got = _join(res["out"][:, oy::2, ox::2], MODES[mode][1]).double()
    _assert_regions(mode, "stride 2, class (%d, %d)" % (oy, ox), got, c["ref_bias"], REGIONS)
    assert torch.equal(raw[oy::2, ox::2].double(), e["ref"]["sum"])


@pytest.mark.parametrize("code,ntaps,c0,c1,tune,mode", SHAPE_CASES)
def test_fused_head(code, ntaps, c0, c1, tune, mode):
    """head_out (128 output channels): class probabilities against float64's softmax at the network tests' bounds, and against
    tip_unet_head_dev on the same layer's stored planes at the same bound"""
    from tissue_image_processing_amd import _lib
    c = random_case(ntaps, c0, c1, 128)
    with _lib.tuning(**tune):
        fused = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"], head=(c["hw"], c["hb"]))
        stored = run_case(mode, code, c, bias=c["bias"], scale=c["scale"], shift=c["shift"])["out"]
    assert fused.get("status", 0) == 0
    ref = c["ref"]["head"]
    assert float((ref * (1 - ref) > 0.05).double().mean()) > 0.9        # (the softmax is not saturated: errors are not hidden)
    separate = ul.head_dev(mode, stored, c["hw"], c["hb"], 0)
    e_f, e_s, e_fs = (float(t.abs().max()) for t in (fused["head"].double() - ref, separate.double() - ref, fused["head"].double() - separate.double()))
    print("%s fused head: max |dp| vs float64 %.2e, tip_unet_head_dev vs float64 %.2e, fused vs separate %.2e" % (mode, e_f, e_s, e_fs))
    assert e_f < HEAD_TOL[mode] and e_s < HEAD_TOL[mode] and e_fs < HEAD_TOL[mode]


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3", "bf16x6"])
def test_head_logits_against_float64(mode):
    """tip_unet_head_dev(logits = 1) on split planes against the float64 dot product of the SAME (joined) values: the kernel rejoins
    the pieces exactly and sums 128 products and the bias in float32 in some order, so per pixel and class
    |error| <= 130 x 2^-24 x (sum |v w| + |b|) (every one of at most 129 additions and 128 products rounds once; first order)."""
    import torch
    planes, fmt = MODES[mode]
    g = torch.Generator().manual_seed(41)
    h, w = 24, 40                                               # 960 pixels: no multiple of the kernel's 32 pixels per block
    v = torch.randn((h, w, 128), generator=g) * 3
    hw, hb = torch.randn((2, 128), generator=g) * 0.05, torch.randn(2, generator=g) * 0.1
    stored = _split(v, planes, fmt)
    joined = _join(stored, fmt).double()
    z = ul.head_dev(mode, stored, hw, hb, 1).double()
    ref = (joined @ hw.double().t() + hb.double()).permute(2, 0, 1)
    bound = 130 * 2.0 ** -24 * ((joined.abs() @ hw.double().abs().t()) + hb.double().abs()).permute(2, 0, 1)
    ratio = float(((z - ref).abs() / bound).max())
    print("%s head logits: max |error| %.2e, largest error / bound %.3f" % (mode, float((z - ref).abs().max()), ratio))
    assert ratio <= 1.0
    p = ul.head_dev(mode, stored, hw, hb, 0).double()
    assert float((p - torch.softmax(ref, 0)).abs().max()) < HEAD_TOL[mode]


def test_refusals_without_a_launch():
    """what the dispatcher refuses, asked through tip_unet_conv_flavour (dummy pointers: nothing is launched or read)"""
    import ctypes
    from tissue_image_processing_amd import _lib
    lib = _lib.lib()
    ARG, UNSUPPORTED = -2, -5
    dy, dx = ul.tap_offsets(9)

    def flavour(mode="f16x3", a0=(32, 64, 32), a1=None, cout=256, taps=9, dy=dy, dx=dx, **kw):
        return lib.tip_unet_conv_flavour(ctypes.byref(ul.describe(mode, a0, a1, taps, dy, dx, cout, **kw)))

    assert flavour() == 0 and flavour("bf16x6") == 3 and flavour(a0=(32, 64, 144)) == 6          # (the descriptor itself is fine)
    assert flavour(a0=(36, 64, 32), out_h=36) == UNSUPPORTED                    # h % 8 != 0
    assert flavour(a0=(32, 48, 32), out_w=48) == UNSUPPORTED                    # w % 32 != 0
    assert flavour(a0=(32, 64, 24)) == UNSUPPORTED                              # c0 % 16 != 0
    assert flavour(a0=(32, 64, 32), a1=(32, 64, 8)) == UNSUPPORTED              # c1 % 16 != 0
    assert flavour(cout=192) == UNSUPPORTED                                     # cout % 128 != 0
    assert flavour(cout=128, head_w=64, head_b=64, head_out=64) == 0            # the head on 128 channels ...
    assert flavour(cout=256, head_w=64, head_b=64, head_out=64) == ARG          # ... and on 256
    assert flavour(pool_out=64) == 0
    assert flavour(pool_out=64, sy=2, sx=2, out_h=64, out_w=128) == ARG         # pool with stride 2
    assert flavour(raw_out=64) == 0
    assert flavour(cout=128, raw_out=64, head_w=64, head_b=64, head_out=64) == ARG      # raw output together with the head
    assert flavour(seed=64) == 0
    assert flavour(seed=64, sy=2, sx=2, out_h=64, out_w=128) == ARG             # seed with stride 2
    assert flavour(sy=2, sx=2, out_h=64, out_w=128) == 0
    assert flavour(taps=1, dy=[2], dx=[0]) == ARG and flavour(taps=1, dy=[0], dx=[-2]) == ARG      # a tap offset of 2
    assert flavour(taps=1, dy=[1], dx=[-1]) == 4
    assert flavour(planes=3) == ARG                                             # fp16 pieces with three planes
    assert flavour(taps=0) == ARG and flavour(taps=10) == ARG
    with _lib.tuning(TIP_UNET_TILE8="0"):
        assert flavour() == 6 and flavour("bf16x6") == 3 and flavour(a0=(24, 64, 32), out_h=24) == 0
        with _lib.tuning(TIP_UNET_SPB="1"):
            assert flavour() == 2
        assert flavour(taps=3, dy=dy[:3], dx=dx[:3]) == 1 and flavour(taps=4, dy=dy[:4], dx=dx[:4]) == 2
    assert _lib.last_error() != ""
