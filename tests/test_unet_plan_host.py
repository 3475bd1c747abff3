"""CPU: the rule by which tip_unet_conv_dev picks what it launches (csrc/tip_unet.hip: unet_conv_plan and the launch table), asked
through tip_unet_conv_flavour and tip_unet_conv_mfma_k -- neither touches a device, and loading the library needs none.  The rule is
restated here from its description (include/tissue_hip.h) and swept over modes, tap counts, channel counts on both
sides of every threshold, both tile heights and the tunings that enter it; the GPU tests assert the same two answers in front of
their launches, for the cases they run."""
import ctypes

import pytest

import unet_layers as ul
from tissue_image_processing_amd import _lib

ARG, UNSUPPORTED = -2, -5
CODE_OF = {shape: code for code, shape in ul.FLAVOURS.items()}
CHANNELS = [(16, 0), (128, 0), (112, 16), (240, 0), (256, 0), (128, 128)]
TUNINGS = [{}, {"TIP_UNET_TILE8": "0"}, {"TIP_UNET_TILE8": "1"}, {"TIP_UNET_SPB": "1"}, {"TIP_UNET_MFMA": "16"}]


def expected(mode, ntaps, c0, c1, h, tune):
    """(flavour code, MFMA K) of a launch: tile rows, weight steps ahead, activation chunks ahead, steps per barrier, then K"""
    planes, fmt = ul.MODES[mode]
    tile8, spb_max, mfma = (int(tune.get(k, v)) for k, v in (("TIP_UNET_TILE8", -1), ("TIP_UNET_SPB", 3), ("TIP_UNET_MFMA", 32)))
    want8 = tile8 == 1 or (tile8 < 0 and ntaps == 9 and c0 + c1 <= 128)
    th = 16 if planes == 2 and h % 16 == 0 and not want8 else 8
    d = 4 if th == 16 and ntaps >= 4 else 2
    da = 2 if th == 16 and ntaps <= 2 else 1
    three = ntaps == 9 or (ntaps == 6 and c0 + c1 >= 256)
    spb = 3 if th == 16 and d == 4 and three and spb_max > 1 else 1
    return CODE_OF[(planes, th, d, da, spb)], 32 if fmt == 1 and th == 16 and d == 4 and mfma == 32 else 16


def _desc(mode, taps, c0, c1, h, w=64, cout=256, **kw):
    """keywords: descriptor fields to override"""
    dy, dx = ul.tap_offsets(taps)
    return ul.describe(mode, (h, w, c0), (h, w, c1) if c1 else None, taps, dy, dx, cout, **kw)


@pytest.mark.parametrize("tune", TUNINGS, ids=lambda t: "-".join("%s=%s" % kv for kv in t.items()) or "default")
def test_code_and_mfma_k_follow_the_rule(tune):
    lib = _lib.load()
    wrong = []
    with _lib.tuning(**tune):
        for mode in ul.MODES:
            for ntaps in range(1, 10):
                for c0, c1 in CHANNELS:
                    for h in (24, 32):
                        d = _desc(mode, ntaps, c0, c1, h)
                        got = (lib.tip_unet_conv_flavour(ctypes.byref(d)), lib.tip_unet_conv_mfma_k(ctypes.byref(d)))
                        if got != expected(mode, ntaps, c0, c1, h, tune):
                            wrong.append(((mode, ntaps, c0, c1, h), got, expected(mode, ntaps, c0, c1, h, tune)))
    assert not wrong, "%d launches (mode, taps, c0, c1, h): (code, K) got, expected: %s ..." % (len(wrong), wrong[:4])


def test_the_tunings_reach_every_code_and_both_shapes():
    """the sweep is not vacuous: over its cases the rule yields all six codes, and K = 32 under codes 2 and 6 alone"""
    seen = {expected(mode, n, c0, c1, h, t) for t in TUNINGS for mode in ul.MODES for n in range(1, 10) for c0, c1 in CHANNELS for h in (24, 32)}
    assert {code for code, _ in seen} == set(ul.FLAVOURS)
    assert {code for code, k in seen if k == 32} == {2, 6}


def test_refusals_by_return_code():
    """both entries return the launch's error (test_gpu_unet_flavours.py::test_refusals_without_a_launch has the full list)"""
    lib = _lib.load()

    def both(*a, **kw):
        d = _desc(*a, **kw)
        rc = lib.tip_unet_conv_flavour(ctypes.byref(d))
        assert lib.tip_unet_conv_mfma_k(ctypes.byref(d)) == (rc if rc < 0 else expected(*a[:5], {})[1])
        return rc

    assert both("f16x3", 9, 32, 0, 32) == 0 and both("bf16x6", 9, 32, 0, 32) == 3 and both("f16x3", 9, 144, 0, 32) == 6
    assert both("f16x3", 9, 32, 0, 36) == UNSUPPORTED                       # h % 8 != 0
    assert both("f16x3", 9, 32, 0, 32, w=48) == UNSUPPORTED                 # w % 32 != 0
    assert both("f16x3", 9, 24, 0, 32) == UNSUPPORTED                       # c0 % 16 != 0
    assert both("f16x3", 9, 32, 8, 32) == UNSUPPORTED                       # c1 % 16 != 0
    assert both("f16x3", 9, 32, 0, 32, cout=192) == UNSUPPORTED             # cout % 128 != 0
    assert both("f16x3", 9, 32, 0, 32, planes=3) == ARG                     # fp16 pieces with three planes
    assert both("f16x3", 9, 32, 0, 32, acc_scale=0.0) == ARG                # fp16 pieces without their scale
    assert both("f16x3", 9, 32, 0, 32, ntaps=0) == ARG and both("f16x3", 9, 32, 0, 32, ntaps=10) == ARG
    assert both("f16x3", 9, 32, 0, 32, pool_out=64, sy=2, sx=2, out_h=64, out_w=128) == ARG      # pool with stride 2
    assert both("f16x3", 9, 32, 0, 32, seed=64, sy=2, sx=2, out_h=64, out_w=128) == ARG          # seed with stride 2
    assert both("f16x3", 9, 32, 0, 32, head_w=64, head_b=64, head_out=64) == ARG                 # the head on 256 channels
    assert lib.tip_unet_conv_flavour(None) == ARG and lib.tip_unet_conv_mfma_k(None) == ARG
    assert _lib.last_error() != ""
