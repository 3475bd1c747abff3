"""CPU: the flag-taking twins of the plan's three entries (tip_unet_conv_ex_dev, tip_unet_conv_flavour_ex, tip_unet_conv_mfma_k_ex;
include/tissue_hip.h) over the sweep of test_unet_plan_host.py.  With flags 0 they are the old entries.  TIP_UNET_CONV_ROWS8_K32
changes ONE answer: the MFMA K of fp16 pieces in two planes on 8-row tiles with four and more taps becomes 32 (unless
TIP_UNET_MFMA=16).  The flavour code never changes, every other launch keeps the unflagged answer, the refusals are the same.
No device is touched."""
import ctypes

import pytest

import test_unet_plan_host as base
import unet_layers as ul
from tissue_image_processing_amd import _lib, _unet_hip

FLAG = _unet_hip.CONV_ROWS8_K32
HEIGHTS = (24, 32)


def expected_ex(mode, ntaps, c0, c1, h, tune, flags):
    """the unflagged rule, and on top of it the flag's one change"""
    code, k = base.expected(mode, ntaps, c0, c1, h, tune)
    planes, fmt = ul.MODES[mode]
    th = ul.FLAVOURS[code][1]
    if flags & FLAG and fmt == 1 and planes == 2 and th == 8 and ntaps >= 4 and int(tune.get("TIP_UNET_MFMA", 32)) == 32:
        k = 32
    return code, k


def _sweep():
    for mode in ul.MODES:
        for ntaps in range(1, 10):
            for c0, c1 in base.CHANNELS:
                for h in HEIGHTS:
                    yield mode, ntaps, c0, c1, h


def test_the_header_names_the_flag():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tissue_hip.h")).read()
    assert int(re.search(r"#define\s+TIP_UNET_CONV_ROWS8_K32\s+(\d+)", text).group(1)) == FLAG


@pytest.mark.parametrize("tune", base.TUNINGS, ids=lambda t: "-".join("%s=%s" % kv for kv in t.items()) or "default")
def test_flags_zero_is_the_old_entries(tune):
    lib = _lib.load()
    wrong = []
    with _lib.tuning(**tune):
        for case in _sweep():
            d = base._desc(*case)
            old = (lib.tip_unet_conv_flavour(ctypes.byref(d)), lib.tip_unet_conv_mfma_k(ctypes.byref(d)))
            new = (lib.tip_unet_conv_flavour_ex(ctypes.byref(d), 0), lib.tip_unet_conv_mfma_k_ex(ctypes.byref(d), 0))
            if old != new or old != base.expected(*case, tune):
                wrong.append((case, old, new))
    assert not wrong, "%d launches (mode, taps, c0, c1, h): old, _ex(0): %s ..." % (len(wrong), wrong[:4])


@pytest.mark.parametrize("tune", base.TUNINGS, ids=lambda t: "-".join("%s=%s" % kv for kv in t.items()) or "default")
def test_the_flag_changes_k_of_the_8_row_fp16_launches_alone(tune):
    lib = _lib.load()
    wrong, changed = [], 0
    with _lib.tuning(**tune):
        for case in _sweep():
            d = base._desc(*case)
            old = (lib.tip_unet_conv_flavour(ctypes.byref(d)), lib.tip_unet_conv_mfma_k(ctypes.byref(d)))
            got = (lib.tip_unet_conv_flavour_ex(ctypes.byref(d), FLAG), lib.tip_unet_conv_mfma_k_ex(ctypes.byref(d), FLAG))
            want = expected_ex(*case, tune, FLAG)
            mode, ntaps = case[0], case[1]
            th = ul.FLAVOURS[old[0]][1]
            converted = mode == "f16x3" and th == 8 and ntaps >= 4 and tune.get("TIP_UNET_MFMA") != "16"
            # the rule, and its pieces spelled out: the code never changes; K changes exactly on the converted launches, to 32
            if got != want or got[0] != old[0] or (got[1] != old[1]) != converted or (converted and got != (0, 32)):
                wrong.append((case, old, got, want))
            changed += converted
    assert not wrong, "%d launches (mode, taps, c0, c1, h): unflagged, flagged, expected: %s ..." % (len(wrong), wrong[:4])
    assert (changed > 0) == (tune.get("TIP_UNET_MFMA") != "16"), "the sweep reaches the converted launches"


def test_what_stays_with_the_flag():
    """named cases: bf16 and three-piece modes, fewer than four taps, 16-row launches (a 16-row f16x3 launch keeps its K = 32
    kernel), TIP_UNET_MFMA=16"""
    lib = _lib.load()

    def ask(mode, ntaps, c0, h, flags=FLAG):
        d = base._desc(mode, ntaps, c0, 0, h)
        return lib.tip_unet_conv_flavour_ex(ctypes.byref(d), flags), lib.tip_unet_conv_mfma_k_ex(ctypes.byref(d), flags)

    assert ask("f16x3", 9, 128, 32) == (0, 32) and ask("f16x3", 9, 128, 32, 0) == (0, 16)      # the network's 128-channel 3x3 layers
    assert ask("f16x3", 4, 16, 24) == (0, 32) and ask("f16x3", 3, 16, 24) == (0, 16)
    assert ask("bf16x3", 9, 128, 32) == (0, 16) and ask("bf16x6", 9, 128, 32) == (3, 16)
    assert ask("f16x3", 9, 144, 32) == (6, 32) and ask("f16x3", 9, 144, 32, 0) == (6, 32)
    assert ask("f16x3", 5, 32, 32) == (2, 32) and ask("f16x3", 3, 32, 32) == (1, 16) and ask("f16x3", 2, 32, 32) == (4, 16)
    with _lib.tuning(TIP_UNET_MFMA="16"):
        assert ask("f16x3", 9, 128, 32) == (0, 16) and ask("f16x3", 9, 144, 32) == (6, 16)
    with _lib.tuning(TIP_UNET_TILE8="1"):
        assert ask("f16x3", 9, 256, 32) == (0, 32) and ask("f16x3", 9, 256, 32, 0) == (0, 16)


def test_refusals_are_the_same():
    """every refusal of test_unet_plan_host.py::test_refusals_by_return_code through the _ex entries, flag off and on; an unknown
    flag bit is an argument error"""
    lib = _lib.load()

    def all_four(*a, **kw):
        d = base._desc(*a, **kw)
        rc = lib.tip_unet_conv_flavour(ctypes.byref(d))
        for flags in (0, FLAG):
            assert lib.tip_unet_conv_flavour_ex(ctypes.byref(d), flags) == rc
            k = lib.tip_unet_conv_mfma_k_ex(ctypes.byref(d), flags)
            assert k == (rc if rc < 0 else expected_ex(*a[:5], {}, flags)[1])
        return rc

    ARG, UNSUPPORTED = base.ARG, base.UNSUPPORTED
    assert all_four("f16x3", 9, 32, 0, 32) == 0 and all_four("bf16x6", 9, 32, 0, 32) == 3 and all_four("f16x3", 9, 144, 0, 32) == 6
    assert all_four("f16x3", 9, 32, 0, 36) == UNSUPPORTED
    assert all_four("f16x3", 9, 32, 0, 32, w=48) == UNSUPPORTED
    assert all_four("f16x3", 9, 24, 0, 32) == UNSUPPORTED
    assert all_four("f16x3", 9, 32, 8, 32) == UNSUPPORTED
    assert all_four("f16x3", 9, 32, 0, 32, cout=192) == UNSUPPORTED
    assert all_four("f16x3", 9, 32, 0, 32, planes=3) == ARG
    assert all_four("f16x3", 9, 32, 0, 32, acc_scale=0.0) == ARG
    assert all_four("f16x3", 9, 32, 0, 32, ntaps=0) == ARG and all_four("f16x3", 9, 32, 0, 32, ntaps=10) == ARG
    assert all_four("f16x3", 9, 32, 0, 32, pool_out=64, sy=2, sx=2, out_h=64, out_w=128) == ARG
    assert all_four("f16x3", 9, 32, 0, 32, seed=64, sy=2, sx=2, out_h=64, out_w=128) == ARG
    assert all_four("f16x3", 9, 32, 0, 32, head_w=64, head_b=64, head_out=64) == ARG
    for flags in (0, FLAG):
        assert lib.tip_unet_conv_flavour_ex(None, flags) == ARG and lib.tip_unet_conv_mfma_k_ex(None, flags) == ARG
    d = base._desc("f16x3", 9, 32, 0, 32)
    assert lib.tip_unet_conv_flavour_ex(ctypes.byref(d), 2) == ARG and lib.tip_unet_conv_mfma_k_ex(ctypes.byref(d), FLAG | 4) == ARG
    assert _lib.last_error() != ""
