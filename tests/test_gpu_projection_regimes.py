"""GPU: every switch of the projection (csrc/tip_project.hip: project_dev) on both sides, projection and z-map bit for bit
against the CPU oracle's time_point_surface_projection.

The switches: fast = X % 4 == 0 (register-sliding / fused / fp16 kernels) against the generic kernels; the certified fp16 argmax
and the fused mask only up to 64 planes, the exact score + k_argmax_z + the dense mask (a Zs x Zs table, k_xpass_wmax<8>) above;
k_mask_wmax_fused<2 | 4 | 8> by channel count; two mask passes with channel masks when atoh_shift != 0.  The launch profiler
names the kernels that ran (gpu_util.launches), so every case also asserts the tier it was built for.  Every case first asserts
that the oracle's z-map holds at least four distinct planes: the argmax under test is not a constant.
"""
import numpy as np
import pytest

from gpu_util import launches, taps_patch

pytestmark = pytest.mark.gpu

FAST, GENERIC = (40, 48), (33, 50)          # X % 4 == 0, and not
HOOKS = ["TIP_PROJECT_EXACT_SCORE", "TIP_PROJECT_UNFUSED_MASK", "TIP_PROJECT_UNFUSED_PREBLUR"]


@pytest.fixture()
def mods(monkeypatch, golden_taps, oracle_with_golden_taps):
    from tissue_image_processing_amd import surface_projection as sp
    taps_patch(monkeypatch, golden_taps)
    return sp, oracle_with_golden_taps


_STACKS = {}
# The sigma-30 score blur is wider than these small frames, so the chosen plane varies little over most stacks: the seeds are
# the ones (found on the host, with the oracle alone) whose z-maps meet the distinct-planes precondition for every reference
# channel of the case.  nine planes: {(Y, X, C): seed}; 64 / 65 / 70 planes: seed 3.
NINE_PLANE_SEEDS = {(33, 50, 1): 383, (33, 50, 4): 383, (33, 50, 5): 383, (33, 50, 8): 383,
                    (40, 136, 1): 100, (40, 136, 4): 100, (40, 136, 5): 100, (40, 136, 8): 122}


def stack(Z, Y, X, C, offset=0, seed=None):
    """synthetic.make_stack, made once per shape and left unchanged (every call below gets a copy)"""
    from tissue_image_processing_amd import synthetic
    if seed is None:
        seed = NINE_PLANE_SEEDS[(Y, X, C)] if Z == 9 else 3
    key = (Z, Y, X, C, offset, seed)
    if key not in _STACKS:
        st = synthetic.make_stack(Z, Y, X, seed=seed, channels=C, offset=offset)
        st.setflags(write=False)
        _STACKS[key] = st
    return _STACKS[key]


def expected_tier(Zs, X, C, generic_hook=False):
    """launch names that must / must not appear for a bin_size == 1 projection of Zs planes, X columns, C channels"""
    fast = X % 4 == 0 and not generic_hook
    if fast and Zs <= 64:
        return {"preblur_fused", "score_fast_y", "score_fast_x", "argmax_certify", "mask_wmax_fused"}, {"argmax_z", "xpass_wmax"}
    if fast:
        return {"preblur_fused", "argmax_z", "mask_ypass", "xpass_wmax"}, {"score_fast_y", "argmax_certify", "mask_wmax_fused"}
    return {"corr_z_u16clip", "argmax_z", "mask_ypass", "xpass_wmax"}, {"preblur_fused", "score_fast_y", "mask_wmax_fused"}


def check_case(sp, orc, st, ref_ch, **kw):
    """Device projection + z-map == the oracle's (after the distinct-planes precondition), the expected tier ran, and -- fast
    cases of at most 64 planes -- each tuning hook alone gives the same bits.  Where the oracle raises (a shifted plane
    beyond the stack), the device path raises the same exception type."""
    from tissue_image_processing_amd import _lib
    C, Z, Y, X = st.shape
    kw = dict(kw, z_map=True)
    kw.setdefault("airyscan", False)
    try:
        p_ref, z_ref = orc.time_point_surface_projection(st.copy(), "CZYX", ref_ch, **kw)
    except Exception as e:          # the reference's own IndexError for a plane index beyond the stack (sp.py:62, 68-69)
        with pytest.raises(type(e)):
            sp.time_point_surface_projection(st.copy(), "CZYX", ref_ch, **kw)
        return None
    planes = np.unique(z_ref).size
    assert planes >= 4, "precondition: the oracle's z-map holds %d distinct planes" % planes
    Zs = (min(kw["max_z"], Z) - kw.get("min_z", 0)) if kw.get("max_z", 0) > 0 else Z
    with launches() as ran:
        p, z = sp.time_point_surface_projection(st.copy(), "CZYX", ref_ch, **kw)
    need, never = expected_tier(Zs, X, C)
    assert need <= set(ran) and not (never & set(ran)), (sorted(ran), Zs, X, C)
    tag = "C=%d Zs=%d %dx%d ref %d %s" % (C, Zs, Y, X, ref_ch, kw)
    np.testing.assert_array_equal(z, z_ref, err_msg=tag)
    np.testing.assert_array_equal(p, p_ref, err_msg=tag)
    if X % 4 == 0 and Zs <= 64:
        for hook in HOOKS:
            with _lib.tuning(**{hook: "1"}):
                p_h, z_h = sp.time_point_surface_projection(st.copy(), "CZYX", ref_ch, **kw)
            np.testing.assert_array_equal(z_h, z_ref, err_msg=hook + " " + tag)
            np.testing.assert_array_equal(p_h, p_ref, err_msg=hook + " " + tag)
    return p_ref, z_ref


# ---- plane count across the 64 edge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [FAST, GENERIC], ids=["fast", "generic"])
@pytest.mark.parametrize("Zs", [64, 65])
def test_plane_count_across_64(mods, Zs, frame):
    """64 planes: the last stack that takes the certified fp16 argmax and the fused mask (its Zs x Zs table in LDS, its chosen
    planes in bytes); 65: the exact score, k_argmax_z, the dense mask.  Two channels, one mask pass and two (atoh_shift -1)."""
    sp, orc = mods
    st = stack(Zs, frame[0], frame[1], 2)
    for shift in (0, -1):
        assert check_case(sp, orc, st, 0, atoh_shift=shift) is not None


@pytest.mark.parametrize("frame", [FAST, GENERIC], ids=["fast", "generic"])
@pytest.mark.parametrize("min_z,max_z", [(3, 67), (2, 67)], ids=["Zs64", "Zs65"])
def test_plane_range_inside_a_70_plane_stack(mods, min_z, max_z, frame):
    """zlo > 0: planes [3, 67) (64 of them) and [2, 67) (65) of 70; the z-map carries min_z like the reference's"""
    sp, orc = mods
    st = stack(70, frame[0], frame[1], 2)
    assert check_case(sp, orc, st, 0, min_z=min_z, max_z=max_z) is not None


def test_plane_index_beyond_the_slice_raises_like_the_reference(mods):
    """the reference adds min_z to the argmax and then indexes the SLICED stack with it (sp.py:61, 68): on this stack a chosen
    plane + 3 reaches 64, the oracle raises IndexError and so does the device path, at 64 planes and at 65"""
    sp, orc = mods
    st = stack(70, GENERIC[0], GENERIC[1], 2, seed=20)
    for min_z in (3, 2):
        with pytest.raises(IndexError):
            orc.time_point_surface_projection(st.copy(), "CZYX", 0, airyscan=False, z_map=True, min_z=min_z, max_z=67)
        assert check_case(sp, orc, st, 0, min_z=min_z, max_z=67) is None


# ---- channel count -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [(40, 136), GENERIC], ids=["fast", "generic"])
@pytest.mark.parametrize("C", [1, 4, 5, 8])
def test_channel_counts(mods, C, frame):
    """C = 1, 4, 5, 8 (k_mask_wmax_fused<2>, <4> at its last count, <8> at its first and last) at nine planes; (40, 136) spans
    the fused mask's 128-column tile seam and the preblur's 128 x 32 tile.  reference_channel first, last and -1 (numpy's last:
    the reference then compares the channel number with -1, so NO channel takes the unshifted mask), atoh_shift 0, 1, -1 (one
    mask pass, or two with channel masks; with one channel the second pass's mask is empty)."""
    sp, orc = mods
    st = stack(9, frame[0], frame[1], C)
    compared = 0
    for ref_ch in sorted({0, C - 1, -1}):
        for shift in (0, 1, -1):
            compared += check_case(sp, orc, st, ref_ch, atoh_shift=shift) is not None
    assert compared >= 6          # (a shift of +1 may leave the stack, as in the reference; the others cannot)


def test_airyscan_offset_five_channels(mods):
    sp, orc = mods
    st = stack(9, 40, 136, 5, offset=10000)
    assert check_case(sp, orc, st, 0, airyscan=True, atoh_shift=-1) is not None


def test_five_channels_65_planes_dense_mask(mods):
    """the dense mask with more than four channels, (48, 260): in the fast path (Zs > 64) and under TIP_PROJECT_GENERIC"""
    from tissue_image_processing_amd import _lib
    sp, orc = mods
    st = stack(65, 48, 260, 5)
    p_ref, z_ref = check_case(sp, orc, st, 0, atoh_shift=-1)
    with _lib.tuning(TIP_PROJECT_GENERIC="1"):
        with launches() as ran:
            p, z = sp.time_point_surface_projection(st.copy(), "CZYX", 0, airyscan=False, z_map=True, atoh_shift=-1)
    need, never = expected_tier(65, 260, 5, generic_hook=True)
    assert need <= set(ran) and not (never & set(ran)), sorted(ran)
    np.testing.assert_array_equal(z, z_ref)
    np.testing.assert_array_equal(p, p_ref)


def test_nine_channels_raise(mods):
    sp, _ = mods
    with pytest.raises(ValueError, match="1..8 channels"):
        sp.time_point_surface_projection(np.zeros((9, 4, 8, 8), np.uint16), "CZYX", 0, airyscan=False)
