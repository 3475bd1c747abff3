"""GPU: every dispatch regime of the separable Gaussian (csrc/tip_gauss.hip: correlate1d_dev, gaussian3d_dev) at its
boundaries, one launch at a time, bit for bit against the CPU oracle (float64 accumulation in scipy's tap order).

The radius is chosen directly (gpu_util.radius_taps), so a case can sit on either side of a threshold: 11 / 12 / 13 and
119 / 120 / 121 around the long float32 kernel, 12 alone for the float64 slide kernels, 127 (255 taps, the kernel-argument
table's last size) against 128.  Every array sits between NaN bands on the device (gpu_util.GuardedBuffer): a read outside the
input poisons the result, a write outside the output changes a band.  The launch profiler names the kernel that ran
(gpu_util.launches), so a case that silently moved to another regime fails instead of passing on the other kernel.

What a comparison can see differs by dtype.  In float64 the result is the accumulator, and a tap sum in another order differs
from scipy's in most elements: every float64 case with r >= 11 first asserts that on the host (the sum with d running 1 .. r
differs from the oracle in at least a quarter of the elements), so equality there pins the ORDER.  In float32 the final
rounding to 24 bits hides the order of a 53-bit sum almost everywhere: the float32 cases pin taps, indices, clamping and tile
seams, not the order -- the kernels share their accumulation loop shape with the float64 ones, where it is pinned.
"""
import numpy as np
import pytest

from gpu_util import (correlate1d_guarded, launches, order_sensitive_share, radius_taps, taps_patch, wide_range_data)

pytestmark = pytest.mark.gpu

RADII = [1, 11, 12, 13, 64, 119, 120, 121, 127]
F32, F64 = np.float32, np.float64


def expected_kernel(dtype, axis, r):
    """the regime table of correlate1d_dev, as launch names"""
    if dtype == F32:
        if axis != 0 and 12 <= r <= 120:
            return "corr_long_" + "zyx"[axis]
        return "corr_generic_" + "zyx"[axis]
    if r == 12 and axis != 0:
        return ("yslide_r12_f64", "xslide_r12_f64")[axis - 1]
    return "corr_generic_%s_f64" % "zyx"[axis]


def check_against_oracle(orc, vol, taps, axis, kernel=None):
    """One launch through the auto dispatch == the oracle; float64 with r >= 11: the order precondition first.  Returns the
    oracle's array."""
    r = taps.size // 2
    ref = orc.correlate1d(vol, taps, axis)
    if vol.dtype == F64 and r >= 11:
        share = order_sensitive_share(vol, taps, axis, ref)
        assert share >= 0.25, "precondition: only %.0f %% of %s (axis %d, r %d) depend on the tap order" % (
            100 * share, vol.shape, axis, r)
    with launches() as ran:
        out = correlate1d_guarded(vol, taps, axis)
    assert ran == {kernel or expected_kernel(vol.dtype.type, axis, r): 1}, (ran, vol.shape, axis, r)
    np.testing.assert_array_equal(out, ref, err_msg="%s %s axis %d r %d" % (vol.dtype, vol.shape, axis, r))
    return ref


@pytest.fixture()
def orc():
    from oracle import oracle
    return oracle


# ---- every radius, dtype and axis on one ragged volume ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("r", RADII)
def test_every_radius_dtype_axis(orc, r, dtype):
    """(3, 70, 300): lines shorter than most radii along z and y, one tile seam (256) along x; all three axes."""
    rng = np.random.default_rng(1000 + r)
    vol = wide_range_data(rng, (3, 70, 300), dtype)
    taps = radius_taps(r)
    for axis in (0, 1, 2):
        check_against_oracle(orc, vol, taps, axis)


# ---- the long float32 kernel: 256-output tiles of 64 lines, 4 waves x 64 outputs in groups of 8 ----------------------------------
def long_extents(r):
    """(filter-axis length, line-axis length): every filter length once (shorter than a group of 8, shorter than the radius,
    either side of a tile seam) over a ragged line count, every line count once (either side of a 64-line tile) over a ragged
    filter length"""
    filt = [1, 7, r - 1, 255, 256, 257, 300]
    lines = [1, 63, 64, 65, 130]
    return ([(f, (65, 130, 63)[i % 3]) for i, f in enumerate(filt)] +
            [((257, 300)[i % 2], l) for i, l in enumerate(lines)])


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("r", [11, 12, 13, 64, 119, 120, 121])
def test_long_f32_kernel_extents(orc, r, axis):
    """Auto dispatch, the forced generic form (axis + 100) and the forced long form (axis + 200) all equal the oracle, two
    planes each (the plane stride).  r = 11 and r = 121 lie outside [12, 120]: auto is the generic kernel there; the long form
    still runs at r = 11 and refuses r = 121 (its LDS tile is sized for r <= 120) with the argument error.
    float32: pins taps, indices, clamping and seams (module docstring)."""
    from tissue_image_processing_amd import _lib
    taps = radius_taps(r)
    rng = np.random.default_rng(2000 + 10 * r + axis)
    for flen, nlines in long_extents(r):
        shape = (2, flen, nlines) if axis == 1 else (2, nlines, flen)
        vol = wide_range_data(rng, shape, F32)
        ref = check_against_oracle(orc, vol, taps, axis)
        with launches() as ran:
            forced_generic = correlate1d_guarded(vol, taps, axis + 100)
        assert ran == {"corr_generic_" + "zyx"[axis]: 1}
        np.testing.assert_array_equal(forced_generic, ref, err_msg="forced generic %s r %d" % (shape, r))
        if r > 120:
            with pytest.raises(ValueError, match="r<=120"):
                correlate1d_guarded(vol, taps, axis + 200)
            continue
        with launches() as ran:
            forced_long = correlate1d_guarded(vol, taps, axis + 200)
        assert ran == {"corr_long_" + "zyx"[axis]: 1}
        np.testing.assert_array_equal(forced_long, ref, err_msg="forced long %s r %d" % (shape, r))


def test_long_form_refuses_f64_and_axis0(orc):
    taps = radius_taps(12)
    with pytest.raises(ValueError, match="long kernel"):
        correlate1d_guarded(np.zeros((2, 20, 20), F64), taps, 201)
    with pytest.raises(ValueError, match="long kernel"):
        correlate1d_guarded(np.zeros((2, 20, 20), F32), taps, 200)


# ---- the float64 slide kernels (r == 12 only) and the generic float64 kernel next to them -------------------------------------------
def slide_extents(axis):
    """(Y, X): the y pass walks 50-row segments (2 x 25), one thread per column; the x pass makes 8 outputs per thread,
    256 threads per block (2048 outputs: 2047 and 2049 straddle one block)"""
    if axis == 1:
        return [(y, x) for y in (1, 11, 49, 50, 51, 101) for x in (1, 255, 257)]
    return [(y, x) for y in (1, 3) for x in (1, 7, 8, 9, 13, 2047, 2049)]


def slide_planes(y, x):
    """at least two planes, and enough of them that the order precondition is a share of a few hundred elements"""
    return max(2, -(-256 // (y * x)))


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("r", [11, 12, 13])
def test_f64_slide_extents(orc, r, axis):
    """r = 12 runs k_ypass_slide<double, 12, 2> / k_xpass_slide<double, 12>; r = 11 and r = 13 at the same extents run the
    generic float64 kernel.  float64: the order precondition holds for every case, so equality pins the order."""
    taps = radius_taps(r)
    rng = np.random.default_rng(3000 + 10 * r + axis)
    for y, x in slide_extents(axis):
        vol = wide_range_data(rng, (slide_planes(y, x), y, x), F64)
        check_against_oracle(orc, vol, taps, axis)


# ---- axis 0: always the generic kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("r", RADII)
def test_axis0_plane_counts(orc, r, dtype):
    """Z in {1, 2, r - 1, r + 3}: a single plane, fewer planes than the radius, a few more"""
    taps = radius_taps(r)
    rng = np.random.default_rng(4000 + r)
    for Z in sorted({1, 2, r - 1, r + 3} - {0}):
        vol = wide_range_data(rng, (Z, 5, 70), dtype)
        check_against_oracle(orc, vol, taps, 0)


def test_correlate1d_refuses_more_than_65535_rows_or_planes():
    """y and z are grid dimensions: a launch with more of either is refused with a message that names the limit (blur_image
    refolds such arrays on the host, test_blur_image_beyond_65535_lines)"""
    taps = radius_taps(1)
    for shape in [(1, 65536, 1), (65536, 1, 1)]:
        for axis in (0, 1, 2):
            with pytest.raises(ValueError, match="65535"):
                correlate1d_guarded(np.zeros(shape, F32), taps, axis)


# ---- blur_image: the tap table's last size, the device-tap kernel, the ping-pong --------------------------------------------------
@pytest.fixture()
def mods(monkeypatch, golden_taps, oracle_with_golden_taps):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    taps_patch(monkeypatch, golden_taps)
    return bim, oracle_with_golden_taps


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_255_taps_in_the_table_257_in_memory(mods, dtype):
    """sigma 31.8 -> r = 127, 255 taps: the last size the kernel-argument table holds; sigma 31.9 -> r = 128, 257 taps: the
    generic kernel with device taps (corr_big).  Both along y (40 < r) and x (300) of a (40, 300) image."""
    bim, orc = mods
    img = wide_range_data(np.random.default_rng(31), (40, 300), dtype)
    assert bim.gaussian_taps(31.8).size == 255 and bim.gaussian_taps(31.9).size == 257
    with launches() as ran:
        out = bim.blur_image(img, 31.8)
    assert "corr_big" not in ran and sum(ran.values()) == 2, ran
    np.testing.assert_array_equal(out, orc.blur_image(img, 31.8))
    with launches() as ran:
        out = bim.blur_image(img, 31.9)
    assert ran == {"corr_big": 2}, ran
    np.testing.assert_array_equal(out, orc.blur_image(img, 31.9))


SUBSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("subset", SUBSETS, ids=["z", "y", "x", "zy", "zx", "yx", "zyx"])
def test_gaussian3d_ping_pong_axis_subsets(mods, subset, dtype):
    """gaussian3d_dev sends 1 to 3 passes through `out` and one workspace so that the last lands in `out`: all seven axis
    subsets of a (5, 37, 70) volume, sigmas (1, 3, 2) from the table path (r = 4, 12, 8: generic, long / slide, generic).
    The same call twice gives the same bits (the workspace is reused)."""
    bim, orc = mods
    vol = wide_range_data(np.random.default_rng(50 + sum(subset)), (5, 37, 70), dtype)
    sigma = tuple(s * on for s, on in zip((1, 3, 2), subset))
    with launches() as ran:
        out = bim.blur_image(vol, sigma)
    assert sum(ran.values()) == sum(subset), ran
    ref = orc.blur_image(vol, sigma)
    np.testing.assert_array_equal(out, ref)
    np.testing.assert_array_equal(bim.blur_image(vol, sigma), ref)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("sigma", [(1, 40, 2), (0, 3, 40)], ids=["big_in_the_middle", "big_at_the_end"])
def test_gaussian3d_ping_pong_with_device_taps(mods, sigma, dtype):
    """sigma 40 (321 taps) goes through the corr_big launch, whose taps take a workspace slice of their own between the ping-pong's
    passes: in the middle of three passes and at the end of two"""
    bim, orc = mods
    vol = wide_range_data(np.random.default_rng(60), (5, 37, 70), dtype)
    with launches() as ran:
        out = bim.blur_image(vol, sigma)
    assert ran.get("corr_big") == 1 and sum(ran.values()) == sum(s > 0 for s in sigma), ran
    ref = orc.blur_image(vol, sigma)
    np.testing.assert_array_equal(out, ref)
    np.testing.assert_array_equal(bim.blur_image(vol, sigma), ref)


# ---- blur_image beyond 65535 independent lines ---------------------------------------------------------------------------------------
BEYOND = [((65537, 1, 3), (0, 0, 1), F32),          # more planes than a grid takes, x pass
          ((70000, 4), (0, 1.5), F32),              # more rows, x pass
          ((70000, 4), (1.5, 0), F32),              # the FILTERED axis is the long one, and not the last
          ((70000, 4), (1.5, 0), F64),
          ((3, 2, 11000, 5), (0, 0, 0, 1), F32),    # rank 4: 66000 leading lines folded into z
          ((65537, 3, 2), (0, 1, 0), F64),          # y pass under more planes than a grid takes
          ((65537, 3, 2), (1, 1, 1), F32),          # every axis, the first one long
          ((3, 70000, 2), (1, 0, 0), F32)]          # z pass over more rows than a grid takes


@pytest.mark.parametrize("shape,sigma,dtype", BEYOND, ids=["%s-%s-%s" % ("x".join(map(str, s)), "_".join(map(str, g)), np.dtype(d).name)
                                                           for s, g, d in BEYOND])
def test_blur_image_beyond_65535_lines(mods, shape, sigma, dtype):
    """Unfiltered extents are independent lines, and scipy filters any number of them: blur_image refolds the array on the host
    so that no launch sees more than 65535 rows or planes, with the oracle's bits."""
    bim, orc = mods
    img = wide_range_data(np.random.default_rng(70 + len(shape)), shape, dtype)
    out = bim.blur_image(img, sigma)
    assert out.dtype == img.dtype and out.shape == img.shape
    np.testing.assert_array_equal(out, orc.blur_image(img, sigma))


def test_blur_image_beyond_65535_lines_integer_image(mods):
    """an integer table goes the same way (float64 passes truncated after every axis, as scipy's C core stores them)"""
    bim, orc = mods
    img = np.random.default_rng(80).integers(0, 4000, (70000, 4)).astype(np.uint16)
    ref = img.astype(np.float64)
    for sg in [(1.5, 0), (0, 1.5)]:
        ref = np.trunc(orc.blur_image(ref, sg))
    np.testing.assert_array_equal(bim.blur_image(img, 1.5), ref.astype(np.uint16))
