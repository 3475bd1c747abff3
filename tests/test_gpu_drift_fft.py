"""GPU: the float64 FFT behind the drift estimate (csrc/tip_fft.hip) by itself, through tip_fft2_c128, against the high-precision
direct DFT of tests/dft_restate.py; and the phase correlation at its edges (8192-point Bluestein rows, shifts on the wrap
midpoint, every parity of the upsampled region, every dtype branch, the argmax tie rule, the C-ABI's error returns) against the
oracle and, for whole-pixel circular rolls, against the analytic shift."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import dft_restate as dr
from oracle_guard import guarded_oracle

pytestmark = pytest.mark.gpu

U = dr.U
LENGTHS = [2, 3, 4, 5, 16, 17, 97, 255, 256, 1024, 2048, 2049, 3001, 4095, 4096]
RAGGED = [(5, 7), (17, 33), (16, 48), (97, 64), (3, 2049)]
MARGIN = 16                       # library error <= MARGIN * numpy.fft's error on the same input and bins


def pow2(n):
    return n & (n - 1) == 0


def probe_shape(N, axis):
    """a 1-D length as a 2-D array of a handful of rows: 2 rows for a power of two (the whole transform stays radix-2 and
    the derived bound applies), 3 rows otherwise"""
    other = 2 if pow2(N) else 3
    return (other, N) if axis == "x" else (N, other)


ALL_SHAPES = [probe_shape(N, ax) for N in LENGTHS for ax in "xy"] + RAGGED
ALL_SHAPES = sorted(set(ALL_SHAPES), key=ALL_SHAPES.index)


def bins_of(N):
    """every bin up to 1024; beyond, 0, 1, N/2, N-1 and 64 seeded others"""
    if N <= 1024:
        return np.arange(N)
    extra = np.random.default_rng(N).choice(N, 64, replace=False)
    return np.array(sorted({0, 1, N // 2, N - 1} | set(int(v) for v in extra)))


def all_bins(shape):
    return max(shape) <= 1024


@functools.lru_cache(maxsize=None)
def case(shape, inverse, real=False):
    """(input, bins_y, bins_x, reference at the bins, numpy.fft at the bins, ||x||_2), computed once per case"""
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    z = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if real:
        z = z.real + 0j
    by, bx = bins_of(shape[0]), bins_of(shape[1])
    ref = dr.dft2(z, by, bx, inverse=inverse)
    npy = (np.fft.ifft2(z, norm="forward") if inverse else np.fft.fft2(z))[np.ix_(by, bx)]
    for a in (z, by, bx, npy):
        a.setflags(write=False)
    return z, by, bx, ref, npy, dr.norm2(z)


def higham(shape):
    """Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2, for a radix-2 transform of t = log2(Ny Nx) stages:
    ||yhat - y||_2 / ||y||_2 <= t eta / (1 - t eta), eta = mu + gamma_4 (sqrt 2 + mu) < 8u with twiddles good to mu = 2u."""
    t = int(np.log2(shape[0])) + int(np.log2(shape[1]))
    mu = 2 * U
    g4 = 4 * U / (1 - 4 * U)
    eta = mu + g4 * (np.sqrt(2.0) + mu)
    assert eta < 8 * U
    return t, t * eta / (1 - t * eta)


def fft2(z, inverse=False):
    from tissue_image_processing_amd import _lib
    return _lib.fft2_c128(z, inverse)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fft2_against_high_precision_dft(shape, inverse):
    """Two criteria on complex standard-normal input.

    Derived (both extents powers of two): Higham's Thm 24.2 bound in the 2-norm where every bin is compared, elsewhere its
    per-bin consequence |yhat_k - y_k| <= 8u t sqrt(N) ||x||_2 (N = Ny Nx points, t = log2 N).  ASSUMPTION: the sincospi
    twiddles are good to mu <= 2u (relative, as complex numbers); the bound is not proved for a worse table.

    Measured (every shape, Bluestein's three-transform rows included): the worst error over the compared bins is at most 16
    times numpy.fft's worst error on the same input and bins, both relative to ||x||_2."""
    z, by, bx, ref, npy, xn = case(shape, inverse)
    got = fft2(z, inverse)
    assert got.shape == z.shape and got.dtype == np.complex128
    err = dr.abs_diff(got[np.ix_(by, bx)], ref)
    e_lib, e_np = err.max() / xn, dr.abs_diff(npy, ref).max() / xn
    print("fft2 %dx%d %s: library %.2fu numpy %.2fu ratio %.2f"
          % (shape[0], shape[1], "inverse" if inverse else "forward", e_lib / U, e_np / U, e_lib / e_np))
    if pow2(shape[0]) and pow2(shape[1]):
        t, bound = higham(shape)
        n = shape[0] * shape[1]
        if all_bins(shape):
            yn = np.sqrt(n) * xn                                   # Parseval: ||y||_2 = sqrt(N) ||x||_2
            assert np.sqrt(np.sum(err ** 2)) <= bound * yn
        assert err.max() <= 8 * U * t * np.sqrt(n) * xn
    assert e_lib <= MARGIN * e_np


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fft2_forward_then_inverse(shape):
    """inverse(forward(z)) = Ny Nx z within twice the forward bound: the inverse transforms the forward pass's error (its
    2-norm grows by exactly sqrt N) and adds as much of its own.  Powers of two: 2 B + B^2 in the 2-norm, B from Thm 24.2.
    Other shapes: per bin the forward error is at most 16 e_np ||z||_2, so an element of the result is off by at most
    N * 16 e_np ||z||_2 from those and sqrt N * 16 e_np ||z||_2 from the inverse pass: together under 2 * 16 e_np N ||z||_2,
    e_np the larger of numpy's two measured errors."""
    z, _, _, ref_f, npy_f, xn = case(shape, False)
    back = fft2(fft2(z), inverse=True)
    n = shape[0] * shape[1]
    err = np.abs(back - n * z)
    if pow2(shape[0]) and pow2(shape[1]):
        _, b = higham(shape)
        assert np.sqrt(np.sum(err ** 2)) <= (2 * b + b * b) * n * xn
    else:
        _, _, _, ref_i, npy_i, _ = case(shape, True)
        e_np = max(dr.abs_diff(npy_f, ref_f).max(), dr.abs_diff(npy_i, ref_i).max()) / xn
        assert err.max() <= 2 * MARGIN * e_np * n * xn + 2 * U * n * np.abs(z).max()       # + rounding n * z itself


@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "%dx%d" % s)
def test_fft2_of_real_input_is_hermitian(shape):
    """X[-k, -l] = conj(X[k, l]) for real input, to the per-bin bound of the forward test (a transpose that swaps ragged edge
    tiles breaks the symmetry by whole values)."""
    z, by, bx, ref, npy, xn = case(shape, False, True)
    got = fft2(z)
    err = dr.abs_diff(got[np.ix_(by, bx)], ref)
    e_np = dr.abs_diff(npy, ref).max() / xn
    assert err.max() / xn <= MARGIN * e_np
    if pow2(shape[0]) and pow2(shape[1]):
        t, _ = higham(shape)
        bound = 8 * U * t * np.sqrt(shape[0] * shape[1]) * xn
    else:
        bound = MARGIN * e_np * xn
    mirror = got[np.ix_((-np.arange(shape[0])) % shape[0], (-np.arange(shape[1])) % shape[1])]
    assert np.abs(got - np.conj(mirror)).max() <= bound


def test_fft2_errors():
    from tissue_image_processing_amd import _lib
    lib = _lib.lib()
    z = np.zeros((4, 4), np.complex128)
    out = np.empty_like(z)
    assert lib.tip_fft2_c128(None, _lib.ptr(out), 4, 4, 0) == -2
    assert lib.tip_fft2_c128(_lib.ptr(z), None, 4, 4, 0) == -2
    for y, x in [(1, 4), (4, 1), (4097, 4), (4, 4097)]:
        assert lib.tip_fft2_c128(_lib.ptr(z), _lib.ptr(out), y, x, 0) == -5
    with pytest.raises(NotImplementedError):
        _lib.fft2_c128(np.zeros((1, 8), np.complex128))
    with pytest.raises(NotImplementedError):
        _lib.fft2_c128(np.zeros((2, 4097), np.complex128))
    z[1, 2] = 1.0
    np.testing.assert_array_equal(_lib.fft2_c128(_lib.fft2_c128(z), inverse=True), 16 * z)


# ---- the correlation at its edges ------------------------------------------------------------------------------------------
def frames_u16(shape, seed):
    return np.random.default_rng(seed).integers(0, 30000, shape, dtype=np.uint16)


def wrapped(roll, shape):
    """the shift skimage reports for mov = np.roll(ref, roll): -roll modulo the extent, minus the extent past fix(N / 2)"""
    s = np.array([(-r) % n for r, n in zip(roll, shape)], np.float64)
    mid = np.array([np.fix(n / 2) for n in shape])
    s[s > mid] -= np.array(shape)[s > mid]
    return s


def check_roll(ref, roll, ups, mov=None):
    from tissue_image_processing_amd._registration import phase_cross_correlation
    mov = np.roll(ref, roll, axis=(0, 1)) if mov is None else mov
    want = guarded_oracle(ref, mov, ups)
    np.testing.assert_array_equal(want, wrapped(roll, ref.shape))
    got, _, _ = phase_cross_correlation(ref, mov, upsample_factor=ups)
    np.testing.assert_array_equal(got, want)


M8192_SHAPES = [(4095, 3), (3, 4095), (2049, 2), (2, 2049), (2050, 6)]


@pytest.mark.parametrize("shape", M8192_SHAPES, ids=lambda s: "%dx%d" % s)
def test_drift_8192_point_rows(shape):
    """extents 2049 .. 4095 that are no power of two: Bluestein rows of M = 8192 in 128 KiB of LDS"""
    assert any(2 * n - 1 > 4096 and not pow2(n) for n in shape)
    ref = frames_u16(shape, shape[0] + shape[1])
    check_roll(ref, ((2 * shape[0]) // 3, shape[1] // 2), 100)


def midpoint_rolls(n):
    return sorted({n // 2, (n - 1) // 2, (n + 1) // 2, 1, n - 1})


@pytest.mark.parametrize("shape", [(64, 48), (63, 49), (6, 10)], ids=lambda s: "%dx%d" % s)
def test_drift_wrap_at_the_midpoint(shape):
    """rolls of N/2 (even N: the shift stays +N/2, `shifts > midpoint` is strict), (N-1)/2 and (N+1)/2 (odd N), 1 and N-1"""
    ref = frames_u16(shape, 7 + shape[0])
    for roll in itertools.product(midpoint_rolls(shape[0]), midpoint_rolls(shape[1])):
        for ups in (1, 100):
            check_roll(ref, roll, ups)


FACTORS = [1, 2, 3, 10, 100, 1000]


def subpixel_pair(shape, shift, seed, sigma=2.0):
    """blurred content and its circular sub-pixel shift in Fourier space, both as uint16 (as test_drift_vs_oracle builds them)"""
    from oracle import oracle as orc
    base = orc.blur_image(np.random.default_rng(seed).random(shape), sigma)
    fy = np.fft.fftfreq(shape[0])[:, None]
    fx = np.fft.fftfreq(shape[1])[None, :]
    moved = np.real(np.fft.ifft2(np.fft.fft2(base) * np.exp(-2j * np.pi * (fy * shift[0] + fx * shift[1]))))
    return np.round(base * 30000).astype(np.uint16), np.round(np.clip(moved, 0, None) * 30000).astype(np.uint16)


SUBPIXEL_SHIFT = (3.27, -8.4)
# at factor 1000 two grid points 0.001 pixel apart straddle the peak: content blurred with sigma 2 (test_drift_vs_oracle's) is too
# flat there for the guard's 1e-9 (about 3e-10 for any seed), sigma 0.5 with these seeds leaves 1.2e-7 and 5.6e-8
SUBPIXEL_SIGMA, SUBPIXEL_SEED = 0.5, {(97, 64): 115, (128, 128): 148}


@pytest.mark.parametrize("ups", FACTORS)
@pytest.mark.parametrize("shape", [(97, 64), (128, 128)], ids=lambda s: "%dx%d" % s)
def test_drift_upsample_factors(shape, ups):
    """region = ceil(1.5 ups) is odd for 2, 3, 10 (3, 5, 15) and even for 100, 1000 (150, 1500)"""
    from tissue_image_processing_amd._registration import phase_cross_correlation
    check_roll(frames_u16(shape, 3 + shape[0]), (5, shape[1] - 9), ups)
    a, b = subpixel_pair(shape, SUBPIXEL_SHIFT, SUBPIXEL_SEED[shape], SUBPIXEL_SIGMA)
    want = guarded_oracle(a, b, ups)
    got, _, _ = phase_cross_correlation(a, b, upsample_factor=ups)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_allclose(got, [-SUBPIXEL_SHIFT[0], -SUBPIXEL_SHIFT[1]], atol=0.5 / ups + 0.02)


@pytest.mark.parametrize("ups", [0, 1001, -1])
def test_drift_upsample_factor_out_of_range(ups):
    from tissue_image_processing_amd._registration import phase_cross_correlation
    a = frames_u16((16, 16), 1)
    with pytest.raises(ValueError):
        phase_cross_correlation(a, np.roll(a, 3, axis=0), upsample_factor=ups)
    got, _, _ = phase_cross_correlation(a, np.roll(a, 3, axis=0), upsample_factor=1)          # the next valid call succeeds
    np.testing.assert_array_equal(got, [-3, 0])


DTYPE_SHAPE = (97, 64)


def dtype_pairs():
    a16 = frames_u16(DTYPE_SHAPE, 41)
    roll = (11, 50)
    b16 = np.roll(a16, roll, axis=(0, 1))
    f = np.random.default_rng(42).random(DTYPE_SHAPE)
    return roll, {
        "float32": (f.astype(np.float32), np.roll(f.astype(np.float32), roll, axis=(0, 1))),        # dtype 0
        "uint8": ((a16 % 251).astype(np.uint8), (b16 % 251).astype(np.uint8)),                      # other dtype -> float64
        "int32": (a16.astype(np.int32) - 15000, b16.astype(np.int32) - 15000),
        "uint16+float64": (a16, b16.astype(np.float64)),                                            # mixed -> float64
        "float64+float32": (f, np.roll(f.astype(np.float32), roll, axis=(0, 1))),
    }


@pytest.mark.parametrize("name", ["float32", "uint8", "int32", "uint16+float64", "float64+float32"])
def test_drift_dtype_branches(name):
    """every branch of _registration.phase_cross_correlation's dtype dispatch, against the oracle on the same values (the
    library promotes float32 frames to float64 exactly)"""
    roll, pairs = dtype_pairs()
    a, b = pairs[name]
    check_roll(a, roll, 100, mov=b)


@pytest.mark.parametrize("dtype", ["float32", "float64", "uint16"])
def test_drift_dev_entry_equals_host_entry(dtype):
    from tissue_image_processing_amd import _lib
    from tissue_image_processing_amd._registration import phase_cross_correlation, phase_cross_correlation_dev
    a, b = subpixel_pair((97, 64), SUBPIXEL_SHIFT, 23)
    if dtype != "uint16":
        a, b = (a / 30000.0).astype(dtype), (b / 30000.0).astype(dtype)
    want = guarded_oracle(a, b, 100)
    host, _, _ = phase_cross_correlation(a, b, upsample_factor=100)
    np.testing.assert_array_equal(host, want)
    da, db = _lib.DeviceBuffer(a.nbytes).upload(a), _lib.DeviceBuffer(b.nbytes).upload(b)
    try:
        dev = phase_cross_correlation_dev(da.ptr, db.ptr, a.shape[0], a.shape[1], 100, dtype=dtype)
    finally:
        da.free()
        db.free()
    np.testing.assert_array_equal(dev, host)


@pytest.mark.parametrize("ups", [1, 100])
@pytest.mark.parametrize("shape", [(5, 7), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_drift_argmax_takes_the_first_of_equals(shape, ups):
    """mov all zero: every |cc| is exactly 0 on both surfaces, and np.argmax's first-in-raster-order rule decides everything:
    peak (0, 0), fine peak (0, 0), shift -fix(ceil(1.5 ups) / 2) / ups per axis (0 for ups 1)"""
    from oracle import oracle as orc
    from tissue_image_processing_amd import _lib
    from tissue_image_processing_amd._registration import phase_cross_correlation
    ref = frames_u16(shape, 5)
    mov = np.zeros(shape, np.uint16)
    out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    assert _lib.lib().tip_phase_correlation(_lib.ptr(ref), _lib.ptr(mov), 3, shape[0], shape[1], ups, out) == 0
    assert list(out) == [0, 0, 0, 0]
    want = -np.fix(np.ceil(1.5 * ups) / 2) / ups if ups > 1 else 0.0
    got, _, _ = phase_cross_correlation(ref, mov, upsample_factor=ups)
    np.testing.assert_array_equal(got, [want, want])
    np.testing.assert_array_equal(got, orc.phase_cross_correlation(ref, mov, upsample_factor=ups))


def test_drift_c_abi_error_returns():
    """argument checks of tip_phase_correlation[_dev]: TIP_ERR_ARG (-2) for a null pointer and dtype 2, TIP_ERR_UNSUPPORTED (-5)
    for extents 1 and 4097; the thread's next valid call succeeds"""
    from tissue_image_processing_amd import _lib
    from tissue_image_processing_amd._registration import phase_cross_correlation
    lib = _lib.lib()
    big = frames_u16((4097, 4), 9)                 # every extent below reads at most this many elements
    a, b = _lib.ptr(big), _lib.ptr(big.copy())
    out = (ctypes.c_int64 * 4)()
    dbuf = _lib.DeviceBuffer(big.nbytes).upload(big)
    try:
        d = _lib.dptr(dbuf.ptr)
        for fn, p, q in ((lib.tip_phase_correlation, a, b), (lib.tip_phase_correlation_dev, d, d)):
            assert fn(None, q, 3, 8, 4, 100, out) == -2
            assert fn(p, None, 3, 8, 4, 100, out) == -2
            assert fn(p, q, 3, 8, 4, 100, None) == -2
            assert fn(p, q, 2, 8, 4, 100, out) == -2
            assert "dtype" in _lib.last_error()
            for y, x in [(1, 4), (4, 1), (4097, 4), (4, 4097)]:
                assert fn(p, q, 3, y, x, 100, out) == -5
            assert fn(p, q, 3, 8, 4, 100, out) == 0                       # identical frames: no shift
            assert list(out) == [0, 0, 75, 75]
    finally:
        dbuf.free()
    for shape in [(1, 16), (16, 1), (4097, 2), (2, 4097)]:
        with pytest.raises(NotImplementedError):
            phase_cross_correlation(np.zeros(shape), np.zeros(shape))
    r = frames_u16((8, 4), 2)
    got, _, _ = phase_cross_correlation(r, np.roll(r, 1, axis=1), upsample_factor=100)
    np.testing.assert_array_equal(got, [0, -1])
