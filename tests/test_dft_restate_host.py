"""CPU: the high-precision DFT of tests/dft_restate.py against closed forms that need no FFT."""
import numpy as np
import pytest

import dft_restate as dr

LENGTHS = [2, 3, 97, 2049, 4095, 4096]
# what the long double evaluation may be off by, relative to ||x||_2: every term carries a root of unity good to a few 2^-64
# (argument 2 pi r / N rounded three times, then cosl / sinl) and one product; a pairwise sum of N <= 4096 terms adds
# log2 N roundings.  2^-58 = 64 * 2^-64 covers that and is still 1/32 of float64's unit roundoff.
TOL = 2.0 ** -58


def sample_bins(N, count=8):
    fixed = {0, 1 % N, N // 2, N - 1}
    extra = np.random.default_rng(N).integers(0, N, count)
    return np.array(sorted(fixed | set(int(v) for v in extra)))


def exact_roots(nums, N):
    """exp(-2 pi i num / N) for every num, from mpmath: an object array of mpc good to MP_BITS bits"""
    import mpmath
    with mpmath.workprec(dr.MP_BITS):
        flat = [mpmath.expjpi(mpmath.mpf(-2 * (int(v) % N)) / N) for v in np.asarray(nums).reshape(-1)]
    out = np.empty(len(flat), object)
    out[:] = flat
    return out.reshape(np.shape(nums))


def conj(obj):
    import mpmath
    out = np.empty(obj.size, object)
    with mpmath.workprec(dr.MP_BITS):
        out[:] = [v.conjugate() for v in obj.reshape(-1)]
    return out.reshape(obj.shape)


def backends():
    return [b for b in ("longdouble", "mpmath") if b == "mpmath" or dr.longdouble_ok()]


def test_a_backend_exists():
    assert dr.default_backend() in backends()
    if not dr.longdouble_ok():
        import mpmath  # noqa: F401  (the only fallback)


def combine(amps, arrays):
    """sum_i amps[i] * arrays[i] at MP_BITS bits (arrays in either back end's number type), as an object array of mpc"""
    import mpmath
    with mpmath.workprec(dr.MP_BITS):
        acc = [mpmath.mpc(0) for _ in range(arrays[0].size)]
        for a, arr in zip(amps, arrays):
            a = dr._mpc(a)
            acc = [s + a * dr._mpc(v) for s, v in zip(acc, arr.reshape(-1))]
    out = np.empty(len(acc), object)
    out[:] = acc
    return out.reshape(arrays[0].shape)


@pytest.mark.parametrize("N", LENGTHS)
def test_impulse(N):
    """x = delta[n - n0]  ->  X[k] = exp(-2 pi i k n0 / N)"""
    bins = sample_bins(N)
    for n0 in sorted({0, 1, N // 3, N - 1}):
        x = np.zeros(N)
        x[n0] = 1.0
        want = exact_roots(bins * n0, N)
        assert dr.abs_diff(dr.dft(x, bins), want).max() <= TOL
        assert dr.abs_diff(dr.dft(x, bins, inverse=True), conj(want)).max() <= TOL


@pytest.mark.parametrize("N", LENGTHS)
def test_single_tone(N):
    """x[n] = exp(+2 pi i j n / N)  ->  X[k] = N delta[k - j]; the tone's samples come from mpmath"""
    for j in sorted({0, 1, N // 2, N - 1}):
        tone = conj(exact_roots(j * np.arange(N), N))
        bins = np.array(sorted(set(sample_bins(N).tolist()) | {j}))
        want = np.where(bins == j, float(N), 0.0)
        assert dr.abs_diff(dr.dft(tone, bins), want).max() <= TOL * np.sqrt(N)            # ||tone||_2 = sqrt(N)


@pytest.mark.parametrize("N", LENGTHS)
def test_linearity_three_impulses(N):
    rng = np.random.default_rng(100 + N)
    pos = rng.choice(N, size=min(3, N), replace=False)
    amp = rng.standard_normal(pos.size) + 1j * rng.standard_normal(pos.size)
    bins = sample_bins(N)
    x = np.zeros(N, np.complex128)
    x[pos] = amp
    got = dr.dft(x, bins)
    singles = []
    for p in pos:
        e = np.zeros(N)
        e[p] = 1.0
        singles.append(dr.dft(e, bins))
    assert dr.abs_diff(got, combine(amp, singles)).max() <= TOL * dr.norm2(x)
    assert dr.abs_diff(got, combine(amp, [exact_roots(bins * int(p), N) for p in pos])).max() <= TOL * dr.norm2(x)


@pytest.mark.parametrize("N", LENGTHS)
def test_backends_agree(N):
    if len(backends()) < 2:
        pytest.skip("np.longdouble is a plain double here: mpmath is the only back end")
    rng = np.random.default_rng(200 + N)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    bins = sample_bins(N, 4) if N > 97 else np.arange(N)
    a = dr.dft(x, bins, backend="longdouble")
    b = dr.dft(x, bins, backend="mpmath")
    assert dr.abs_diff(a, b).max() <= 1e-17 * dr.norm2(x)


def test_two_dimensions_and_axes():
    """dft2 = the 1-D form along both axes; an impulse at (y0, x0) gives the product of the two roots"""
    Ny, Nx = 5, 7
    a = np.zeros((Ny, Nx))
    a[3, 2] = 1.0
    by, bx = np.array([0, 1, 4]), np.array([0, 3, 6, 5])
    got = dr.dft2(a, by, bx)
    want = exact_roots(by[:, None] * 3 * Nx + bx[None, :] * 2 * Ny, Ny * Nx)      # k 3 / 5 + l 2 / 7 over the common 35
    assert got.shape == (3, 4) and dr.abs_diff(got, want).max() <= TOL
    rng = np.random.default_rng(5)
    z = rng.standard_normal((Ny, Nx)) + 1j * rng.standard_normal((Ny, Nx))
    full = dr.dft2(z)
    assert dr.abs_diff(np.fft.fft2(z), full).max() <= 64 * dr.U * dr.norm2(z)      # numpy agrees to float64 precision
    assert dr.abs_diff(dr.dft(z, axis=0), np.moveaxis(dr.dft(z.T.copy(), axis=1), 0, 1)).max() == 0


def test_bins_are_checked():
    with pytest.raises(ValueError):
        dr.dft(np.ones(4), [4])
    with pytest.raises(ValueError):
        dr.dft(np.ones(4), [-1])
    with pytest.raises(ValueError):
        dr.dft(np.ones(4), backend="float32")
