"""High-precision restatement of the discrete Fourier transform, for the tests of csrc/tip_fft.hip.

    X[k] = sum_n x[n] exp(-/+ 2 pi i (n k mod N) / N)

evaluated directly (no FFT) at chosen output bins.  The phase index n * k is reduced modulo N in integers before any
floating-point step, so the argument of the exponential never exceeds 2 pi.  Two back ends, and no other fallback:

  "longdouble"  numpy's long double where it has at least 64 significand bits (x87: unit roundoff 2^-64, 2048 times finer than
                float64's); sums are numpy's pairwise ones.
  "mpmath"      mpmath at MP_BITS (>= 80) bits: the default where long double is a plain double, and the cross-check elsewhere.

A reference value stays in its back end's number type (np.clongdouble, or an object array of mpmath.mpc) so that a float64
result can be compared with it below float64's own rounding; abs_diff() takes the difference there and returns float64."""
import numpy as np

MP_BITS = 100
U = 2.0 ** -53                      # float64 unit roundoff


def longdouble_ok():
    return np.finfo(np.longdouble).nmant >= 63


def default_backend():
    return "longdouble" if longdouble_ok() else "mpmath"


def _roots_longdouble(N, inverse):
    """w[r] = exp(-/+ 2 pi i r / N), r = 0 .. N-1, as np.clongdouble"""
    ld = np.longdouble
    pi = ld(4) * np.arctan(ld(1))
    ang = (ld(2) * pi) * np.arange(N, dtype=np.longdouble) / ld(N)
    w = np.empty(N, np.clongdouble)
    w.real = np.cos(ang)
    w.imag = np.sin(ang) if inverse else -np.sin(ang)
    return w


def _rows_longdouble(rows, bins, inverse):
    R, N = rows.shape
    w = _roots_longdouble(N, inverse)
    n = np.arange(N, dtype=np.int64)
    W = w[(np.asarray(bins, np.int64)[:, None] * n[None, :]) % N]           # (K, N), phase index reduced in integers
    out = np.empty((R, len(bins)), np.clongdouble)
    for r in range(R):
        out[r] = (W * rows[r][None, :]).sum(axis=1)
    return out


def _rows_mpmath(rows, bins, inverse):
    import mpmath
    R, N = rows.shape
    with mpmath.workprec(MP_BITS):
        sign = 2 if inverse else -2
        w = [mpmath.expjpi(mpmath.mpf(sign * r) / N) for r in range(N)]
        out = np.empty((R, len(bins)), object)
        for r in range(R):
            xr = [_mpc(v) for v in rows[r]]
            for j, k in enumerate(bins):
                k = int(k)
                out[r, j] = mpmath.fsum(xr[i] * w[(i * k) % N] for i in range(N))
    return out


def _mpf(v):
    """a float64 or long double as an mpf, exactly"""
    import mpmath
    v = np.longdouble(v)
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))


def dft(x, bins=None, axis=-1, inverse=False, backend=None):
    """The DFT of x along `axis` at the output bins `bins` (default: all), unscaled in both directions (inverse = conjugate
    roots, i.e. N * ifft).  The result has len(bins) entries along `axis` and the back end's number type."""
    backend = backend or default_backend()
    if backend == "longdouble" and not longdouble_ok():
        raise RuntimeError("np.longdouble has only %d significand bits here" % (np.finfo(np.longdouble).nmant + 1))
    if backend not in ("longdouble", "mpmath"):
        raise ValueError("backend %r" % (backend,))
    x = np.asarray(x)
    if backend == "longdouble":
        x = _clongdouble_of(x) if x.dtype == object else x.astype(np.clongdouble)
    elif x.dtype != object:
        x = x.astype(np.clongdouble if longdouble_ok() else np.complex128)
    x = np.moveaxis(x, axis, -1)
    N = x.shape[-1]
    bins = np.arange(N) if bins is None else np.asarray(bins, np.int64)
    if bins.ndim != 1 or bins.size == 0 or bins.min() < 0 or bins.max() >= N:
        raise ValueError("bins must be a non-empty 1-D selection of 0 .. N-1")
    rows = x.reshape(-1, N)
    out = (_rows_longdouble if backend == "longdouble" else _rows_mpmath)(rows, bins, inverse)
    return np.moveaxis(out.reshape(x.shape[:-1] + (bins.size,)), -1, axis)


def dft2(a, bins_y=None, bins_x=None, inverse=False, backend=None):
    """The 2-D DFT of a (y, x) array at the bins bins_y x bins_x: the 1-D form along x, then along y."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("dft2 takes a 2-D array")
    return dft(dft(a, bins_x, axis=1, inverse=inverse, backend=backend), bins_y, axis=0, inverse=inverse, backend=backend)


def _clongdouble_of(obj):
    """an object array of mpmath numbers rounded to long double (through two float64 pieces per part)"""
    import mpmath
    out = np.empty(obj.size, np.clongdouble)
    with mpmath.workprec(MP_BITS):
        for i, v in enumerate(obj.reshape(-1)):
            parts = []
            for c in (mpmath.re(v), mpmath.im(v)):
                hi = float(c)
                parts.append(np.longdouble(hi) + np.longdouble(float(c - hi)))
            out[i] = parts[0] + 1j * parts[1]
    return out.reshape(obj.shape)


def _mpc(v):
    import mpmath
    return v if isinstance(v, (mpmath.mpc, mpmath.mpf)) else mpmath.mpc(_mpf(v.real), _mpf(v.imag))


def abs_diff(a, b):
    """|a - b| as float64 for two arrays of one shape, each float64 / complex128 values or a reference in a back end's number
    type; the difference is taken in the wider of the two types."""
    a = np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape:
        raise ValueError("shapes %s and %s" % (a.shape, b.shape))
    if a.dtype != object and b.dtype != object:
        return np.abs(a.astype(np.clongdouble) - b.astype(np.clongdouble)).astype(np.float64)
    import mpmath
    with mpmath.workprec(MP_BITS):
        flat = [float(abs(_mpc(p) - _mpc(q))) for p, q in zip(a.reshape(-1), b.reshape(-1))]
    return np.array(flat, np.float64).reshape(a.shape)


def norm2(x):
    """the 2-norm of all entries of a float64 / complex128 array, as a float"""
    x = np.asarray(x)
    return float(np.sqrt(np.sum(np.abs(x.astype(np.clongdouble if longdouble_ok() else np.complex128)) ** 2)))
