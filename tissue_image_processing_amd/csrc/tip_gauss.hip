// tip_gauss.hip -- separable Gaussian entry points (scipy.ndimage.gaussian_filter(mode='nearest'),
// reference call site bim.py:389 via sp.py:37,55,70,71 and ti.py:142).
#include "tip_corr.h"
#include "tip_slide.h"

namespace tip {

constexpr int LONG_TO = 256;  // outputs per line per block in the long-kernel variant
constexpr int LONG_R = 8;     // outputs per register window

// name: the launch-profiler name.  TapSrc: Taps (the table, by value) or TapsDev
template <typename T, typename TapSrc>
static int corr_generic(const char *name, const T *in, T *out, int Z, int Y, int X, int axis, const TapSrc &t)
{
    LoadPlain<T> ld{in, (long)Y * X, (long)X};
    return with_axis(axis, [&](auto A) -> int {
        TIP_LAUNCH(name, (k_corr_generic<T, decltype(A)::value, LoadPlain<T>, TapSrc>), dim3(cdiv(X, 256), Y, Z), dim3(256), 0, ld, out, Z,
                   Y, X, t);
        return TIP_OK;
    });
}
static const char *const GENERIC_NAME[2][3] = {{"corr_generic_z", "corr_generic_y", "corr_generic_x"},
                                               {"corr_generic_z_f64", "corr_generic_y_f64", "corr_generic_x_f64"}};

int corr_long_f32(const float *in, float *out, int Z, int Y, int X, int axis, const Taps &t)
{
    return with_axis<1>(axis, [&](auto A) -> int {
        constexpr int AX = decltype(A)::value;      // lanes along x (AX 1, LDS[pos][64]) or along y (AX 2, LDS[pos][65])
        const size_t lds = (size_t)(LONG_TO + 2 * (t.n >> 1)) * (AX == 1 ? 64 : 65) * sizeof(float);
        auto k = k_corr_long_f32<AX, LONG_TO, LONG_R>;
        TIP_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const dim3 grid(cdiv(AX == 1 ? X : Y, 64), cdiv(AX == 1 ? Y : X, LONG_TO), Z);
        TIP_LAUNCH(AX == 1 ? "corr_long_y" : "corr_long_x", k, grid, dim3(256), lds, in, out, Z, Y, X, t);
        return TIP_OK;
    });
}

// dtype 0 = f32, 1 = f64.  force: 0 auto, 1 generic, 2 long
int correlate1d_dev(const void *in, void *out, int dtype, int Z, int Y, int X, int axis, const Taps &t, int force)
{
    if (Z <= 0 || Y <= 0 || X <= 0) return fail(TIP_ERR_ARG, "correlate1d: empty volume");
    if (Y > 65535 || Z > 65535) return fail(TIP_ERR_ARG, "correlate1d: y and z must be <= 65535");
    if (axis < 0 || axis > 2) return fail(TIP_ERR_ARG, "correlate1d: axis %d", axis);
    if (in == out) return fail(TIP_ERR_ARG, "correlate1d: in-place is not supported");
    const int r = t.n >> 1;
    bool use_long = dtype == 0 && axis != 0 && r >= 12 && r <= 120;
    if (force == 1) use_long = false;
    if (force == 2) {
        if (dtype != 0 || axis == 0 || r > 120) return fail(TIP_ERR_ARG, "long kernel needs f32, axis 1|2, r<=120");
        use_long = true;
    }
    if (use_long) return corr_long_f32((const float *)in, (float *)out, Z, Y, X, axis, t);
    if (dtype == 0) return corr_generic(GENERIC_NAME[0][axis], (const float *)in, (float *)out, Z, Y, X, axis, t);
    if (dtype == 1) {
        // radius 12 (sigma 3, the watershed's default blur, bim.py:474) along y / x: register-sliding kernels, each
        // input loaded once per thread instead of 25 times through the caches
        if (r == 12 && axis == 1) {
            TIP_LAUNCH("yslide_r12_f64", (k_ypass_slide<double, 12, 2>), dim3(cdiv(X, 256), cdiv(Y, 50), Z), dim3(256), 0,
                       (const double *)in, (double *)out, Y, X, t);
            return TIP_OK;
        }
        if (r == 12 && axis == 2) {
            TIP_LAUNCH("xslide_r12_f64", (k_xpass_slide<double, 12>), dim3(cdiv(cdiv(X, 8), 256), Y, Z), dim3(256), 0,
                       (const double *)in, (double *)out, Y, X, t);
            return TIP_OK;
        }
        return corr_generic(GENERIC_NAME[1][axis], (const double *)in, (double *)out, Z, Y, X, axis, t);
    }
    return fail(TIP_ERR_ARG, "correlate1d: dtype %d", dtype);
}

// in -> out through up to three axis passes; `out` doubles as scratch together with one workspace.
int gaussian3d_dev(const void *in, void *out, int dtype, int Z, int Y, int X, const double *tz, int nz,
                   const double *ty, int ny, const double *tx, int nx)
{
    const size_t es = dtype == 0 ? 4 : 8;
    const size_t bytes = (size_t)Z * Y * X * es;
    const double *tp[3] = {tz, ty, tx};
    const int np_[3] = {nz, ny, nx};
    int passes = 0;
    for (int a = 0; a < 3; a++) passes += np_[a] > 0;
    if (passes == 0) {
        TIP_HIP(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, ctx().stream));
        return TIP_OK;
    }
    WsGuard ws;
    void *tmp = nullptr;
    if (passes > 1) {
        tmp = ws.get<char>(bytes);
        if (!tmp) return TIP_ERR_NOMEM;
    }
    // ping-pong so that the last pass lands in `out`
    const void *cur = in;
    int done = 0;
    for (int a = 0; a < 3; a++) {
        if (np_[a] <= 0) continue;
        const int remaining = passes - done - 1;
        void *dst = (remaining % 2 == 0) ? out : tmp;
        int rc;
        if (np_[a] > 255) {
            // radius > 127 (sigma > 31.8): more taps than the kernel-argument tap table holds; they go to device memory and a
            // the generic kernel walks them there in scipy's order (no reference call site is this wide: slow path)
            const int n = np_[a];
            if (n % 2 == 0 || n > 8191) return fail(TIP_ERR_ARG, "gaussian: %d taps (odd, at most 8191)", n);
            for (int i = 0; i < n / 2; ++i)
                if (tp[a][i] != tp[a][n - 1 - i]) return fail(TIP_ERR_ARG, "gaussian: taps must be symmetric");
            double *wd = ws.get<double>((size_t)n);
            if (!wd) return TIP_ERR_NOMEM;
            TIP_HIP(hipMemcpyAsync(wd, tp[a], (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
            TIP_HIP(hipStreamSynchronize(ctx().stream));      // (the host tap array may be a temporary of the caller)
            const TapsDev td{wd, n};
            rc = dtype == 0 ? corr_generic("corr_big", (const float *)cur, (float *)dst, Z, Y, X, a, td)
                            : corr_generic("corr_big", (const double *)cur, (double *)dst, Z, Y, X, a, td);
            if (rc) return rc;
        } else {
            Taps t;
            rc = make_taps(t, tp[a], np_[a]);
            if (rc) return rc;
            rc = correlate1d_dev(cur, dst, dtype, Z, Y, X, a, t, 0);
            if (rc) return rc;
        }
        cur = dst;
        done++;
    }
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_correlate1d_dev(const void *in, void *out, int dtype, int z, int y, int x, int axis, const double *taps_host,
                        int n)
{
    if (!in || !out || !taps_host) return fail(TIP_ERR_ARG, "tip_correlate1d_dev: null pointer");
    int force = 0;
    if (axis >= 100) { force = axis / 100; axis %= 100; }  // test hook: 1xx generic, 2xx long kernel
    Taps t;
    int rc = make_taps(t, taps_host, n);
    if (rc) return rc;
    return correlate1d_dev(in, out, dtype, z, y, x, axis, t, force);
}

int tip_gaussian3d_dev_w(const void *in, void *out, int dtype, int z, int y, int x, const double *tz, int nz,
                         const double *ty, int ny, const double *tx, int nx)
{
    if (!in || !out) return fail(TIP_ERR_ARG, "tip_gaussian3d_dev_w: null pointer");
    if (dtype != 0 && dtype != 1) return fail(TIP_ERR_ARG, "dtype must be 0 (f32) or 1 (f64)");
    return gaussian3d_dev(in, out, dtype, z, y, x, tz, nz, ty, ny, tx, nx);
}

int tip_gaussian3d_w(const void *in, void *out, int dtype, int z, int y, int x, const double *tz, int nz,
                     const double *ty, int ny, const double *tx, int nx)
{
    if (!in || !out) return fail(TIP_ERR_ARG, "tip_gaussian3d_w: null pointer");
    if (dtype != 0 && dtype != 1) return fail(TIP_ERR_ARG, "dtype must be 0 (f32) or 1 (f64)");
    if (z <= 0 || y <= 0 || x <= 0) return fail(TIP_ERR_ARG, "empty volume");
    if (!ctx().stream) return TIP_ERR_HIP;
    const size_t bytes = (size_t)z * y * x * (dtype == 0 ? 4 : 8);
    Staging st;
    const char *din = st.in((const char *)in, bytes);
    char *dout = st.out((char *)out, bytes);
    if (st.rc) return st.rc;
    int rc = gaussian3d_dev(din, dout, dtype, z, y, x, tz, nz, ty, ny, tx, nx);
    if (rc) return rc;
    return st.finish();
}

static int taps_for(double sigma, double truncate, double *buf, int *n)
{
    *n = 0;
    if (sigma > 1e-15) {
        int k = libm_taps(sigma, truncate, buf, 255);
        if (k < 0) return fail(TIP_ERR_ARG, "sigma %g too large (radius > 127)", sigma);
        *n = k;
    }
    return TIP_OK;
}

int tip_gaussian3d_f32(const float *in, float *out, int z, int y, int x, double sz, double sy, double sx,
                       double truncate)
{
    double tz[256], ty[256], tx[256];
    int nz, ny, nx, rc;
    if ((rc = taps_for(sz, truncate, tz, &nz)) || (rc = taps_for(sy, truncate, ty, &ny)) ||
        (rc = taps_for(sx, truncate, tx, &nx)))
        return rc;
    return tip_gaussian3d_w(in, out, 0, z, y, x, tz, nz, ty, ny, tx, nx);
}

int tip_gaussian2d_f64(const double *in, double *out, int y, int x, double sy, double sx, double truncate)
{
    double ty[256], tx[256];
    int ny, nx, rc;
    if ((rc = taps_for(sy, truncate, ty, &ny)) || (rc = taps_for(sx, truncate, tx, &nx))) return rc;
    return tip_gaussian3d_w(in, out, 1, 1, y, x, nullptr, 0, ty, ny, tx, nx);
}

}  // extern "C"
