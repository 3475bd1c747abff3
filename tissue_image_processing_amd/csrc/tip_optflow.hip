// tip_optflow.hip -- skimage.registration.optical_flow_tvl1 (scikit-image 0.18.3, 2-D, float32, prefilter=False) on the
// device: the PIV drift of Tissue.track_cells_iterator(use_piv=True) (ti.py:2061-2070).
//
// Every expression keeps scikit-image's float32 operation order and rounding (the library is built with
// -ffp-contract=off); the two interpolations run in double and round once to float32 like scipy's map_coordinates and
// skimage's _warp_fast.  Two things differ: the stopping test's sum (double here, numpy's float32 pairwise sum upstream)
// and the Gaussian taps' exp() (the host's libm, numpy's own upstream).  DESIGN.md section 9 has the numerical contract.
//
// One level, one warp:  k_of_warp (bilinear sample, 'nearest' border) -> k_of_prep (np.gradient, NI, rho_0) ->
// num_iter x k_of_iter (data step + both components' two regularisation steps, fused over an LDS tile) -> k_of_diff +
// k_of_check (the stopping test).  Every kernel of a level reads the level's `done` flag first and returns when the test
// has passed, so an early stop costs no host round trip.
#include "tip_internal.h"
#include <cmath>

namespace tip {

namespace {

constexpr int OF_TX = 32, OF_TY = 16;                 // k_of_iter's output tile (cols x rows), 256 threads
constexpr int OF_MAX_LEVELS = 10;

__global__ void __launch_bounds__(256) k_of_convert(const void *__restrict__ src, int dtype, float *__restrict__ dst, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v;
    if (dtype == 0) v = ((const float *)src)[i];
    else if (dtype == 1) v = (float)((const double *)src)[i];
    else if (dtype == 3) v = (float)((const uint16_t *)src)[i] * (float)(1.0 / 65535.0);   // np.multiply(img, 1/imax, dtype=float32)
    else if (dtype == OF_F64_AS_U16) {
        // a float64 plane as the GUI loads it: astype(uint16) first (truncation; outside [0, 65535] the x86 cast's int32
        // wrap, NaN and values past int32 give 0), then as code 3
        const double d = trunc(((const double *)src)[i]);
        const uint16_t u = (d >= -2147483648.0 && d <= 2147483647.0) ? (uint16_t)(int32_t)d : (uint16_t)0;
        v = (float)u * (float)(1.0 / 65535.0);
    }
    else v = (float)((const uint8_t *)src)[i] * (float)(1.0 / 255.0);
    dst[i] = v;
}

struct Taps7 { double w[7]; };

// ndi.gaussian_filter(sigma=2/3, mode='reflect') one axis at a time into float32: double accumulation in scipy's
// symmetric-kernel order (centre, then the outermost pair inwards).  blockIdx.z selects the frame.
template <int AXIS>
__global__ void __launch_bounds__(256) k_of_blur(const float *__restrict__ in0, const float *__restrict__ in1,
                                                 float *__restrict__ out0, float *__restrict__ out1, int H, int W, Taps7 t)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= W) return;
    const float *in = blockIdx.z ? in1 : in0;
    float *out = blockIdx.z ? out1 : out0;
    const int n = AXIS == 0 ? H : W, c = AXIS == 0 ? i : j;
    auto at = [&](int k) -> double {
        k = k < 0 ? -k - 1 : (k >= n ? 2 * n - 1 - k : k);
        k = k < 0 ? 0 : (k >= n ? n - 1 : k);
        return AXIS == 0 ? (double)in[(long)k * W + j] : (double)in[(long)i * W + k];
    };
    double acc = at(c) * t.w[3];
    for (int q = 3; q >= 1; q--) acc = acc + (at(c - q) + at(c + q)) * t.w[3 + q];
    out[(long)i * W + j] = (float)acc;
}

// resize(order=1, mode='reflect') to ceil(shape/2): _warp_fast's metric transform in float32, skimage's bilinear
// interpolation in double (the coordinates stay inside the image, so the border mode never applies).
__global__ void __launch_bounds__(256) k_of_decimate(const float *__restrict__ in0, const float *__restrict__ in1,
                                                     float *__restrict__ out0, float *__restrict__ out1, int H, int W, int h,
                                                     int w, float ar, float br, float ac, float bc)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= w) return;
    const float *in = blockIdx.z ? in1 : in0;
    float *out = blockIdx.z ? out1 : out0;
    const float r = ar * (float)i + br, c = ac * (float)j + bc;
    int r0 = (int)floorf(r), c0 = (int)floorf(c), r1 = (int)ceilf(r), c1 = (int)ceilf(c);
    const double dr = (double)r - r0, dc = (double)c - c0;
    r0 = min(max(r0, 0), H - 1); r1 = min(max(r1, 0), H - 1);
    c0 = min(max(c0, 0), W - 1); c1 = min(max(c1, 0), W - 1);
    const double top = (1 - dc) * (double)in[(long)r0 * W + c0] + dc * (double)in[(long)r0 * W + c1];
    const double bot = (1 - dc) * (double)in[(long)r1 * W + c0] + dc * (double)in[(long)r1 * W + c1];
    out[(long)i * w + j] = (float)((1 - dr) * top + dr * bot);
}

// resize_flow: ndi.zoom(order=0, mode='nearest') from (h, w) to (H, W), each component times new/old in float32
__global__ void __launch_bounds__(256) k_of_resize(const float *__restrict__ u, float *__restrict__ v, int h, int w, int H,
                                                   int W, double zr, double zc, float sr, float sc)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= W) return;
    const int si = min((int)floor((double)i * zr + 0.5), h - 1), sj = min((int)floor((double)j * zc + 0.5), w - 1);
    const long n = (long)h * w, N = (long)H * W;
    v[(long)i * W + j] = sr * u[(long)si * w + sj];
    v[N + (long)i * W + j] = sc * u[n + (long)si * w + sj];
}

// one warp's image: map_coordinates(mov, grid + flow, order=1, mode='nearest') into float32; counts the warp
__global__ void __launch_bounds__(256) k_of_warp(const float *__restrict__ mov, const float *__restrict__ u,
                                                 float *__restrict__ wimg, int H, int W, const int *__restrict__ done,
                                                 int *__restrict__ count)
{
    if (*done) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *count += 1;
    if (j >= W) return;
    const long p = (long)i * W + j, n = (long)H * W;
    double r = (double)(u[p] + (float)i), c = (double)(u[n + p] + (float)j);
    r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
    c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
    if (r != r) r = 0;                                   // (a NaN flow: keep the reads inside the image)
    if (c != c) c = 0;
    const int r0 = (int)floor(r), c0 = (int)floor(c);
    const double tr = r - r0, tc = c - c0;
    const int r1 = min(r0 + 1, H - 1), c1 = min(c0 + 1, W - 1);
    double t = (double)mov[(long)r0 * W + c0] * (1 - tr) * (1 - tc);
    t = t + (double)mov[(long)r0 * W + c1] * (1 - tr) * tc;
    t = t + (double)mov[(long)r1 * W + c0] * tr * (1 - tc);
    t = t + (double)mov[(long)r1 * W + c1] * tr * tc;
    wimg[p] = (float)t;
}

// np.gradient of the warped image, NI = |grad|^2 (1 where 0), rho_0 = warped - ref - grad . flow
__global__ void __launch_bounds__(256) k_of_prep(const float *__restrict__ wimg, const float *__restrict__ ref,
                                                 const float *__restrict__ u, float *__restrict__ grad, float *__restrict__ NI,
                                                 float *__restrict__ rho0, int H, int W, const int *__restrict__ done)
{
    if (*done) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= W) return;
    const long p = (long)i * W + j, n = (long)H * W;
    float g0, g1;
    if (i == 0) g0 = wimg[p + W] - wimg[p];
    else if (i == H - 1) g0 = wimg[p] - wimg[p - W];
    else g0 = (wimg[p + W] - wimg[p - W]) / 2.0f;
    if (j == 0) g1 = wimg[p + 1] - wimg[p];
    else if (j == W - 1) g1 = wimg[p] - wimg[p - 1];
    else g1 = (wimg[p + 1] - wimg[p - 1]) / 2.0f;
    float ni = g0 * g0 + g1 * g1;
    if (ni == 0.0f) ni = 1.0f;
    grad[p] = g0;
    grad[n + p] = g1;
    NI[p] = ni;
    rho0[p] = (wimg[p] - ref[p]) - (g0 * u[p] + g1 * u[n + p]);
}

// One inner iteration, fused: the data step on the tile plus a 2-pixel halo, then for each component the two
// regularisation steps (forward differences, the proj update, the backward divergence).  The output tile of u and proj
// goes to the other ping-pong buffers, so no tile reads a neighbour's new values; the halo is recomputed, with the
// same arithmetic, by every tile that needs it.  Pixels outside the frame hold zeros and are never read by one inside
// (g is 0 on the last row / column, the divergence skips the first).  `snap` (first iteration of a warp only) keeps the
// flow after the data step: skimage's flow_previous aliases it (the stopping test's quirk).
constexpr int RA_Y = OF_TY + 4, RA_X = OF_TX + 4;   // data step:   rows r0-2 .. r0+TY+1
constexpr int R1_Y = OF_TY + 3, R1_X = OF_TX + 3;   // first proj:  rows r0-2 .. r0+TY
constexpr int R2_Y = OF_TY + 2, R2_X = OF_TX + 2;   // first flow:  rows r0-1 .. r0+TY
constexpr int R3_Y = OF_TY + 1, R3_X = OF_TX + 1;   // second proj: rows r0-1 .. r0+TY-1

__global__ void __launch_bounds__(256) k_of_iter(const float *__restrict__ u_in, const float *__restrict__ p_in,
                                                 float *__restrict__ u_out, float *__restrict__ p_out,
                                                 const float *__restrict__ grad, const float *__restrict__ NI,
                                                 const float *__restrict__ rho0, float *__restrict__ snap, int H, int W,
                                                 float f0, float f1, const int *__restrict__ done)
{
    if (*done) return;
    __shared__ float s_ua[2][RA_Y][RA_X];
    __shared__ float s_p1[2][R1_Y][R1_X];
    __shared__ float s_u1[R2_Y][R2_X];
    __shared__ float s_p2[2][R3_Y][R3_X];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * OF_TY, c0 = blockIdx.x * OF_TX;
    const long n = (long)H * W;

    // data step (skimage's flow_auxiliary) over the tile + 2-pixel halo
    for (int e = tid; e < RA_Y * RA_X; e += 256) {
        const int ly = e / RA_X, lx = e % RA_X, gi = r0 - 2 + ly, gj = c0 - 2 + lx;
        float a0 = 0.0f, a1 = 0.0f;
        if (gi >= 0 && gi < H && gj >= 0 && gj < W) {
            const long p = (long)gi * W + gj;
            const float u0 = u_in[p], u1 = u_in[n + p], g0 = grad[p], g1 = grad[n + p], ni = NI[p];
            const float rho = rho0[p] + (g0 * u0 + g1 * u1);
            if (fabsf(rho) <= f0 * ni) {
                a0 = u0 - rho * g0 / ni;
                a1 = u1 - rho * g1 / ni;
            } else {
                const float srho = f0 * (rho > 0.0f ? 1.0f : (rho < 0.0f ? -1.0f : rho));   // np.sign (NaN stays NaN)
                a0 = u0 - srho * g0;
                a1 = u1 - srho * g1;
            }
            if (snap && ly >= 2 && ly < 2 + OF_TY && lx >= 2 && lx < 2 + OF_TX) {
                snap[p] = a0;
                snap[n + p] = a1;
            }
        }
        s_ua[0][ly][lx] = a0;
        s_ua[1][ly][lx] = a1;
    }
    __syncthreads();

    for (int k = 0; k < 2; k++) {
        const float *pk = p_in + 2 * k * n;
        // first regularisation step: proj from the data-step flow (region R1, offset 2)
        for (int e = tid; e < R1_Y * R1_X; e += 256) {
            const int ly = e / R1_X, lx = e % R1_X, gi = r0 - 2 + ly, gj = c0 - 2 + lx;
            float q0 = 0.0f, q1 = 0.0f;
            if (gi >= 0 && gi < H && gj >= 0 && gj < W) {
                const long p = (long)gi * W + gj;
                const float uc = s_ua[k][ly][lx];
                const float g0 = gi < H - 1 ? s_ua[k][ly + 1][lx] - uc : 0.0f;
                const float g1 = gj < W - 1 ? s_ua[k][ly][lx + 1] - uc : 0.0f;
                float norm = sqrtf(g0 * g0 + g1 * g1);
                norm = norm * f1;
                norm = norm + 1.0f;
                q0 = (pk[p] - 0.25f * g0) / norm;
                q1 = (pk[n + p] - 0.25f * g1) / norm;
            }
            s_p1[0][ly][lx] = q0;
            s_p1[1][ly][lx] = q1;
        }
        __syncthreads();
        // ... and the flow it gives (region R2, offset 1)
        for (int e = tid; e < R2_Y * R2_X; e += 256) {
            const int ly = e / R2_X, lx = e % R2_X, gi = r0 - 1 + ly, gj = c0 - 1 + lx;
            float d = -(s_p1[0][ly + 1][lx + 1] + s_p1[1][ly + 1][lx + 1]);
            if (gi >= 1) d = d + s_p1[0][ly][lx + 1];
            if (gj >= 1) d = d + s_p1[1][ly + 1][lx];
            s_u1[ly][lx] = s_ua[k][ly + 1][lx + 1] + d;
        }
        __syncthreads();
        // second regularisation step: proj (region R3, offset 1)
        for (int e = tid; e < R3_Y * R3_X; e += 256) {
            const int ly = e / R3_X, lx = e % R3_X, gi = r0 - 1 + ly, gj = c0 - 1 + lx;
            const float uc = s_u1[ly][lx];
            const float g0 = gi < H - 1 ? s_u1[ly + 1][lx] - uc : 0.0f;
            const float g1 = gj < W - 1 ? s_u1[ly][lx + 1] - uc : 0.0f;
            float norm = sqrtf(g0 * g0 + g1 * g1);
            norm = norm * f1;
            norm = norm + 1.0f;
            s_p2[0][ly][lx] = (s_p1[0][ly + 1][lx + 1] - 0.25f * g0) / norm;
            s_p2[1][ly][lx] = (s_p1[1][ly + 1][lx + 1] - 0.25f * g1) / norm;
        }
        __syncthreads();
        // ... and the final flow on the tile
        for (int e = tid; e < OF_TY * OF_TX; e += 256) {
            const int ly = e / OF_TX, lx = e % OF_TX, gi = r0 + ly, gj = c0 + lx;
            if (gi >= H || gj >= W) continue;
            const long p = (long)gi * W + gj;
            const float q0 = s_p2[0][ly + 1][lx + 1], q1 = s_p2[1][ly + 1][lx + 1];
            float d = -(q0 + q1);
            if (gi >= 1) d = d + s_p2[0][ly][lx + 1];
            if (gj >= 1) d = d + s_p2[1][ly + 1][lx];
            u_out[k * n + p] = s_ua[k][ly + 2][lx + 2] + d;
            p_out[2 * k * n + p] = q0;
            p_out[(2 * k + 1) * n + p] = q1;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_of_copy(const float *__restrict__ a, float *__restrict__ b, long n,
                                                 const int *__restrict__ done)
{
    if (*done) return;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = a[i];
}

// the stopping test's sum((flow_previous - flow_current)^2), squares in float32, accumulated in double
__global__ void __launch_bounds__(256) k_of_diff(const float *__restrict__ snap, const float *__restrict__ u, long n,
                                                 double *__restrict__ acc, const int *__restrict__ done)
{
    if (*done) return;
    __shared__ double part[4];
    double s = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float d0 = snap[i] - u[i], d1 = snap[n + i] - u[n + i];
        s += (double)(d0 * d0) + (double)(d1 * d1);
    }
    s = block_sum<4>(s, part);                   // (the order of the additions is block_reduce's)
    if (threadIdx.x == 0) atomicAdd(acc, s);
}

__global__ void k_of_check(const double *__restrict__ acc, double tol, int *__restrict__ done)
{
    if (*done) return;
    if (*acc < tol) *done = 1;
}

struct Level { int H, W; float *ref, *mov; };

}  // namespace

// ref, mov: device (y, x) planes of `dtype` (0 f32, 1 f64, 3 u16, 4 u8, or the internal OF_F64_AS_U16); flow_out: device
// (2, y, x) float32; warps_host: NULL or a host array of `cap` ints (then the call waits for the stream)
int optical_flow_tvl1_dev(const void *ref, const void *mov, int dtype, int y, int x, float attachment, float tightness,
                          int num_warp, int num_iter, double tol, float *flow_out, int32_t *warps_host, int cap)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!ref || !mov || !flow_out) return fail(TIP_ERR_ARG, "tip_optical_flow_tvl1: null pointer");
    if (y < 2 || x < 2) return fail(TIP_ERR_ARG, "tip_optical_flow_tvl1: frames need at least 2 rows and 2 columns (got %dx%d)", y, x);
    if (dtype != 0 && dtype != 1 && dtype != 3 && dtype != 4 && dtype != OF_F64_AS_U16)
        return fail(TIP_ERR_ARG, "tip_optical_flow_tvl1: dtype %d (0 f32, 1 f64, 3 u16, 4 u8)", dtype);
    // get_pyramid(downscale=2, nlevel=10, min_size=16): reduce while min(shape) > 32
    Level lv[OF_MAX_LEVELS];
    int nl = 1;
    lv[0].H = y; lv[0].W = x;
    while (nl < OF_MAX_LEVELS && std::min(lv[nl - 1].H, lv[nl - 1].W) > 32) {
        lv[nl].H = (lv[nl - 1].H + 1) / 2;
        lv[nl].W = (lv[nl - 1].W + 1) / 2;
        nl++;
    }
    if (warps_host && cap < nl) return fail(TIP_ERR_OVERFLOW, "tip_optical_flow_tvl1: %d levels, capacity %d", nl, cap);
    const long N = (long)y * x;
    long pyr = 0;
    for (int l = 0; l < nl; l++) pyr += (long)lv[l].H * lv[l].W;
    WsGuard ws;
    float *pbuf = ws.get<float>(2 * pyr);
    float *blur = ws.get<float>(2 * N);             // the axis-0 pass of both frames
    float *ux = ws.get<float>(2 * N), *uy = ws.get<float>(2 * N), *upong = ws.get<float>(2 * N), *snap = ws.get<float>(2 * N);
    float *pa = ws.get<float>(4 * N), *pb = ws.get<float>(4 * N);
    float *wimg = ws.get<float>(N), *grad = ws.get<float>(2 * N), *NI = ws.get<float>(N), *rho0 = ws.get<float>(N);
    int *flags = ws.get<int>(2 * OF_MAX_LEVELS);     // done[level], count[level]
    double *acc = ws.get<double>((size_t)OF_MAX_LEVELS * std::max(num_warp, 1));
    if (!pbuf || !blur || !ux || !uy || !upong || !snap || !pa || !pb || !wimg || !grad || !NI || !rho0 || !flags || !acc)
        return TIP_ERR_NOMEM;
    int *done = flags, *count = flags + OF_MAX_LEVELS;
    TIP_HIP(hipMemsetAsync(flags, 0, 2 * OF_MAX_LEVELS * sizeof(int), c.stream));
    TIP_HIP(hipMemsetAsync(acc, 0, (size_t)OF_MAX_LEVELS * std::max(num_warp, 1) * sizeof(double), c.stream));

    // pyramid, finest level first: lv[l] is the l-th reduction
    {
        float *q = pbuf;
        for (int l = 0; l < nl; l++) {
            const long m = (long)lv[l].H * lv[l].W;
            lv[l].ref = q; lv[l].mov = q + m;
            q += 2 * m;
        }
    }
    TIP_LAUNCH("of_convert", k_of_convert, dim3(cdiv(N, 256)), dim3(256), 0, ref, dtype, lv[0].ref, N);
    TIP_LAUNCH("of_convert", k_of_convert, dim3(cdiv(N, 256)), dim3(256), 0, mov, dtype, lv[0].mov, N);
    if (nl > 1) {
        Taps7 t;
        const double sigma = 2 * 2 / 6.0, s2 = sigma * sigma;
        double sum = 0.0;
        for (int q = 0; q < 7; q++) { const double xx = q - 3; t.w[q] = exp(-0.5 / s2 * (xx * xx)); }
        for (int q = 0; q < 7; q++) sum += t.w[q];
        for (int q = 0; q < 7; q++) t.w[q] = t.w[q] / sum;
        for (int l = 1; l < nl; l++) {
            const int H = lv[l - 1].H, W = lv[l - 1].W, h = lv[l].H, w = lv[l].W;
            float *b0 = blur, *b1 = blur + (long)H * W;
            float *s0 = wimg, *s1 = grad;             // (free until the first warp: the smoothed frames)
            TIP_LAUNCH("of_blur0", k_of_blur<0>, dim3(cdiv(W, 256), H, 2), dim3(256), 0, (const float *)lv[l - 1].ref,
                       (const float *)lv[l - 1].mov, b0, b1, H, W, t);
            TIP_LAUNCH("of_blur1", k_of_blur<1>, dim3(cdiv(W, 256), H, 2), dim3(256), 0, (const float *)b0, (const float *)b1,
                       s0, s1, H, W, t);
            const double ar = (double)H / h, ac = (double)W / w;
            TIP_LAUNCH("of_decimate", k_of_decimate, dim3(cdiv(w, 256), h, 2), dim3(256), 0, (const float *)s0,
                       (const float *)s1, lv[l].ref, lv[l].mov, H, W, h, w, (float)ar, (float)(0.5 * ar - 0.5), (float)ac,
                       (float)(0.5 * ac - 0.5));
        }
    }

    const bool run = num_warp >= 1 && num_iter >= 1;
    const float f0 = (float)((double)attachment * (double)tightness), f1 = (float)(0.25 / (double)tightness);
    float *prev = nullptr;                            // the previous (coarser) level's flow
    for (int l = nl - 1; l >= 0; l--) {
        const int H = lv[l].H, W = lv[l].W;
        const long n = (long)H * W;
        float *ua = l == 0 ? flow_out : ((l & 1) ? ux : uy);   // this level's flow (alternates, never prev)
        const dim3 rows(cdiv(W, 256), H);
        if (l == nl - 1) {
            TIP_HIP(hipMemsetAsync(ua, 0, 2 * n * sizeof(float), c.stream));
        } else {
            const int h = lv[l + 1].H, w = lv[l + 1].W;
            const double zr = H > 1 ? (double)(h - 1) / (H - 1) : 1.0, zc = W > 1 ? (double)(w - 1) / (W - 1) : 1.0;
            TIP_LAUNCH("of_resize", k_of_resize, rows, dim3(256), 0, (const float *)prev, ua, h, w, H, W, zr, zc,
                       (float)((double)H / h), (float)((double)W / w));
        }
        prev = ua;
        if (!run) continue;            // the flow stays 0 (num_iter == 0: one warp per level, whose test passes at once)
        TIP_HIP(hipMemsetAsync(pa, 0, 4 * n * sizeof(float), c.stream));
        const double tol_l = tol * (double)n;
        const dim3 tiles(cdiv(W, OF_TX), cdiv(H, OF_TY));
        for (int wp = 0; wp < num_warp; wp++) {
            TIP_LAUNCH("of_warp", k_of_warp, rows, dim3(256), 0, (const float *)lv[l].mov, (const float *)ua, wimg, H, W,
                       (const int *)(done + l), count + l);
            TIP_LAUNCH("of_prep", k_of_prep, rows, dim3(256), 0, (const float *)wimg, (const float *)lv[l].ref,
                       (const float *)ua, grad, NI, rho0, H, W, (const int *)(done + l));
            float *uin = ua, *uout = upong, *pin = pa, *pout = pb;
            for (int it = 0; it < num_iter; it++) {
                TIP_LAUNCH("of_iter", k_of_iter, tiles, dim3(256), 0, (const float *)uin, (const float *)pin, uout, pout,
                           (const float *)grad, (const float *)NI, (const float *)rho0, it == 0 ? snap : (float *)nullptr, H, W,
                           f0, f1, (const int *)(done + l));
                std::swap(uin, uout);
                std::swap(pin, pout);
            }
            if (num_iter & 1) {        // bring the result back to (ua, pa)
                TIP_LAUNCH("of_copy", k_of_copy, dim3(cdiv(2 * n, 256)), dim3(256), 0, (const float *)upong, ua, 2 * n,
                           (const int *)(done + l));
                TIP_LAUNCH("of_copy", k_of_copy, dim3(cdiv(4 * n, 256)), dim3(256), 0, (const float *)pb, pa, 4 * n,
                           (const int *)(done + l));
            }
            double *a = acc + (size_t)l * num_warp + wp;
            TIP_LAUNCH("of_diff", k_of_diff, dim3(std::min(cdiv(n, 256), 1024)), dim3(256), 0, (const float *)snap,
                       (const float *)ua, n, a, (const int *)(done + l));
            TIP_LAUNCH("of_check", k_of_check, dim3(1), dim3(1), 0, (const double *)a, tol_l, done + l);
        }
    }
    if (warps_host && !run) {
        for (int l = 0; l < nl; l++) warps_host[l] = num_warp >= 1 ? 1 : 0;
    } else if (warps_host) {
        int h[OF_MAX_LEVELS];
        TIP_HIP(hipMemcpyAsync(h, count, nl * sizeof(int), hipMemcpyDeviceToHost, c.stream));
        TIP_HIP(hipStreamSynchronize(c.stream));
        for (int l = 0; l < nl; l++) warps_host[l] = h[nl - 1 - l];   // coarse to fine, like skimage's solver calls
    }
    return nl;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_optical_flow_tvl1_dev(const void *ref, const void *mov, int dtype, int y, int x, float attachment, float tightness,
                              int num_warp, int num_iter, double tol, float *flow_out, int32_t *warps_per_level, int cap)
{
    if (dtype == OF_F64_AS_U16) return fail(TIP_ERR_ARG, "tip_optical_flow_tvl1: dtype %d (0 f32, 1 f64, 3 u16, 4 u8)", dtype);
    int rc = optical_flow_tvl1_dev(ref, mov, dtype, y, x, attachment, tightness, num_warp, num_iter, tol, flow_out,
                                   warps_per_level, cap);
    return rc < 0 ? rc : TIP_OK;
}

int tip_optical_flow_tvl1(const void *ref, const void *mov, int dtype, int y, int x, float attachment, float tightness,
                          int num_warp, int num_iter, double tol, float *flow_out, int32_t *warps_per_level, int cap)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!ref || !mov || !flow_out || y < 2 || x < 2) return fail(TIP_ERR_ARG, "tip_optical_flow_tvl1: bad arguments");
    if (dtype == OF_F64_AS_U16) return fail(TIP_ERR_ARG, "tip_optical_flow_tvl1: dtype %d (0 f32, 1 f64, 3 u16, 4 u8)", dtype);
    const size_t es = dtype == 1 ? 8 : (dtype == 0 ? 4 : (dtype == 3 ? 2 : 1));
    const size_t bytes = (size_t)y * x * es;
    WsGuard ws;
    char *da = ws.get<char>(bytes), *db = ws.get<char>(bytes);
    float *df = ws.get<float>((size_t)2 * y * x);
    if (!da || !db || !df) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(da, ref, bytes, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemcpyAsync(db, mov, bytes, hipMemcpyHostToDevice, c.stream));
    int rc = optical_flow_tvl1_dev(da, db, dtype, y, x, attachment, tightness, num_warp, num_iter, tol, df, warps_per_level, cap);
    if (rc < 0) return rc;
    TIP_HIP(hipMemcpyAsync(flow_out, df, (size_t)2 * y * x * sizeof(float), hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    return TIP_OK;
}

}  // extern "C"
