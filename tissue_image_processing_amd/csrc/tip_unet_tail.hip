// tip_unet_tail.hip -- the post-network tail (pl.py:167-194) as one submission on the library's stream: threshold, the morphology chain
// on bytes in LDS, the watershed.
#include "tip_internal.h"

namespace tip {

// HC_B = 255 * (p > thr)  (pl.py:168), p read with a row pitch (the un-padded view of the network's output)
template <typename T>
__global__ void __launch_bounds__(256) k_tail_threshold(const T *__restrict__ p, long ld, int Y, int X, T thr, double *__restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x < X) out[(long)y * X + x] = p[(long)y * ld + x] > thr ? 255.0 : 0.0;
}

__global__ void __launch_bounds__(256) k_tail_sub(const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] - b[i];
}

// The tail's whole morphology (pl.py:168-193) in ONE kernel.  Every image of the chain is two-valued, so it runs on bytes in LDS:
//   A = p > thr -> B = dilation 5x5 -> closed = erosion 5x5 -> HC = erosion 7x7 -> D = closed - HC -> boundary = dilation 5x5.
// skimage / scipy filter with 'reflect' borders; a symmetric window on a reflect-extended image yields the reflect-extension of
// the filtered image, so the chain of reflect-bordered filters equals the chain on the reflect-extended input: a block loads its
// 64 x 64 tile with a 9-pixel halo (2 + 2 + 3 + 2) through reflected coordinates and runs the separable passes on shrinking
// margins.  As four generic float64 rank-filter launches + a subtraction this was 0.58 ms per 2048^2 frame.
constexpr int TM_T = 64, TM_H = 9, TM_W = TM_T + 2 * TM_H, TM_P = TM_W + 2;
template <typename T>
__global__ void __launch_bounds__(256) k_tail_morph(const T *__restrict__ p, long ld, int Y, int X, T thr, double *__restrict__ hc,
                                                    double *__restrict__ bd)
{
    __shared__ unsigned char s0[TM_W][TM_P], s1[TM_W][TM_P], s2[TM_W][TM_P];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TM_T - TM_H, y0 = blockIdx.y * TM_T - TM_H;
    auto refl = [](int i, int n) {                 // scipy 'reflect' (d c b a | a b c d | d c b a), any overshoot
        const int period = 2 * n;
        i %= period;
        if (i < 0) i += period;
        return i < n ? i : period - 1 - i;
    };
    for (int i = tid; i < TM_W * TM_W; i += 256) {
        const int r = i / TM_W, c = i - r * TM_W;
        s0[r][c] = p[(long)refl(y0 + r, Y) * ld + refl(x0 + c, X)] > thr ? 1 : 0;
    }
    __syncthreads();
    // separable window passes over the largest region whose window fits the array (what they compute from cells outside the valid
    // margin never reaches the interior: the margins add up to the halo)
    auto row_pass = [&](unsigned char (*src)[TM_P], unsigned char (*dst)[TM_P], int rad, bool is_max) {
        const int wc = TM_W - 2 * rad;
        for (int i = tid; i < TM_W * wc; i += 256) {
            const int r = i / wc, c = rad + i - r * wc;
            unsigned v = src[r][c - rad];
            for (int d = -rad + 1; d <= rad; ++d) v = is_max ? (v | src[r][c + d]) : (v & src[r][c + d]);
            dst[r][c] = (unsigned char)v;
        }
        __syncthreads();
    };
    auto col_pass = [&](unsigned char (*src)[TM_P], unsigned char (*dst)[TM_P], int rad, bool is_max) {
        const int hr = TM_W - 2 * rad;
        for (int i = tid; i < hr * TM_W; i += 256) {
            const int r = rad + i / TM_W, c = i % TM_W;
            unsigned v = src[r - rad][c];
            for (int d = -rad + 1; d <= rad; ++d) v = is_max ? (v | src[r + d][c]) : (v & src[r + d][c]);
            dst[r][c] = (unsigned char)v;
        }
        __syncthreads();
    };
    row_pass(s0, s1, 2, true);  col_pass(s1, s0, 2, true);      // B = dilation 5x5            (valid margin 2)
    row_pass(s0, s1, 2, false); col_pass(s1, s2, 2, false);     // closed = erosion 5x5 in s2  (4)
    row_pass(s2, s1, 3, false); col_pass(s1, s0, 3, false);     // HC = erosion 7x7 in s0      (7)
    for (int i = tid; i < TM_W * TM_W; i += 256) {              // D = closed - HC in s1; HC out
        const int r = i / TM_W, c = i - r * TM_W;
        s1[r][c] = s2[r][c] & (s0[r][c] ^ 1);                  // (erosion never exceeds its input: closed - HC is 255 or 0)
        const int y = y0 + r, x = x0 + c;
        if (r >= TM_H && r < TM_H + TM_T && c >= TM_H && c < TM_H + TM_T && y < Y && x < X) hc[(long)y * X + x] = s0[r][c] ? 255.0 : 0.0;
    }
    __syncthreads();
    row_pass(s1, s2, 2, true);  col_pass(s2, s0, 2, true);      // boundary = dilation 5x5 in s0 (9)
    for (int i = tid; i < TM_T * TM_T; i += 256) {
        const int r = TM_H + i / TM_T, c = TM_H + i % TM_T;
        const int y = y0 + r, x = x0 + c;
        if (y < Y && x < X) bd[(long)y * X + x] = s0[r][c] ? 255.0 : 0.0;
    }
}

}  // namespace tip

using namespace tip;

extern "C" {

// pl.py:167-194 on a device-resident class-0 probability map p (y rows of x values, row pitch ld elements; dtype 0 =
// float32, 1 = float64): HC_B = 255 (p > thr) -> 5x5 closing (the reference's 101 iterations are idempotent) -> HC = 7x7
// erosion -> boundary = 5x5 dilation of (closed - HC) -> watershed(boundary, watershed_line=True).  labels (int32) and hc
// (float64) are caller-owned device buffers of y * x elements.  Everything runs on the library's stream in library
// workspaces.  The boundary image is {0, 255} by construction; anything else means a corrupted intermediate and is an
// error, not a slow flood.
int tip_unet_tail_dev(const void *p, int dtype, long ld, int y, int x, double thr, int32_t *labels, double *hc, int32_t *flags_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!p || !labels || !hc || y < 1 || x < 1 || ld < x || (dtype != 0 && dtype != 1)) return fail(TIP_ERR_ARG, "tip_unet_tail_dev: bad arguments");
    const long n = (long)y * x;
    WsGuard ws;
    double *b = ws.get<double>(n);
    if (!b) return TIP_ERR_NOMEM;
    const dim3 mgrid(cdiv(x, TM_T), cdiv(y, TM_T));
    if (tuning().unet_tail_unfused) {        // the same chain as separate launches (tests compare the two)
        double *a = ws.get<double>(n), *d = ws.get<double>(n);
        if (!a || !d) return TIP_ERR_NOMEM;
        if (dtype == 0)
            TIP_LAUNCH("tail_threshold", k_tail_threshold<float>, dim3(cdiv(x, 256), y), dim3(256), 0, (const float *)p, ld, y, x, (float)thr, a);
        else
            TIP_LAUNCH("tail_threshold", k_tail_threshold<double>, dim3(cdiv(x, 256), y), dim3(256), 0, (const double *)p, ld, y, x, thr, a);
        int rc0;
        if ((rc0 = rankfilter2d_dev(a, b, 1, y, x, 5, 5, 0, 1, 1))) return rc0;     // dilation 5x5, reflect
        if ((rc0 = rankfilter2d_dev(b, a, 1, y, x, 5, 5, 0, 1, 0))) return rc0;     // erosion 5x5 -> closed
        if ((rc0 = rankfilter2d_dev(a, hc, 1, y, x, 7, 7, 0, 1, 0))) return rc0;    // HC = erosion 7x7
        TIP_LAUNCH("tail_sub", k_tail_sub, dim3(cdiv(n, 256)), dim3(256), 0, (const double *)a, (const double *)hc, d, n);
        if ((rc0 = rankfilter2d_dev(d, b, 1, y, x, 5, 5, 0, 1, 1))) return rc0;     // boundary = dilation 5x5
    } else if (dtype == 0) {
        TIP_LAUNCH("tail_morph", k_tail_morph<float>, mgrid, dim3(256), 0, (const float *)p, ld, y, x, (float)thr, hc, b);
    } else {
        TIP_LAUNCH("tail_morph", k_tail_morph<double>, mgrid, dim3(256), 0, (const double *)p, ld, y, x, thr, hc, b);
    }
    int rc;
    int32_t flags = 0;
    if ((rc = watershed_dev(b, labels, y, x, 1, &flags))) return rc;
    if (flags_host) *flags_host = flags;
    if (c.last_ws_other != 0)
        return fail(TIP_ERR_HIP, "tip_unet_tail_dev: the boundary image is not two-valued (%ld other values): corrupted intermediate", c.last_ws_other);
    return TIP_OK;
}

}  // extern "C"
