// tip_project_binned.h -- the bin_size > 1 kernels of the projection (sp.py:39-65): skimage's block_reduce and resize and
// numpy's summation order, reproduced to the bit.  tip_project.hip's binned stage launches them.
#pragma once
#include "tip_internal.h"

namespace tip {

// build_manifold with bin_size > 1 (sp.py:56-65): the (Yb, Xb) plane map of the binned score goes back to the frame through
// skimage.transform.resize(order 1, mode 'reflect') -- for 2-D arrays the bilinear warp of _warps_cy: source coordinate
// a * i + b (a = n_in / n_out, b = a / 2 - 1 / 2) evaluated in float32, corners floor / ceil with numpy 'reflect' (mirror
// without the edge: index -1 -> 1), top = (1 - dc) v00 + dc v01, bottom likewise, (1 - dr) top + dr bottom in double, float32
// result -- and np.round (half to even).  The float result agrees with skimage's to ~1e-6 (upstream's affine matrix comes out
// of a least-squares estimate, LAPACK-dependent in the last bit); the rounded maps equal the reference's on every golden,
// exact .5 ties included.  The atoh map is clip(plane + shift, 0, Z) BEFORE the resize, as upstream.
__device__ __forceinline__ int mirror_index(int n, int c)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    c = (c < 0 ? -c : c) % p;
    return c > n - 1 ? p - c : c;
}
__global__ void __launch_bounds__(256) k_resize_round_zmaps(const int *__restrict__ bz, int Yb, int Xb, int Y, int X, int Z, int atoh_shift,
                                                            int32_t *__restrict__ zsel, int32_t *__restrict__ zsel_atoh,
                                                            int64_t *__restrict__ zmap, int *__restrict__ err)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= X) return;
    const double sy = (double)Yb / Y, sx = (double)Xb / X;
    const float ar = (float)sy, br = (float)(0.5 * sy - 0.5), ac = (float)sx, bc = (float)(0.5 * sx - 0.5);
    const float fr = ar * (float)y + br, fc = ac * (float)x + bc;
    const int r0 = (int)floorf(fr), c0 = (int)floorf(fc), r1 = (int)ceilf(fr), c1 = (int)ceilf(fc);
    const double dr = (double)(fr - (float)r0), dc = (double)(fc - (float)c0);
    const int y0 = mirror_index(Yb, r0), y1 = mirror_index(Yb, r1), x0 = mirror_index(Xb, c0), x1 = mirror_index(Xb, c1);
    int res[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        auto at = [&](int yy, int xx) -> double {
            int v = bz[(long)yy * Xb + xx];
            if (k == 1 && atoh_shift != 0) { v += atoh_shift; v = v < 0 ? 0 : (v > Z ? Z : v); }
            return (double)v;
        };
        const double top = (1.0 - dc) * at(y0, x0) + dc * at(y0, x1);
        const double bot = (1.0 - dc) * at(y1, x0) + dc * at(y1, x1);
        res[k] = (int)rintf((float)((1.0 - dr) * top + dr * bot));      // np.round: half to even (default rounding mode)
    }
    const long p = (long)y * X + x;
    if (zmap) zmap[p] = res[0];
    if (res[0] >= Z || res[1] >= Z) atomicOr(err, 1);
    zsel[p] = res[0] >= Z ? Z - 1 : res[0];
    zsel_atoh[p] = res[1] >= Z ? Z - 1 : res[1];
}

// ---- P4': bin_size > 1 (sp.py:39-65) -------------------------------------------------------------------------------
// skimage.measure.block_reduce(vol, (1, b, b), np.mean / np.var) in float32 with numpy's summation order: every row of
// a block (b contiguous samples, zeros beyond the frame) goes through numpy's pairwise_sum -- a running sum below 8
// elements, else eight running partial sums combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus the tail -- and the row
// sums are added up one after the other; mean = sum / float32(b*b); var = the same reduction of (x - mean)^2.
__device__ __forceinline__ float pw_row_sum(const float *__restrict__ row, int b, int valid, float mean, bool sq)
{
    auto at = [&](int i) -> float {
        const float v = i < valid ? row[i] : 0.f;
        if (!sq) return v;
        const float d = v - mean;
        return d * d;
    };
    if (b < 8) {
        float res = at(0);
        for (int i = 1; i < b; ++i) res += at(i);
        return res;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = at(j);
    int i = 8;
    for (; i < b - (b % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += at(i + j);
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < b; ++i) res += at(i);
    return res;
}

template <bool VAR>
__global__ void __launch_bounds__(256) k_block_reduce(const float *__restrict__ vol, float *__restrict__ out, int Z, int Y, int X,
                                                      int b, int Yb, int Xb)
{
    const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (long)Z * Yb * Xb) return;
    const int xb = (int)(o % Xb), yb = (int)((o / Xb) % Yb), z = (int)(o / ((long)Xb * Yb));
    const int x0 = xb * b, y0 = yb * b;
    const int valid = min(b, X - x0);
    const float *base = vol + ((long)z * Y + y0) * X + x0;
    const float cnt = (float)(b * b);
    float acc = 0.f;
    for (int r = 0; r < b; ++r) {
        const float row = pw_row_sum(base + (long)r * X, b, y0 + r < Y ? valid : 0, 0.f, false);
        acc = r == 0 ? row : acc + row;
    }
    const float mean = acc / cnt;
    if (!VAR) { out[o] = mean; return; }
    for (int r = 0; r < b; ++r) {
        const float row = pw_row_sum(base + (long)r * X, b, y0 + r < Y ? valid : 0, mean, true);
        acc = r == 0 ? row : acc + row;
    }
    out[o] = acc / cnt;
}

__global__ void __launch_bounds__(256) k_mul_f32(float *__restrict__ a, const float *__restrict__ b, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = a[i] * b[i];
}

// skimage.transform.resize(score, (Z, Y, X)) (order 1, mode 'reflect' -> scipy map_coordinates 'mirror'; the z factor is
// 1) fused with the first-maximum argmax over z.  One axis: coordinate f * (i + 0.5) - 0.5 in float64 with f = n_in /
// n_out, mirrored at both ends, weights (1 - t, 1 - (1 - t)); scipy adds the four corner terms (v * wy) * wx in float64 in
// the order (y0,x0), (y0,x1), (y1,x0), (y1,x1) and rounds to float32.
struct LinTap { int i0, i1; double w0, w1; };
__device__ __forceinline__ LinTap lin_tap(int i, int n_in, int n_out)
{
    LinTap t;
    if (n_in <= 1) { t.i0 = 0; t.i1 = 0; t.w0 = 1.0; t.w1 = 0.0; return t; }
    const double f = (double)n_in / (double)n_out;
    double c = f * ((double)i + 0.5) - 0.5;
    if (c < 0.0) c = -c;
    const double fl = floor(c);
    t.i0 = (int)fl;
    t.i1 = t.i0 + 1;
    if (t.i1 >= n_in) t.i1 = 2 * n_in - 2 - t.i1;
    t.w0 = 1.0 - (c - fl);
    t.w1 = 1.0 - t.w0;
    return t;
}

__global__ void __launch_bounds__(256) k_resize_argmax(const float *__restrict__ binned, int Z, int Yb, int Xb, int Y, int X,
                                                       int *__restrict__ best_z)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= X) return;
    const LinTap ty = lin_tap(y, Yb, Y), tx = lin_tap(x, Xb, X);
    float best = 0.f;
    int bi = 0;
    for (int z = 0; z < Z; ++z) {
        const float *pl = binned + (long)z * Yb * Xb;
        const double v00 = pl[(long)ty.i0 * Xb + tx.i0], v01 = pl[(long)ty.i0 * Xb + tx.i1];
        const double v10 = pl[(long)ty.i1 * Xb + tx.i0], v11 = pl[(long)ty.i1 * Xb + tx.i1];
        double t = (v00 * ty.w0) * tx.w0;
        t += (v01 * ty.w0) * tx.w1;
        t += (v10 * ty.w1) * tx.w0;
        t += (v11 * ty.w1) * tx.w1;
        const float s = (float)t;
        if (z == 0 || s > best) { best = s; bi = z; }
    }
    best_z[(long)y * X + x] = bi;
}

}  // namespace tip
