// tip_corr.h -- exact scipy-order separable correlation kernels (device templates) and the one tap sum they all share.
#pragma once
#include "tip_internal.h"
#include <type_traits>

namespace tip {

template <typename T>
struct LoadPlain {
    const T *p;
    long sz, sy;  // strides of z and y in elements (x stride 1)
    __device__ __forceinline__ double operator()(int z, int y, int x) const { return (double)p[z * sz + y * sy + x]; }
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The arithmetic contract of every exact Gaussian pass (scipy/ndimage/src/ni_filters.c NI_Correlate1D, symmetric branch;
// called through gaussian_filter at bim.py:389), spelled here and nowhere else:
//     tmp  = x[c] * w[r]
//     tmp += (x[c-d] + x[c+d]) * w[r-d]      for d = r, r-1, ..., 1      (all in double, no FMA contraction)
//     out  = (T) tmp
// with mode='nearest' (index clamp).  The whole library is compiled with -ffp-contract=off so that the
// multiply and the add round separately, as scipy's x86-64 builds do.
// at(j): window sample j = 0 .. 2r as double (centre at r; the clamp and the cast to double are the accessor's);
// w: anything indexable that yields double.  Compile-time radius: fully unrolled, so ring indices inside at() fold.
template <int R, typename At, typename W>
__device__ __forceinline__ double tap_sum(At at, const W &w)
{
    double tmp = at(R) * w[R];
#pragma unroll
    for (int d = R; d >= 1; --d) tmp += (at(R - d) + at(R + d)) * w[R - d];
    return tmp;
}
template <typename At, typename W>
__device__ __forceinline__ double tap_sum(int r, At at, const W &w)
{
    double tmp = at(r) * w[r];
    for (int d = r; d >= 1; --d) tmp += (at(r - d) + at(r + d)) * w[r - d];
    return tmp;
}

struct TapsDev {   // taps in device memory: any odd, symmetric count, for radii beyond the table of a Taps
    const double *w;
    int n;
};

// run-time axis -> compile-time axis: f(std::integral_constant<int, A>) for A = axis; FIRST = 1 for in-plane-only kernels
template <int FIRST = 0, typename F>
static inline int with_axis(int axis, F &&f)
{
    if constexpr (FIRST == 0)
        if (axis == 0) return f(std::integral_constant<int, 0>{});
    if (axis == 1) return f(std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, 2>{});
}

// Generic kernel: one thread per output element, taps (a Taps by value or a TapsDev) read through the cache hierarchy.
// AXIS: 0 = z, 1 = y, 2 = x of a (Z,Y,X) volume.  Good for short kernels (<= ~25 taps).
template <typename T, int AXIS, typename Load, typename TapSrc = Taps>
__global__ void __launch_bounds__(256) k_corr_generic(Load in, T *__restrict__ out, int Z, int Y, int X, TapSrc taps)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int z = blockIdx.z;
    if (x >= X) return;
    const int r = taps.n >> 1;
    const int len = AXIS == 0 ? Z : (AXIS == 1 ? Y : X);
    const int c = AXIS == 0 ? z : (AXIS == 1 ? y : x);
    auto at = [&](int j) -> double {
        const int i = clampi(c - r + j, 0, len - 1);
        return AXIS == 0 ? in(i, y, x) : (AXIS == 1 ? in(z, i, x) : in(z, y, i));
    };
    out[((long)z * Y + y) * X + x] = (T)tap_sum(r, at, taps.w);
}

// Stage a (positions x 64 lines) float tile into LDS with 'nearest' clamping.  A block owns its CU's LDS alone, so
// nothing else hides the HBM latency of this phase: every wave keeps 8 (AXIS 1) or 16 (AXIS 2) loads in flight
// before the first LDS write.  first = plane coordinate of tile position 0 along the filter axis.
template <int AXIS, int NW>
__device__ __forceinline__ void stage_tile(float *tile, const float *__restrict__ src, int npos, int first, int l0, int Y, int X,
                                           int lane, int wave)
{
    constexpr int LS = AXIS == 1 ? 64 : 65;
    if (AXIS == 1) {
        constexpr int UL = 8;
        const int xx = min(l0 + lane, X - 1);
        for (int pb = wave; pb < npos; pb += NW * UL) {
            float v[UL];
#pragma unroll
            for (int u = 0; u < UL; ++u) v[u] = src[(long)clampi(first + pb + u * NW, 0, Y - 1) * X + xx];
#pragma unroll
            for (int u = 0; u < UL; ++u)
                if (pb + u * NW < npos) tile[(pb + u * NW) * LS + lane] = v[u];
        }
    } else {
        // npos <= 256 + 2*127 < 512: eight 64-wide chunks cover a line; two lines per trip
        for (int l = wave; l < 64; l += 2 * NW) {
            float v[2][8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int yy = min(l0 + l + h * NW, Y - 1);
#pragma unroll
                for (int u = 0; u < 8; ++u) v[h][u] = src[(long)yy * X + clampi(first + lane + 64 * u, 0, X - 1)];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (lane + 64 * u < npos && l + h * NW < 64) tile[(lane + 64 * u) * LS + l + h * NW] = v[h][u];
        }
    }
}

// Long-kernel variant (radius up to 127, float32 volumes): every lane owns one line and slides along
// the filter axis with register-resident left/right windows of R outputs, the line segment (tile +
// 2*radius halo) staged once in LDS as float32.
//   AXIS==1: lanes run along x (coalesced loads/stores), positions along y: LDS[pos][64]
//   AXIS==2: lanes run along y, positions along x: loaded coalesced along x and written transposed
//            into LDS[pos][65] (stride 65 keeps both the transposed write and the lane-major read
//            conflict-free)
// Block = 256 threads = 4 waves; the 4 waves split the tile's TO outputs per line.
template <int AXIS, int TO, int R>
__global__ void __launch_bounds__(256) k_corr_long_f32(const float *__restrict__ in, float *__restrict__ out,
                                                       int Z, int Y, int X, Taps taps)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];
    constexpr int LS = AXIS == 1 ? 64 : 65;
    const int r = taps.n >> 1;
    const int npos = TO + 2 * r;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int z = blockIdx.z;
    const int len = AXIS == 1 ? Y : X;      // filter-axis length
    const int nlines = AXIS == 1 ? X : Y;   // line-axis length
    const int p0 = blockIdx.y * TO;         // first output position of this tile
    const int l0 = blockIdx.x * 64;         // first line of this tile
    const float *src = in + (long)z * Y * X;
    float *dst = out + (long)z * Y * X;

    stage_tile<AXIS, 4>(tile, src, npos, p0 - r, l0, Y, X, lane, wave);
    __syncthreads();

    const int line = l0 + lane;
    constexpr int PER_WAVE = TO / 4;
    for (int g = 0; g < PER_WAVE / R; ++g) {
        const int o0 = wave * PER_WAVE + g * R;  // first output (tile-relative) of this group
        if (p0 + o0 >= len) break;               // wave-uniform
        const float *ctr = tile + (r + o0) * LS + lane;
        double acc[R], L[R], Rr[R];
        const double wc = taps.w[r];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            acc[i] = (double)ctr[i * LS] * wc;
            L[i] = (double)ctr[(i - r) * LS];
            Rr[i] = (double)ctr[(i + r) * LS];
        }
#pragma unroll 8
        for (int d = r; d >= 1; --d) {   // tap_sum's contract for R outputs at once, the window shifts interleaved with the sum
            const double w = taps.w[r - d];
#pragma unroll
            for (int i = 0; i < R; ++i) acc[i] += (L[i] + Rr[i]) * w;
            // slide: left window moves right by one, right window moves left by one
#pragma unroll
            for (int i = 0; i < R - 1; ++i) L[i] = L[i + 1];
            L[R - 1] = (double)ctr[(R - 1 - (d - 1)) * LS];
#pragma unroll
            for (int i = R - 1; i > 0; --i) Rr[i] = Rr[i - 1];
            Rr[0] = (double)ctr[(d - 1) * LS];
        }
        if (line < nlines) {
            if (AXIS == 1) {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int yy = p0 + o0 + i;
                    if (yy < Y) dst[(long)yy * X + line] = (float)acc[i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int xx = p0 + o0 + i;
                    if (xx < X) dst[(long)line * X + xx] = (float)acc[i];
                }
            }
        }
    }
}

}  // namespace tip
