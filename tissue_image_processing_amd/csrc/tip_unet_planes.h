// tip_unet_planes.h -- the U-Net's small kernels that read stored split planes back (piece formats: tip_unet_conv.h): MaxPool2D(2), the
// head (Conv2D 1x1 + softmax) and the border pass of a composed decoder level.
#pragma once
#include "tip_unet_conv.h"

namespace tip {

// value of split element e (0..7) of the 16-byte pieces pc[0..NPL)
template <int NPL, bool F16 = false>
__device__ __forceinline__ float split_value(const uint4 *pc, int e)
{
    float v = 0.f;
#pragma unroll
    for (int pl = NPL - 1; pl >= 0; --pl) {     // smallest piece first: the sum is exact either way (<= 24 significant bits)
        const unsigned w = e < 2 ? pc[pl].x : (e < 4 ? pc[pl].y : (e < 6 ? pc[pl].z : pc[pl].w));
        v += uc_piece_value<F16>((e & 1) ? (w >> 16) : (w & 0xffffu));
    }
    return v;
}

// ---- MaxPool2D(2) on split planes: the winner's pieces are copied (the pieces of a value are a function of the value) ---------
template <int NPL, bool F16 = false>
__global__ void __launch_bounds__(256) k_unet_pool2(const uint16_t *__restrict__ in, int H, int W, int C, uint16_t *__restrict__ out)
{
    const int Ho = H / 2, Wo = W / 2, C8 = C / 8;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Ho * Wo * C8) return;
    const int c8 = (int)(i % C8);
    const long op = i / C8;
    const int xo = (int)(op % Wo), yo = (int)(op / Wo);
    const long in_plane = (long)H * W * C, out_plane = (long)Ho * Wo * C;
    uint4 pc[4][NPL];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
            pc[k][pl] = *reinterpret_cast<const uint4 *>(in + pl * in_plane + ((long)(2 * yo + (k >> 1)) * W + 2 * xo + (k & 1)) * C + c8 * 8);
    unsigned res[NPL][4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        int best = 0;
        float bv = split_value<NPL, F16>(pc[0], e);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float v = split_value<NPL, F16>(pc[k], e);
            if (v > bv) { bv = v; best = k; }
        }
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
            const uint4 q = best == 0 ? pc[0][pl] : (best == 1 ? pc[1][pl] : (best == 2 ? pc[2][pl] : pc[3][pl]));
            const unsigned w = e < 2 ? q.x : (e < 4 ? q.y : (e < 6 ? q.z : q.w));
            const unsigned hb = (e & 1) ? (w >> 16) : (w & 0xffffu);
            if (e & 1) res[pl][e >> 1] |= hb << 16; else res[pl][e >> 1] = hb;
        }
    }
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl)
        *reinterpret_cast<uint4 *>(out + pl * out_plane + op * C + c8 * 8) = make_uint4(res[pl][0], res[pl][1], res[pl][2], res[pl][3]);
}

// ---- head: Conv2D(128 -> 2, 1x1) + softmax over the two classes (pl.py:69), float32 out (2, H, W) -------------------------------
// eight lanes per pixel, 16 channels each; logits != 0: the pre-softmax values (the bench's head calibration)
template <int NPL, bool F16 = false>
__global__ void __launch_bounds__(256) k_unet_head(const uint16_t *__restrict__ in, long npix, const float *__restrict__ wgt /* [2][128] */,
                                                   const float *__restrict__ bias, float *__restrict__ out, int logits)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long pix = t >> 3;
    const int part = (int)(t & 7);
    const long plane = npix * 128;
    float z0 = 0.f, z1 = 0.f;
    if (pix < npix) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            uint4 pc[NPL];
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) pc[pl] = *reinterpret_cast<const uint4 *>(in + pl * plane + pix * 128 + part * 16 + g * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = split_value<NPL, F16>(pc, e);
                const int c = part * 16 + g * 8 + e;
                z0 = __builtin_fmaf(v, wgt[c], z0);
                z1 = __builtin_fmaf(v, wgt[128 + c], z1);
            }
        }
    }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) { z0 += __shfl_xor(z0, d, 64); z1 += __shfl_xor(z1, d, 64); }
    if (pix < npix && part == 0) {
        z0 += bias[0]; z1 += bias[1];
        if (logits) { out[pix] = z0; out[npix + pix] = z1; return; }
        uc_softmax2(z0, z1, out, pix, npix + pix);
    }
}

// ---- border pass of a composed decoder level (Conv2DTranspose folded into the next Conv2D) -----------------------------
// The composed launches compute the convolution of the UNCROPPED transposed convolution; the real network crops it to 2N rows and
// columns, so on the last output row / column the term through the virtual row up[2N] = x[N-1] T2 has to go (and comes back once
// at the corner), and the transposed convolution's bias reaches an edge pixel through fewer taps than an interior one.
// k_unet_compose_edge walks ONE edge line of the float32 partial: low-resolution position j of the line owns the output pixels
// 2j (parity 0: taps at j - 1, j) and 2j + 1 (parity 1: taps at j - 1, j, j + 1); part += sum over taps and input channels of
// x[j + d] * wgt[tap] in plain float32 FMAs on the rejoined pieces of x.  A block: EB_J positions x EB_CO output channels, the input
// channels dealt in sixteens to EB_G groups of threads whose sums are added in a fixed order (deterministic).
constexpr int EB_J = 8, EB_CO = 64, EB_G = 8, EB_CH = 16 * EB_G;
struct EdgeParams {
    const uint16_t *x;             // split activations of the low-resolution grid
    long xplane;                   // elements per plane
    int planes, f16;
    float xscale;                  // 1 / activation scale (fp16 pieces)
    int cin, cout, L;              // line length in low-resolution positions
    long x0, xstep;                // element offset of position 0 / from one position to the next
    const float *wgt[5];           // [cin][cout] each: taps (parity, offset) = (0, -1) (0, 0) (1, -1) (1, 0) (1, +1), signs included
    int tapmask;                   // taps that exist (the corner: tap 3 alone)
    float *part;
    long o0, ostep;                // element offset of the line's output pixel 0 / from one output pixel to the next
};
static __global__ void __launch_bounds__(EB_CO * EB_G) k_unet_compose_edge(const EdgeParams p)
{
    __shared__ float xs[EB_J + 2][EB_CH];
    __shared__ float red[EB_G - 1][2 * EB_J][EB_CO];
    const int tid = threadIdx.x, col = tid % EB_CO, g = tid / EB_CO;
    const int j0 = blockIdx.x * EB_J, co = blockIdx.y * EB_CO + col;
    float a[2][EB_J];
#pragma unroll
    for (int jj = 0; jj < EB_J; ++jj) a[0][jj] = a[1][jj] = 0.f;
    for (int c0 = 0; c0 < p.cin; c0 += EB_CH) {
        const int nch = min(EB_CH, p.cin - c0);          // (a multiple of 16: group g's sixteen channels exist or do not)
        __syncthreads();
        for (int i = tid; i < (EB_J + 2) * EB_CH; i += EB_CO * EB_G) {
            const int jj = i / EB_CH, c = i - jj * EB_CH, j = j0 + jj - 1;
            float v = 0.f;
            if (c < nch && j >= 0 && j < p.L) {
                const uint16_t *src = p.x + p.x0 + (long)j * p.xstep + c0 + c;
                for (int pl = p.planes - 1; pl >= 0; --pl)       // smallest piece first; the sum is exact (<= 24 significant bits)
                    v += p.f16 ? uc_piece_value<true>(src[pl * p.xplane]) : uc_piece_value<false>(src[pl * p.xplane]);
                v *= p.xscale;
            }
            xs[jj][c] = v;
        }
        __syncthreads();
        if (g * 16 < nch) {
#pragma unroll
            for (int k8 = 0; k8 < 16; k8 += 8) {
                float w[8][5];          // eight channels' weights on their way before the first is used (the loop is latency-bound otherwise)
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int t = 0; t < 5; ++t)
                        w[u][t] = ((p.tapmask >> t) & 1) ? p.wgt[t][(long)(c0 + g * 16 + k8 + u) * p.cout + co] : 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int k = g * 16 + k8 + u;
#pragma unroll
                    for (int jj = 0; jj < EB_J; ++jj) {
                        const float xm = xs[jj][k], xc = xs[jj + 1][k], xp = xs[jj + 2][k];
                        a[0][jj] = __builtin_fmaf(xc, w[u][1], __builtin_fmaf(xm, w[u][0], a[0][jj]));
                        a[1][jj] = __builtin_fmaf(xp, w[u][4], __builtin_fmaf(xc, w[u][3], __builtin_fmaf(xm, w[u][2], a[1][jj])));
                    }
                }
            }
        }
    }
    if (g > 0) {
#pragma unroll
        for (int jj = 0; jj < EB_J; ++jj) { red[g - 1][2 * jj][col] = a[0][jj]; red[g - 1][2 * jj + 1][col] = a[1][jj]; }
    }
    __syncthreads();
    if (g > 0) return;
#pragma unroll
    for (int jj = 0; jj < EB_J; ++jj)
#pragma unroll
        for (int par = 0; par < 2; ++par) {
            if (j0 + jj >= p.L || !(p.tapmask & (par ? 0x1c : 0x3))) continue;
            float v = a[par][jj];
#pragma unroll
            for (int q = 0; q < EB_G - 1; ++q) v += red[q][2 * jj + par][col];
            p.part[p.o0 + (long)(2 * (j0 + jj) + par) * p.ostep + co] += v;
        }
}

// the transposed convolution's bias through the next convolution's taps: the interior sum sits in that layer's bias vector, an edge
// pixel gets (its own sum - the interior's) from a table [3 rows: top, inside, bottom][3 columns: left, inside, right][cout]
static __global__ void __launch_bounds__(256) k_unet_compose_edge_bias(float *__restrict__ part, int H2, int W2, int cout, const float *__restrict__ tab)
{
    const int c4 = cout / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long npix = 2L * W2 + 2L * (H2 - 2);
    if (i >= npix * c4) return;
    const long e = i / c4;
    const int c = (int)(i - e * c4) * 4;
    int y, x;
    if (e < W2) { y = 0; x = (int)e; }
    else if (e < 2L * W2) { y = H2 - 1; x = (int)(e - W2); }
    else { const long k = e - 2L * W2; y = 1 + (int)(k >> 1); x = (k & 1) ? W2 - 1 : 0; }
    const int type = (y == 0 ? 0 : (y == H2 - 1 ? 2 : 1)) * 3 + (x == 0 ? 0 : (x == W2 - 1 ? 2 : 1));
    float4 *dst = reinterpret_cast<float4 *>(part + ((long)y * W2 + x) * cout + c);
    const float4 t = *reinterpret_cast<const float4 *>(tab + (long)type * cout + c);
    float4 v = *dst;
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    *dst = v;
}

}  // namespace tip
