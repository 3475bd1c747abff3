// tip_unet.hip -- epilogue of the U-Net's convolutions (pl.py:31-37: Conv2D + bias -> ReLU -> BatchNormalization at
// inference = per-channel scale and shift), fused into ONE in-place pass over the NHWC activation.
//
// The convolutions themselves stay with PyTorch-ROCm / MIOpen (north_star: PyTorch only for the U-Net's conv path).  Left
// to torch, the epilogue is four full passes over activations of up to 2.1 GB (bias add, relu, multiply, add): 14 % of the
// network's time at 2048^2.  Same float32 operations in the same order (the library is built with -ffp-contract=off, so
// the multiply and the add round separately like torch's two kernels): bit-identical, one read + one write instead of four.
// Runs on the stream the caller names (torch's current stream), so no cross-stream synchronisation is needed.
#include "tip_internal.h"
#include "tip_unet_conv.h"
#include <algorithm>
#include <atomic>

namespace tip {

__global__ void __launch_bounds__(256) k_bias_relu_affine_f32(float *__restrict__ x, const float *__restrict__ bias,
                                                              const float *__restrict__ scale, const float *__restrict__ shift,
                                                              long n4, int C)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<float4 *>(x)[i];
    const int c = (int)((i * 4) % C);                       // C % 4 == 0: the four lanes are channels c .. c+3
    const float4 b = *reinterpret_cast<const float4 *>(bias + c);
    const float4 s = *reinterpret_cast<const float4 *>(scale + c);
    const float4 t = *reinterpret_cast<const float4 *>(shift + c);
    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
    v.x = v.x * s.x + t.x; v.y = v.y * s.y + t.y; v.z = v.z * s.z + t.z; v.w = v.w * s.w + t.w;
    reinterpret_cast<float4 *>(x)[i] = v;
}

// ---- the post-network tail (pl.py:167-194) as one submission on the library's stream ------------------------------------
int rankfilter2d_dev(const void *in, void *out, int dtype, int Y, int X, int ky, int kx, int fp, int border, int is_max);   // tip_label.hip
int watershed_dev(const double *img, int32_t *labels, int Y, int X, int wsl, int32_t *flags_host);                          // tip_watershed.hip

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


// ---- U1: prepare_image (pl.py:21-29, 90-122) on a device-resident (C, A, B) float64 image ----------------------------------------
// normalize_channel clips every channel to its [1st, 99th] percentile and scales to [0, 1]; prepare_image transposes to (B, A) and
// pads in front to the network's extents.  The percentiles are np.percentile's: order statistics k, k + 1 of the channel plus
// numpy's lerp.  They come from a most-significant-digit radix select over sortable 64-bit keys -- no sort -- and never leave the
// device: the normalise / transpose / pad pass reads them from memory.
//
// The select reads the image five times (digits of 13, 13, 13, 13 and 12 bits), both ranks of every channel in one launch.  A pass
// is a fixed number of workgroups (a small multiple of the CU count) that stride over the plane with 16-byte loads and count into
// histograms in LDS -- one histogram for both ranks as long as they share every digit picked so far, as in the first pass, where
// every key counts -- so a pass adds at most workgroups x touched bins to the histograms in memory.  The workgroup of a channel
// that finishes last (a counter in PrepState, bumped by one wave behind its adds and a __threadfence(); nobody waits for anybody)
// picks the digit of both ranks with a scan, clears the histograms and re-arms the counter.  The smallest key above each selected one (order statistic k + 1 where the selected key occurs once) costs
// no pass of its own: it shares either all but the last digit with the selected key -- then the last histogram holds it -- or
// not, and the last pass keeps the minimum of those keys, one atomicMin per workgroup and rank at the most.
constexpr int PREP_MAXC = 8;
constexpr int PREP_BITS = 13, PREP_BINS = 1 << PREP_BITS;      // the widest digit: two ranks x 8192 bins x 4 B = 64 KB of LDS
constexpr int PREP_T = 512, PREP_U = 4, PREP_W = PREP_T / 64;  // threads of a pass, 16-byte loads in flight per thread, waves
constexpr int PREP_PER = PREP_BINS / PREP_T;                   // bins per thread of the pick's scan
struct PrepState {                      // per (channel, which percentile): [c][0] = the 1st, [c][1] = the 99th
    unsigned int hist[PREP_MAXC][2][PREP_BINS];
    unsigned int done[PREP_MAXC];       // workgroups of the running pass that have added their counts
    unsigned long long prefix[PREP_MAXC][2], above[PREP_MAXC][2];
    long long rank[PREP_MAXC][2], room[PREP_MAXC][2];
    double per[PREP_MAXC][2], clipv[PREP_MAXC][2];      // percentile values; the values written over the clipped pixels
};

__device__ __forceinline__ unsigned long long prep_enc(double d)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(d + 0.0);   // (-0.0 sorts with +0.0, like numpy's <)
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double prep_dec(unsigned long long e)
{
    unsigned long long b = (e >> 63) ? (e & 0x7fffffffffffffffULL) : ~e;
    return __longlong_as_double((long long)b);
}

// grid (PREP_BINS * 2 / PREP_T, C)
__global__ void __launch_bounds__(PREP_T) k_prep_reset(PrepState *st, long long r1, long long r99)
{
    const int c = blockIdx.y, t = threadIdx.x;
    (&st->hist[c][0][0])[blockIdx.x * PREP_T + t] = 0;
    if (blockIdx.x == 0 && t < 2) {
        st->prefix[c][t] = 0; st->above[c][t] = ~0ULL; st->room[c][t] = 0;
        st->rank[c][t] = t ? r99 : r1;
    }
    if (blockIdx.x == 0 && t == 2) st->done[c] = 0;
}

// One key per lane of a whole wave into a histogram in LDS (m: this lane counts).  Projection values share their leading digits:
// when every counting lane has the first one's bin, one lane adds their number.
__device__ __forceinline__ void prep_count(unsigned int *h, int bin, bool m)
{
    const unsigned long long act = __ballot(m);
    if (act == 0) return;
    const int first = __ffsll(act) - 1;
    const int fb = __builtin_amdgcn_readlane(bin, first);
    if (__ballot(m && bin == fb) == act) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[fb], (unsigned int)__popcll(act));
    } else if (m) {
        atomicAdd(&h[bin], 1u);
    }
}

// One digit (bits `shift` .. `shift + bits - 1` of the key) of both selects of channel blockIdx.y; the plane is dense (n consecutive
// doubles from img + c * cstride).  MODE 0: the first digit (nothing selected yet, one histogram), 1: a middle one, 2: the last
// (shift == 0; also the smallest key above each selected one, and `room` = how many more copies of the selected key follow, so
// that rank + 1 can be answered).  The pick: prefix gets the digit, rank becomes the rank inside the bin.
template <int MODE>
__global__ void __launch_bounds__(PREP_T) k_prep_digit(const double *__restrict__ img, long cstride, long n, PrepState *st, int shift, int bits)
{
    constexpr int NH = MODE == 0 ? 1 : 2;
    __shared__ unsigned int sh[NH][PREP_BINS];
    __shared__ unsigned long long s_min[2][PREP_W];
    __shared__ long long s_wsum[2][PREP_W], s_cum[2];
    __shared__ int s_last, s_pick[2], s_nb[2];
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < NH * PREP_BINS; i += PREP_T) (&sh[0][0])[i] = 0;
    __syncthreads();
    const int up = shift + bits;
    const unsigned long long t0 = MODE == 0 ? 0 : st->prefix[c][0] >> up, t1 = MODE == 0 ? 0 : st->prefix[c][1] >> up;
    const unsigned int mask = (1u << bits) - 1u;
    const bool one = MODE == 0 || t0 == t1;      // both ranks still inside one bin of every digit so far: one histogram serves both
    const int nbins = one ? PREP_BINS : 2 * PREP_BINS;
    unsigned long long a0 = ~0ULL, a1 = ~0ULL;
    auto visit = [&](unsigned long long key, bool ok) {          // (called by whole waves)
        const int bin = (int)((unsigned int)(key >> shift) & mask);
        if (MODE == 0) {
            prep_count(sh[0], bin, ok);
        } else {
            const unsigned long long top = key >> up;
            prep_count(sh[0], bin, ok && top == t0);
            if (!one) prep_count(sh[NH - 1], bin, ok && top == t1);
            if (MODE == 2) {
                if (ok && top > t0 && key < a0) a0 = key;
                if (ok && top > t1 && key < a1) a1 = key;
            }
        }
    };
    const double *src = img + (long)c * cstride;
    const long head = min(n, (long)((reinterpret_cast<uintptr_t>(src) >> 3) & 1));     // doubles in front of the first 16-byte boundary
    const long npairs = (n - head) >> 1;
    const double2 *src2 = reinterpret_cast<const double2 *>(src + head);
    if (blockIdx.x == 0 && wave == 0) {                          // the doubles outside the pairs: the first and the last one
        const long i = lane == 0 ? (head ? 0 : -1) : (lane == 1 && ((n - head) & 1) ? n - 1 : -1);
        visit(prep_enc(i >= 0 ? src[i] : 0.0), i >= 0);
    }
    const long stripe = (long)gridDim.x * PREP_T;
    for (long base = (long)blockIdx.x * PREP_T; base < npairs; base += stripe * PREP_U) {
        double2 v[PREP_U];
        bool ok[PREP_U];
#pragma unroll
        for (int u = 0; u < PREP_U; ++u) {
            const long p = base + u * stripe + tid;
            ok[u] = p < npairs;
            v[u] = src2[ok[u] ? p : npairs - 1];          // (no branch around a load: the PREP_U loads are in flight together)
        }
#pragma unroll
        for (int u = 0; u < PREP_U; ++u) {
            visit(prep_enc(v[u].x), ok[u]);
            visit(prep_enc(v[u].y), ok[u]);
        }
    }
    if (MODE == 2) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o0 = __shfl_xor(a0, d, 64), o1 = __shfl_xor(a1, d, 64);
            a0 = o0 < a0 ? o0 : a0;
            a1 = o1 < a1 ? o1 : a1;
        }
        if (lane == 0) { s_min[0][wave] = a0; s_min[1][wave] = a1; }
    }
    __syncthreads();
    unsigned int *gh = &st->hist[c][0][0];
    // One wave adds the workgroup's counts to memory, fences ONCE behind its own adds and counts the workgroup in (a fence per
    // wave is the dearest thing in this kernel: every one walks the L2).  The workgroup whose count arrives last picks.
    if (wave == 0) {
        for (int i = lane; i < nbins; i += 64) {
            const unsigned int v = (&sh[0][0])[i];
            if (v) atomicAdd(&gh[i], v);
        }
        if (MODE == 2 && lane < 2) {     // at most one atomic per workgroup and rank, and none once a smaller key is known
            unsigned long long a = ~0ULL;
            for (int k = 0; k < PREP_W; ++k) a = s_min[lane][k] < a ? s_min[lane][k] : a;
            if (a != ~0ULL && a < __hip_atomic_load(&st->above[c][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&st->above[c][lane], a);
        }
        __threadfence();
        if (lane == 0) s_last = atomicAdd(&st->done[c], 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // (behind the counter's answer: every workgroup's adds are visible)
    // read and clear (the next pass adds behind the end of this kernel); all loads of a thread are in flight together
    for (int i0 = 0; i0 < nbins; i0 += PREP_BINS) {
        unsigned int v[PREP_PER];
#pragma unroll
        for (int k = 0; k < PREP_PER; ++k) v[k] = __hip_atomic_load(&gh[i0 + k * PREP_T + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < PREP_PER; ++k) {
            (&sh[0][0])[i0 + k * PREP_T + tid] = v[k];
            gh[i0 + k * PREP_T + tid] = 0;
        }
    }
    if (tid < 2) { s_pick[tid] = (int)mask; s_cum[tid] = 0; s_nb[tid] = PREP_BINS; }
    __syncthreads();
    // both ranks side by side: every thread sums PREP_PER bins, a scan over the waves and then over the wave sums finds the thread
    // whose bins hold the rank
    const unsigned int *h[2] = {sh[0], sh[one ? 0 : 1]};
    long long r[2], sum[2], incl[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        r[w] = st->rank[c][w];
        sum[w] = 0;
#pragma unroll
        for (int k = 0; k < PREP_PER; ++k) sum[w] += h[w][tid * PREP_PER + k];
        incl[w] = sum[w];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(incl[w], d, 64);
            if (lane >= d) incl[w] += o;
        }
        if (lane == 63) s_wsum[w][wave] = incl[w];
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        long long cum = incl[w] - sum[w];
        for (int k = 0; k < wave; ++k) cum += s_wsum[w][k];
        if (cum <= r[w] && r[w] < cum + sum[w]) {                // (one thread)
            int b = tid * PREP_PER;
            while (cum + (long long)h[w][b] <= r[w]) cum += h[w][b++];
            s_pick[w] = b; s_cum[w] = cum;
        }
    }
    __syncthreads();
    if (MODE == 2) {                                             // the next bin in use: the smallest key above that shares the leading digits
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int pick = s_pick[w];
            int nb = PREP_BINS;
#pragma unroll
            for (int k = PREP_PER - 1; k >= 0; --k) {
                const int b = tid * PREP_PER + k;
                if (b > pick && h[w][b]) nb = b;
            }
            if (nb < PREP_BINS) atomicMin(&s_nb[w], nb);
        }
        __syncthreads();
    }
    if (tid < 2) {
        const int w = tid, pick = s_pick[w];
        const long long in_bin = r[w] - s_cum[w];
        const unsigned long long pre = st->prefix[c][w] | ((unsigned long long)pick << shift);
        st->prefix[c][w] = pre;
        st->rank[c][w] = in_bin;
        if (MODE == 2) {
            st->room[c][w] = (long long)h[w][pick] - in_bin - 1;
            const unsigned long long far = atomicMin(&st->above[c][w], ~0ULL);          // (what every workgroup's minimum left there)
            st->above[c][w] = s_nb[w] < PREP_BINS ? ((pre & ~(unsigned long long)mask) | (unsigned long long)s_nb[w]) : far;
        }
    }
    if (tid == 0) atomicExch(&st->done[c], 0u);
}

// np.percentile's 'linear' lerp (numpy/lib/function_base.py _lerp: lo + diff * g, and hi - diff * (1 - g) from g >= 0.5) and the
// values normalize_channel writes over the clipped pixels, which take the INPUT's dtype (pl.py:26-27 assign into a copy of the
// image): kind 0 = float64 (as is), 1 = float32 (rounded), 2 = integer (truncated)
__global__ void __launch_bounds__(64) k_prep_finish(PrepState *st, int C, double g1, double g99, int kind)
{
    const int t = threadIdx.x;
    if (t >= C * 2) return;
    const int c = t >> 1, w = t & 1;
    const double lo = prep_dec(st->prefix[c][w]);
    const double hi = st->room[c][w] > 0 ? lo : (st->above[c][w] == ~0ULL ? lo : prep_dec(st->above[c][w]));
    const double g = w ? g99 : g1;
    const double diff = hi - lo;
    double res = lo + diff * g;
    if (g >= 0.5) res = hi - diff * (1.0 - g);
    st->per[c][w] = res;
    st->clipv[c][w] = kind == 2 ? trunc(res) : (kind == 1 ? (double)(float)res : res);
}

// out[c][pb + b][pa + a] = normalised in[c][a][b]; A_CONTIG: the input's a index has unit stride (threads run along a on both
// sides), else its b index has (a 32 x 32 tile turns through LDS)
template <bool A_CONTIG>
__global__ void __launch_bounds__(256) k_prep_normalize(const double *__restrict__ img, long cstride, long sa, long sb, int A, int B,
                                                        const PrepState *__restrict__ st, int single, float *__restrict__ out, int Ap,
                                                        int Bp, int pa, int pb)
{
    __shared__ float tile[32][33];
    const int c = blockIdx.z, a0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const double per1 = st->per[c][0], per99 = st->per[c][1], lo = st->clipv[c][0], hi = st->clipv[c][1];
    const double den = per99 - per1;
    const float per1f = (float)per1, denf = (float)den;
    const double *src = img + (long)c * cstride;
    float *dst = out + (long)c * Ap * Bp;
    auto norm = [&](double v) -> float {
        double cl = v > per99 ? hi : v;
        cl = v < per1 ? lo : cl;
        if (single) return ((float)cl - per1f) / denf;       // numpy 1.x: float32 array (op) float64 scalar stays float32
        return (float)((cl - per1) / den);
    };
    if (A_CONTIG) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = a0 + tx, b = b0 + ty + k * 8;
            if (a < A && b < B) dst[(long)(pb + b) * Ap + pa + a] = norm(src[(long)a * sa + (long)b * sb]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = a0 + ty + k * 8, b = b0 + tx;
            if (a < A && b < B) tile[ty + k * 8][tx] = norm(src[(long)a * sa + (long)b * sb]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = a0 + tx, b = b0 + ty + k * 8;
            if (a < A && b < B) dst[(long)(pb + b) * Ap + pa + a] = tile[tx][ty + k * 8];
        }
    }
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

// x: n float32 values of a channels-last (NHWC-contiguous) activation with C channels, updated in place:
// x = relu(x + bias[c]) * scale[c] + shift[c].  `stream`: the hipStream_t to launch on, taken as is -- 0 is HIP's null
// stream, which is what torch.cuda.current_stream() is unless the caller changed it.
int tip_bias_relu_affine_f32_dev(float *x, const float *bias, const float *scale, const float *shift, long n, int c, void *stream)
{
    Ctx &cx = ctx();
    if (!cx.stream) return TIP_ERR_HIP;
    if (!x || !bias || !scale || !shift || n < 0 || c < 4 || (c & 3) || (n % c)) return fail(TIP_ERR_ARG, "bias_relu_affine: bad arguments");
    if (n == 0) return TIP_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bias_relu_affine_f32, dim3(cdiv(n / 4, 256)), dim3(256), 0, s, x, bias, scale, shift, n / 4, c);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TIP_ERR_HIP, "launch bias_relu_affine: %s", hipGetErrorString(e));
    return TIP_OK;
}

// Which device does this runtime think `p` lives on?  >= 0: the ordinal; negative: `p` is not a device pointer THIS copy of
// the HIP runtime knows.  A caller that hands over torch pointers and torch's stream (tip_bias_relu_affine_f32_dev,
// tip_unet_tail_dev) checks once that torch and this library share one runtime: PyTorch wheels bundle their own
// libamdhip64, and two loaded runtimes do not know each other's allocations or stream handles.
int tip_pointer_device(const void *p)
{
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return TIP_ERR_ARG; }
    if (a.type != hipMemoryTypeDevice) return TIP_ERR_ARG;
    return a.device;
}

// Ordering edges between the calling thread's library stream and a foreign HIP stream (torch's current stream).  Neither
// blocks the host.  tip_wait_stream: work submitted to the library AFTER the call starts after everything queued on
// `stream` BEFORE the call -- call it after allocating (from torch's caching allocator) every buffer the library is going
// to write: the allocator hands out blocks whose previous owner's kernels may still be queued on that stream.
int tip_wait_stream(void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!c.edge_event) TIP_HIP(hipEventCreateWithFlags(&c.edge_event, hipEventDisableTiming));
    TIP_HIP(hipEventRecord(c.edge_event, (hipStream_t)stream));
    TIP_HIP(hipStreamWaitEvent(c.stream, c.edge_event, 0));
    return TIP_OK;
}

// ... and the other direction: `stream` waits for everything submitted to the library so far.
int tip_stream_wait_tip(void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!c.edge_event) TIP_HIP(hipEventCreateWithFlags(&c.edge_event, hipEventDisableTiming));
    TIP_HIP(hipEventRecord(c.edge_event, c.stream));
    TIP_HIP(hipStreamWaitEvent((hipStream_t)stream, c.edge_event, 0));
    return TIP_OK;
}

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

// ---- the network's layers on split bf16 planes (tip_unet_conv.h).  All of them launch on the stream the caller names
// (torch's current stream: the buffers are torch tensors), like tip_bias_relu_affine_f32_dev. -----------------------------------
static int unet_launch_check(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TIP_ERR_HIP, "launch %s: %s", what, hipGetErrorString(e));
    return TIP_OK;
}

// the range word's way to the host: one thread stores it into pinned host memory, in stream order (no copy engine, no second queue)
static __global__ void k_unet_range_fetch(const unsigned *__restrict__ word, int *__restrict__ host) { *host = (int)*word; }

// The calling thread's range word of the fp16-piece kernels (tip_unet_conv.h: uc_range_flag): made on the thread's first U-Net
// launch or range call, zeroed in stream order in front of whatever that call queues on `s`, released with the context.  nullptr
// on failure (error text set).
static unsigned *unet_status_word(Ctx &c, hipStream_t s)
{
    if (c.unet_status) return c.unet_status;
    unsigned *w = nullptr;
    int *h = nullptr;
    hipError_t e = hipMalloc(&w, sizeof(unsigned));
    if (e == hipSuccess) e = hipHostMalloc(&h, sizeof(int), hipHostMallocMapped);
    if (e == hipSuccess) e = hipMemsetAsync(w, 0, sizeof(unsigned), s);
    if (e != hipSuccess) {
        if (w) (void)hipFree(w);
        if (h) (void)hipHostFree(h);
        fail(TIP_ERR_HIP, "the U-Net's range word: %s", hipGetErrorString(e));
        return nullptr;
    }
    c.unet_status = w;
    c.unet_status_host = h;
    return w;
}

static int prep_cu_count()
{
    static std::atomic<int> cus{0};          // (same device model on every GPU of a node)
    int v = cus.load(std::memory_order_relaxed);
    if (!v) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, ctx().device) != hipSuccess || v < 1) v = 256;
        cus.store(v, std::memory_order_relaxed);
    }
    return v;
}

// pl.py:90-122 + 21-29 for a device-resident image: img = (c, a, b) float64 with element strides (cstride, sa, sb), every channel
// plane dense (sa == 1 && sb == a, or sb == 1 && sa == b); kind = dtype of the ORIGINAL image (0 float64, 1 float32, 2 integer:
// normalize_channel's clip values take it).  out = (c, bp, ap) float32, zero-filled in front: out[c][bp - b + j][ap - a + i] =
// normalised img[c][i][j].  Launches on `stream` (torch's current stream: the buffers are torch tensors) and returns at once.
int tip_unet_prepare_f64_dev(const double *img, int c, int a, int b, long cstride, long sa, long sb, int kind, float *out, int ap, int bp,
                             void *stream)
{
    Ctx &cx = ctx();
    if (!cx.stream) return TIP_ERR_HIP;
    if (!img || !out || c < 1 || c > PREP_MAXC || a < 1 || b < 1 || ap < a || bp < b || kind < 0 || kind > 2)
        return fail(TIP_ERR_ARG, "tip_unet_prepare_f64_dev: bad arguments");
    const bool a_contig = sa == 1 && sb == a, b_contig = sb == 1 && sa == b;
    if (!a_contig && !b_contig) return fail(TIP_ERR_UNSUPPORTED, "tip_unet_prepare_f64_dev: every channel plane must be dense");
    if (!cx.prep_ws) TIP_HIP(hipMalloc(&cx.prep_ws, sizeof(PrepState)));      // (k_prep_reset initialises what a call uses)
    PrepState *st = (PrepState *)cx.prep_ws;
    hipStream_t s = (hipStream_t)stream;
    const long n = (long)a * b;
    // numpy: virtual index (n - 1) q, previous = floor, gamma = the fraction (function_base.py _quantile / _lerp)
    auto split = [&](double q, long long &prev, double &g) {
        const double virt = (double)(n - 1) * q;
        prev = (long long)floor(virt);
        g = virt - (double)prev;
        if (prev < 0) prev = 0;
        if (prev > n - 1) prev = n - 1;
    };
    long long r1, r99;
    double g1, g99;
    split(1.0 / 100.0, r1, g1);
    split(99.0 / 100.0, r99, g99);
    hipLaunchKernelGGL(k_prep_reset, dim3(PREP_BINS * 2 / PREP_T, (unsigned)c), dim3(PREP_T), 0, s, st, r1, r99);
    // a fixed number of workgroups, two per CU over all channels, each at least one stripe of 16-byte loads long
    const dim3 dgrid((unsigned)std::max<long>(1, std::min<long>(cdiv(n, 2 * PREP_T), std::max(1, 2 * prep_cu_count() / c))), (unsigned)c);
    hipLaunchKernelGGL(k_prep_digit<0>, dgrid, dim3(PREP_T), 0, s, img, cstride, n, st, 51, 13);
    for (int shift = 38; shift >= 12; shift -= 13) hipLaunchKernelGGL(k_prep_digit<1>, dgrid, dim3(PREP_T), 0, s, img, cstride, n, st, shift, 13);
    hipLaunchKernelGGL(k_prep_digit<2>, dgrid, dim3(PREP_T), 0, s, img, cstride, n, st, 0, 12);
    hipLaunchKernelGGL(k_prep_finish, dim3(1), dim3(64), 0, s, st, c, g1, g99, kind);
    if (ap != a || bp != b) TIP_HIP(hipMemsetAsync(out, 0, (size_t)c * ap * bp * sizeof(float), s));
    const dim3 ngrid((unsigned)cdiv(a, 32), (unsigned)cdiv(b, 32), (unsigned)c);
    if (a_contig)
        hipLaunchKernelGGL(k_prep_normalize<true>, ngrid, dim3(256), 0, s, img, cstride, sa, sb, a, b, (const PrepState *)st, kind == 1 ? 1 : 0, out, ap, bp, ap - a, bp - b);
    else
        hipLaunchKernelGGL(k_prep_normalize<false>, ngrid, dim3(256), 0, s, img, cstride, sa, sb, a, b, (const PrepState *)st, kind == 1 ? 1 : 0, out, ap, bp, ap - a, bp - b);
    return unet_launch_check("unet_prepare");
}

// The flavour of k_unet_conv a descriptor's launch runs, and everything else that follows from the descriptor and the tuning alone.
// `which` is the code include/tissue_hip.h tabulates next to tip_unet_conv_flavour.
struct ConvPlan {
    int which;                     // 0 <2,8,2>  1 <2,16,2>  2 <2,16,4>  3 <3,8,2>  4 <2,16,2,2>  6 <2,16,4,1,3>
    int th, spb;                   // tile rows, steps per barrier
    int ntiles, nblks, xcd_map;
    size_t lds;
};

// Validates the descriptor and chooses the flavour: TIP_OK and `pl`, or the error tip_unet_conv_dev returns.  Touches no device.
static int unet_conv_plan(const tip_unet_conv_desc *d, ConvPlan &pl)
{
    if (!d || !d->in0 || !d->weights || (!d->bias && !d->raw_out) || (!d->out && !d->head_out && !d->raw_out)) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: null pointer");
    if (d->planes != 2 && d->planes != 3) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: planes must be 2 or 3");
    if (d->format != 0 && d->format != 1) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: format is 0 (bf16 pieces) or 1 (fp16 pieces)");
    if (d->format == 1 && (d->planes != 2 || !(d->acc_scale > 0.f))) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: fp16 pieces come in two planes with a positive acc_scale");
    if (d->h < 8 || d->w < UC_TW || d->h % 8 || d->w % UC_TW)
        return fail(TIP_ERR_UNSUPPORTED, "tip_unet_conv_dev: the grid %dx%d is not a multiple of the 8x%d pixel tile", d->h, d->w, UC_TW);
    if (d->c0 < UC_KC || d->c0 % UC_KC || d->c1 < 0 || d->c1 % UC_KC || (d->c1 > 0 && !d->in1) || d->cout < UC_BN || d->cout % UC_BN)
        return fail(TIP_ERR_UNSUPPORTED, "tip_unet_conv_dev: channels (%d + %d -> %d) must be multiples of %d / %d", d->c0, d->c1, d->cout, UC_KC, UC_BN);
    if (d->ntaps < 1 || d->ntaps > 9 || d->sy < 1 || d->sx < 1 || d->oy < 0 || d->ox < 0 ||
        (d->h - 1) * d->sy + d->oy >= d->out_h || (d->w - 1) * d->sx + d->ox >= d->out_w)
        return fail(TIP_ERR_ARG, "tip_unet_conv_dev: bad taps / output mapping");
    if ((d->scale == nullptr) != (d->shift == nullptr)) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: scale and shift come together");
    // a tile's halo window ((tile rows + 2) image rows of one plane) is addressed through 32-bit buffer offsets; tensors may be any size
    if (18L * d->w * (d->c0 > d->c1 ? d->c0 : d->c1) * 2 >= (1L << 32) - 65536)
        return fail(TIP_ERR_UNSUPPORTED, "tip_unet_conv_dev: 18 rows of %d pixels x %d channels exceed the 4 GB a buffer resource addresses",
                    d->w, d->c0 > d->c1 ? d->c0 : d->c1);
    for (int t = 0; t < d->ntaps; ++t)
        if (d->dy[t] < -1 || d->dy[t] > 1 || d->dx[t] < -1 || d->dx[t] > 1) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: tap offsets are -1, 0 or 1");
    if (d->head_out && (!d->head_w || !d->head_b || d->cout != UC_BN || !d->scale || d->pool_out || d->sy != 1 || d->sx != 1 || d->oy != 0 || d->ox != 0 ||
                        d->out_h != d->h || d->out_w != d->w))
        return fail(TIP_ERR_ARG, "tip_unet_conv_dev: the fused head needs a 128-channel Conv2D + BatchNorm layer with the plain output mapping");
    if (d->pool_out && (d->sy != 1 || d->sx != 1 || d->oy != 0 || d->ox != 0 || d->out_h != d->h || d->out_w != d->w))
        return fail(TIP_ERR_ARG, "tip_unet_conv_dev: pool_out needs the plain output mapping");
    if (d->raw_out && (d->head_out || d->pool_out)) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: raw output goes without the head and the pooled map");
    if (d->seed && (d->sy != 1 || d->sx != 1 || d->oy != 0 || d->ox != 0 || d->out_h != d->h || d->out_w != d->w))
        return fail(TIP_ERR_ARG, "tip_unet_conv_dev: the accumulator seed needs the plain output mapping");
    // 16-row tiles (one 512-thread workgroup per CU) where the grid allows: half the weight copies per MFMA, and LDS for five
    // weight buffers (copies four steps ahead) when the stencil has >= 4 taps; two pieces only (LDS)
    const int t8 = tuning().unet_tile8;
    // (measured per layer at 2048^2: the short K loops of the 128-channel 3x3 layers gain 1-3 % from two workgroups per CU -- one's
    // epilogue behind the other's products -- every other layer is faster with the shared weight tile of the 16-row workgroup)
    const bool want8 = t8 == 1 || (t8 < 0 && d->ntaps == 9 && d->c0 + d->c1 <= 128);
    const int th = (d->planes == 2 && d->h % 16 == 0 && !want8) ? 16 : 8;
    const int dist = (th == 16 && d->ntaps >= 4) ? 4 : 2;
    const int da = (th == 16 && d->ntaps <= 2) ? 2 : 1;       // one- and two-tap stencils: activation tiles two chunks ahead
    const int threads = th * 32, hp = UC_HW * (th + 2);
    pl.th = th;
    pl.ntiles = (d->h / th) * (d->w / UC_TW); pl.nblks = d->cout / UC_BN;
    pl.xcd_map = (tuning().unet_xcd_map && pl.nblks > 1 && pl.ntiles % 8 == 0) ? 1 : 0;
    const int a_per = (d->planes * ((hp * 2 + 63) / 64) * 64 + threads - 1) / threads;     // (a plane's halo tile padded to whole waves, as in the kernel)
    // three steps per barrier: 3x3 stencils on 16-row tiles (a chunk's nine taps in three iterations, nine weight buffers);
    // TIP_UNET_SPB = 1 keeps one step per barrier, every larger value means three
    pl.spb = (th == 16 && dist == 4 && d->ntaps == 9 && tuning().unet_spb > 1) ? 3 : 1;
    pl.lds = (size_t)(da + 1) * a_per * threads * 16 + (size_t)(pl.spb > 1 ? 3 * pl.spb : dist + 1) * d->planes * 256 * 16;
    // the kernel flavour <pieces, tile rows, weight steps ahead, activation chunks ahead, steps per barrier>
    if (d->planes == 3) pl.which = 3;        // <3, 8, 2>
    else if (th == 8) pl.which = 0;          // <2, 8, 2>
    else if (pl.spb == 3) pl.which = 6;      // <2, 16, 4, 1, 3>: 3x3 stencils
    else if (dist == 4) pl.which = 2;        // <2, 16, 4>: four and more taps, one step per barrier
    else if (da == 2) pl.which = 4;          // <2, 16, 2, 2>: one and two taps
    else pl.which = 1;                       // <2, 16, 2>: three taps
    return TIP_OK;
}

int tip_unet_conv_flavour(const tip_unet_conv_desc *d)
{
    ConvPlan pl;
    const int rc = unet_conv_plan(d, pl);
    return rc ? rc : pl.which;
}

int tip_unet_conv_dev(const tip_unet_conv_desc *d, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    ConvPlan pl;
    if (const int rc = unet_conv_plan(d, pl)) return rc;
    ConvParams p;
    p.in0 = (const uint16_t *)d->in0; p.in1 = (const uint16_t *)(d->c1 > 0 ? d->in1 : d->in0);
    p.c0 = d->c0; p.c1 = d->c1; p.H = d->h; p.W = d->w;
    p.w = (const uint16_t *)d->weights; p.ntaps = d->ntaps;
    for (int t = 0; t < 9; ++t) {
        p.dy[t] = t < d->ntaps ? d->dy[t] : 0; p.dx[t] = t < d->ntaps ? d->dx[t] : 0;
    }
    p.cout = d->cout; p.bias = d->bias; p.scale = d->scale; p.shift = d->shift;
    p.out = (uint16_t *)d->out; p.outH = d->out_h; p.outW = d->out_w; p.sy = d->sy; p.sx = d->sx; p.oy = d->oy; p.ox = d->ox;
    p.pool_out = (uint16_t *)d->pool_out;
    p.acc_scale = d->format == 1 ? d->acc_scale : 1.f;
    p.status = nullptr;
    if (d->format == 1 && !d->raw_out && !(p.status = unet_status_word(c, (hipStream_t)stream))) return TIP_ERR_HIP;
#ifdef UC_TRACE
    static unsigned long long *trace_dev = nullptr;
    if (!trace_dev) { TIP_HIP(hipMalloc(&trace_dev, 1024)); }
    TIP_HIP(hipMemsetAsync(trace_dev, 0, 1024, (hipStream_t)stream));
    p.trace = trace_dev;
#endif
    p.head_w = d->head_w; p.head_b = d->head_b; p.head_out = d->head_out;
    p.raw_out = d->raw_out; p.seed = d->seed;
    p.xcd_map = pl.xcd_map;
    const int which = pl.which, threads = pl.th * 32;
    const size_t lds = pl.lds;
    const dim3 grid = p.xcd_map ? dim3((unsigned)(pl.ntiles * pl.nblks)) : dim3(pl.ntiles, pl.nblks);
    hipStream_t s = (hipStream_t)stream;
    // the >64 KB dynamic LDS attribute is set once per (device, kernel): one atomic bit each
    static std::atomic<unsigned> attr_done[64];
    const unsigned bit = 1u << (which + (d->format ? 9 : 0));
    const int dev = c.device >= 0 && c.device < 64 ? c.device : 0;
#define UC_FLAVOUR(W, ...)                                                                                                                  \
    case W: {                                                                                                                               \
        if (!(attr_done[dev].load(std::memory_order_acquire) & bit)) {                                                                      \
            TIP_HIP(hipFuncSetAttribute((const void *)(__VA_ARGS__), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                \
            attr_done[dev].fetch_or(bit, std::memory_order_release);                                                                        \
        }                                                                                                                                   \
        hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(threads), lds, s, p);                                                                  \
    } break;
    if (d->format == 0) {
        switch (which) {
            UC_FLAVOUR(3, k_unet_conv<3, 8, 2>)
            UC_FLAVOUR(6, k_unet_conv<2, 16, 4, 1, 3>)
            UC_FLAVOUR(2, k_unet_conv<2, 16, 4>)
            UC_FLAVOUR(4, k_unet_conv<2, 16, 2, 2>)
            UC_FLAVOUR(1, k_unet_conv<2, 16, 2>)
            UC_FLAVOUR(0, k_unet_conv<2, 8, 2>)
        }
    } else {
        switch (which) {
            UC_FLAVOUR(6, k_unet_conv<2, 16, 4, 1, 3, true>)
            UC_FLAVOUR(2, k_unet_conv<2, 16, 4, 1, 1, true>)
            UC_FLAVOUR(4, k_unet_conv<2, 16, 2, 2, 1, true>)
            UC_FLAVOUR(1, k_unet_conv<2, 16, 2, 1, 1, true>)
            UC_FLAVOUR(0, k_unet_conv<2, 8, 2, 1, 1, true>)
        }
    }
#undef UC_FLAVOUR
#ifdef UC_TRACE
    {
        unsigned long long tr[128];
        TIP_HIP(hipStreamSynchronize(s));
        TIP_HIP(hipMemcpy(tr, trace_dev, sizeof tr, hipMemcpyDeviceToHost));
        for (int k = 0; k < pl.th / 2; ++k) {
            const unsigned long long *t = tr + 16 * k;
            const double n = (double)t[4];
            fprintf(stderr, "UC_TRACE th %d spb %d taps %d cin %d cout %d grid %dx%d wave %d simd %d: per STEP (shader clocks; sums over the loop / steps): copies %.0f, products %.0f (first MFMA out after %.0f), "
                            "vmcnt wait %.0f, barrier %.0f, total %.0f; steps %.0f; whole loop %.0f, prologue %.0f, epilogue %.0f clocks\n",
                    pl.th, pl.spb, d->ntaps, d->c0 + d->c1, d->cout, d->h, d->w, k, (int)((t[7] >> 4) & 3), t[0] / n, t[2] / n, t[1] / n, t[6] / n, (t[3] - t[6]) / n, t[5] / n, n, (double)t[5], (double)t[8], (double)t[9]);
        }
    }
#endif
    return unet_launch_check("unet_conv");
}

// Border pass of a composed decoder level (tip_unet_conv.h) on the float32 partial of 2h x 2w x cout values: the edge
// bias table on all four edges, then the bottom row's, the right column's and the corner's linear corrections, in stream order.
int tip_unet_compose_border_dev(const void *x, int planes, int format, int h, int w, int cin, int cout, const float *row_w, const float *col_w,
                                const float *corner_w, const float *bias_tab, float *part, float xscale, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!x || !row_w || !col_w || !corner_w || !bias_tab || !part || (planes != 2 && planes != 3) || (format != 0 && !(format == 1 && planes == 2)) ||
        h < 1 || w < 1 || cin < 1 || cout < 128 || cout % 128 || !(xscale > 0.f))
        return fail(TIP_ERR_ARG, "tip_unet_compose_border_dev: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int H2 = 2 * h, W2 = 2 * w;
    const long nb = (2L * W2 + 2L * (H2 - 2)) * (cout / 4);
    hipLaunchKernelGGL(k_unet_compose_edge_bias, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, s, part, H2, W2, cout, bias_tab);
    EdgeParams p;
    p.x = (const uint16_t *)x; p.xplane = (long)h * w * cin; p.planes = planes; p.f16 = format; p.xscale = xscale;
    p.cin = cin; p.cout = cout; p.part = part;
    const long wstride = (long)cin * cout;
    // bottom row: positions run along x on input row h - 1, output row 2h - 1
    p.L = w; p.x0 = (long)(h - 1) * w * cin; p.xstep = cin; p.tapmask = 0x1f;
    for (int t = 0; t < 5; ++t) p.wgt[t] = row_w + t * wstride;
    p.o0 = (long)(H2 - 1) * W2 * cout; p.ostep = cout;
    hipLaunchKernelGGL(k_unet_compose_edge, dim3((unsigned)cdiv(p.L, EB_J), (unsigned)(cout / EB_CO)), dim3(EB_CO * EB_G), 0, s, p);
    // right column: positions run along y on input column w - 1, output column 2w - 1
    p.L = h; p.x0 = (long)(w - 1) * cin; p.xstep = (long)w * cin;
    for (int t = 0; t < 5; ++t) p.wgt[t] = col_w + t * wstride;
    p.o0 = (long)(W2 - 1) * cout; p.ostep = (long)W2 * cout;
    hipLaunchKernelGGL(k_unet_compose_edge, dim3((unsigned)cdiv(p.L, EB_J), (unsigned)(cout / EB_CO)), dim3(EB_CO * EB_G), 0, s, p);
    // corner: the doubly removed term back -- one position, its parity-1 pixel, the tap at offset 0
    p.L = 1; p.x0 = ((long)(h - 1) * w + (w - 1)) * cin; p.xstep = cin; p.tapmask = 0x8;
    for (int t = 0; t < 5; ++t) p.wgt[t] = corner_w;
    p.o0 = ((long)(H2 - 1) * W2 + (W2 - 2)) * cout; p.ostep = cout;
    hipLaunchKernelGGL(k_unet_compose_edge, dim3(1, (unsigned)(cout / EB_CO)), dim3(EB_CO * EB_G), 0, s, p);
    return unet_launch_check("unet_compose_border");
}

int tip_unet_conv_first_dev(const float *in, int h, int w, const float *wgt, const float *bias, const float *scale, const float *shift,
                            void *out, int planes, int format, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !wgt || !bias || !scale || !shift || !out || h < 1 || w < 1 || w % FIRST_RUN || ((long)h * w) % FIRST_PIX || (planes != 2 && planes != 3) ||
        (format != 0 && !(format == 1 && planes == 2)))
        return fail(TIP_ERR_ARG, "tip_unet_conv_first_dev: bad arguments (w must be a multiple of 32, h * w of 256)");
    const dim3 grid((unsigned)((long)h * w / FIRST_PIX));
    hipStream_t s = (hipStream_t)stream;
    unsigned *status = nullptr;
    if (format == 1 && !(status = unet_status_word(c, s))) return TIP_ERR_HIP;
    if (format == 1) hipLaunchKernelGGL((k_unet_conv_first<2, true>), grid, dim3(256), 0, s, in, h, w, wgt, bias, scale, shift, (uint16_t *)out, status);
    else if (planes == 2) hipLaunchKernelGGL(k_unet_conv_first<2>, grid, dim3(256), 0, s, in, h, w, wgt, bias, scale, shift, (uint16_t *)out, status);
    else hipLaunchKernelGGL(k_unet_conv_first<3>, grid, dim3(256), 0, s, in, h, w, wgt, bias, scale, shift, (uint16_t *)out, status);
    return unet_launch_check("unet_conv_first");
}

// The same layer for the fp16 pieces on the matrix cores (k_unet_conv_first_mfma): packed_weights as every layer's, one tap x 32
// input channels whose rows 0 .. 17 are the 18 (tap, channel) terms.  Which of the two entries a forward pass calls is decided
// in one place, by the caller, from tip_unet_first_mfma().
int tip_unet_conv_first_packed_dev(const float *in, int h, int w, const void *packed_weights, float acc_scale, const float *bias,
                                   const float *scale, const float *shift, void *out, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !packed_weights || !bias || !scale || !shift || !out || h < 1 || w < 1 || w % FIRST_RUN || ((long)h * w) % FIRST_PIX)
        return fail(TIP_ERR_ARG, "tip_unet_conv_first_packed_dev: bad arguments (w must be a multiple of 32, h * w of 256)");
    hipStream_t s = (hipStream_t)stream;
    unsigned *status = unet_status_word(c, s);
    if (!status) return TIP_ERR_HIP;
    // four waves per workgroup, a wave walks the 32-pixel segments wave, wave + waves, ...: TIP_UNET_FIRST > 1 is the number of
    // workgroups per CU (256 CUs) the launch is cut to; the default was chosen by measurement
    const long wgs = (long)h * w / 128;                    // one segment per wave
    const int per_cu = tuning().unet_first_mfma > 1 ? tuning().unet_first_mfma : FIRST_MFMA_WGS_PER_CU;
    const dim3 grid((unsigned)std::min(wgs, 256L * per_cu));
    hipLaunchKernelGGL(k_unet_conv_first_mfma, grid, dim3(256), 0, s, in, h, w, (const uint16_t *)packed_weights, acc_scale, bias, scale, shift,
                       (uint16_t *)out, status);
    return unet_launch_check("unet_conv_first_mfma");
}

int tip_unet_first_mfma(void) { return tuning().unet_first_mfma != 0; }

// The fp16 pieces' range flag (tip_unet_conv.h: uc_range_flag).  reset: the calling thread's word is zeroed in stream order; read:
// the word as it stands behind everything queued on `stream` so far -- the host waits for that stream alone.
int tip_unet_range_reset(void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    const bool fresh = !c.unet_status;
    unsigned *w = unet_status_word(c, (hipStream_t)stream);
    if (!w) return TIP_ERR_HIP;
    if (!fresh) TIP_HIP(hipMemsetAsync(w, 0, sizeof(unsigned), (hipStream_t)stream));
    return TIP_OK;
}

int tip_unet_range_read(void *stream, int *flags)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!flags) return fail(TIP_ERR_ARG, "tip_unet_range_read: null pointer");
    unsigned *w = unet_status_word(c, (hipStream_t)stream);
    if (!w) return TIP_ERR_HIP;
    int *host_dev = nullptr;        // (the pinned word as the device addresses it)
    TIP_HIP(hipHostGetDevicePointer((void **)&host_dev, c.unet_status_host, 0));
    hipLaunchKernelGGL(k_unet_range_fetch, dim3(1), dim3(1), 0, (hipStream_t)stream, (const unsigned *)w, host_dev);
    int rc = unet_launch_check("unet_range_fetch");
    if (rc) return rc;
    TIP_HIP(hipStreamSynchronize((hipStream_t)stream));
    *flags = *(volatile int *)c.unet_status_host;
    return TIP_OK;
}

int tip_unet_pool2_dev(const void *in, int h, int w, int ch, int planes, int format, void *out, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !out || h < 2 || w < 2 || (h & 1) || (w & 1) || ch < 8 || ch % 8 || (planes != 2 && planes != 3) || (format != 0 && !(format == 1 && planes == 2)))
        return fail(TIP_ERR_ARG, "tip_unet_pool2_dev: bad arguments");
    const long n = (long)(h / 2) * (w / 2) * (ch / 8);
    hipStream_t s = (hipStream_t)stream;
    if (format == 1) hipLaunchKernelGGL((k_unet_pool2<2, true>), dim3(cdiv(n, 256)), dim3(256), 0, s, (const uint16_t *)in, h, w, ch, (uint16_t *)out);
    else if (planes == 2) hipLaunchKernelGGL(k_unet_pool2<2>, dim3(cdiv(n, 256)), dim3(256), 0, s, (const uint16_t *)in, h, w, ch, (uint16_t *)out);
    else hipLaunchKernelGGL(k_unet_pool2<3>, dim3(cdiv(n, 256)), dim3(256), 0, s, (const uint16_t *)in, h, w, ch, (uint16_t *)out);
    return unet_launch_check("unet_pool2");
}

int tip_unet_head_dev(const void *in, long npix, const float *wgt, const float *bias, float *out, int planes, int format, int logits, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !wgt || !bias || !out || npix < 1 || (planes != 2 && planes != 3) || (format != 0 && !(format == 1 && planes == 2)))
        return fail(TIP_ERR_ARG, "tip_unet_head_dev: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(npix * 8, 256));
    if (format == 1) hipLaunchKernelGGL((k_unet_head<2, true>), grid, dim3(256), 0, s, (const uint16_t *)in, npix, wgt, bias, out, logits);
    else if (planes == 2) hipLaunchKernelGGL(k_unet_head<2>, grid, dim3(256), 0, s, (const uint16_t *)in, npix, wgt, bias, out, logits);
    else hipLaunchKernelGGL(k_unet_head<3>, grid, dim3(256), 0, s, (const uint16_t *)in, npix, wgt, bias, out, logits);
    return unet_launch_check("unet_head");
}

}  // extern "C"
