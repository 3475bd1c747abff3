// tip_unet_prepare.hip -- U1: prepare_image (pl.py:21-29, 90-122) on a device-resident (C, A, B) float64 image.
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
#include "tip_internal.h"
#include <algorithm>
#include <atomic>

namespace tip {

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
        a0 = wave_min(a0); a1 = wave_min(a1);
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
    // both ranks: every thread sums PREP_PER bins, a block scan of the sums finds the thread whose bins hold the rank
    const unsigned int *h[2] = {sh[0], sh[one ? 0 : 1]};
    long long r[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        r[w] = st->rank[c][w];
        long long sum = 0, all;
#pragma unroll
        for (int k = 0; k < PREP_PER; ++k) sum += h[w][tid * PREP_PER + k];
        long long cum = block_exclusive_scan<PREP_W>(sum, s_wsum[w], all);
        if (cum <= r[w] && r[w] < cum + sum) {                   // (one thread)
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

}  // namespace tip

using namespace tip;

extern "C" {

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
    return launch_check("unet_prepare");
}

}  // extern "C"
