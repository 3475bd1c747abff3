// tip_project.hip -- time_point_surface_projection (sp.py:17-85) as a device pipeline.
//
//   P1  uint16 -> float32, airyscan offset (sp.py:26-29)            fused into every reader of the stack
//   P2  95th percentile of the non-zero reference voxels + clip     exact 65536-bin histogram (sp.py:32-36)
//   P3  Gaussian (0.5,1,1)  (sp.py:37)                              exact scipy-order correlate passes
//   P4  Gaussian (0.5,30,30) score (sp.py:55)                       long-kernel passes (tip_corr.h)
//   P5  argmax over z, first maximum (sp.py:61)
//   P6/P7 one-hot mask + Gaussian (1,2,2) (sp.py:62-71)             z pass = ZxZ table; y pass, x pass and the weighted z-max
//   P8  per-channel max_z(image * mask) -> float64 (sp.py:72-81)    in one kernel (k_mask_wmax_fused), or the dense fallback:
//                                                                   y pass from the z-map, x pass fused with the z-max
#include "tip_slide.h"
#include "tip_preblur.h"
#include "tip_corr.h"
#include "tip_corr_f16.h"
#include "tip_manifold.h"
#include "tip_project_binned.h"
#include <algorithm>
#include <atomic>
#include <cstdlib>

namespace tip {

struct ClipInfo {
    double p95d;
    float p95;
    int has;
};

// ---- P2: histogram of the (offset-corrected, airy_offset) reference channel ------------------------------
// One persistent 1024-thread block per CU with a private 65536-bin LDS histogram of 16-bit counters packed two per dword.
// A block walks chunks of 57344 voxels; a chunk adds at most 57344 to a bin, so between chunks every bin that has reached
// 8192 is moved to the global histogram (a handful per chunk) and no counter can overflow; the table is cleared once and
// flushed once per block.  (One block per chunk -- 2196 clears, scans and full flushes of the 128 KB table, 6.6 M global
// atomics on ~3000 addresses -- took 0.13 ms; the 252 MB read alone is 0.06 ms.)
constexpr int HIST_PER_BLOCK = 57344;  // 7 trips of 1024 threads x 8 voxels; 57344 + 8191 < 65536
// the packed table (32768 dwords, bin b in half b & 1 of dword b >> 1) of a 1024-thread block: clear, bump, flush all
__device__ __forceinline__ void hist_clear(unsigned int *h)
{
    for (int i = threadIdx.x; i < 32768; i += 1024) h[i] = 0;
    __syncthreads();
}
__device__ __forceinline__ void hist_bump(unsigned int *h, int val) { atomicAdd(&h[val >> 1], 1u << (16 * (val & 1))); }
__device__ __forceinline__ void hist_flush_all(const unsigned int *h, unsigned long long *__restrict__ hist)
{
    for (int i = threadIdx.x; i < 32768; i += 1024) {
        const unsigned int c = h[i];
        if (c & 0xffffu) atomicAdd(&hist[2 * i], (unsigned long long)(c & 0xffffu));
        if (c >> 16) atomicAdd(&hist[2 * i + 1], (unsigned long long)(c >> 16));
    }
}

__global__ void __launch_bounds__(1024) k_hist_u16(const uint16_t *__restrict__ in, long n, int airy,
                                                   unsigned long long *__restrict__ hist)
{
    __shared__ unsigned int h[32768];
    hist_clear(h);
    const long nchunks = (n + HIST_PER_BLOCK - 1) / HIST_PER_BLOCK;
    for (long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const long base = chunk * HIST_PER_BLOCK;
        constexpr int TRIPS = HIST_PER_BLOCK / (1024 * 8);
        if (base + HIST_PER_BLOCK <= n && ((((uintptr_t)(in + base)) & 15) == 0)) {
            // whole chunk: all seven 16-byte loads of the thread in flight before the first LDS atomic (one block per CU:
            // nothing else hides the memory latency)
            uint4 v[TRIPS];
#pragma unroll
            for (int k = 0; k < TRIPS; ++k) v[k] = *reinterpret_cast<const uint4 *>(in + base + ((long)k * 1024 + threadIdx.x) * 8);
#pragma unroll
            for (int k = 0; k < TRIPS; ++k) {
                const unsigned int w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) hist_bump(h, airy_offset((int)((w[j] >> (16 * s)) & 0xffffu), airy));
                }
            }
        } else {
            for (int k = 0; k < TRIPS; ++k) {
                const long i0 = base + ((long)k * 1024 + threadIdx.x) * 8;
                for (int j = 0; j < 8; ++j)
                    if (i0 + j < n) hist_bump(h, airy_offset((int)in[i0 + j], airy));
            }
        }
        __syncthreads();
        if (chunk + gridDim.x < nchunks) {      // another chunk follows: make room in the bins that are filling up
            for (int i = threadIdx.x; i < 32768; i += 1024) {
                unsigned int c = h[i];
                if ((c & 0xffffu) >= 8192u) { atomicAdd(&hist[2 * i], (unsigned long long)(c & 0xffffu)); c &= 0xffff0000u; h[i] = c; }
                if ((c >> 16) >= 8192u) { atomicAdd(&hist[2 * i + 1], (unsigned long long)(c >> 16)); h[i] = c & 0xffffu; }
            }
            __syncthreads();
        }
    }
    hist_flush_all(h, hist);
}

// The same histogram over a sub-box [z0,z1) x [y0,y1) x [x0,x1) of one channel plane stack (row length X, plane size
// Y*X): spatially tiled frames (config 5) count every voxel once -- tile interiors -- and add the tiles' histograms up
// before anyone clips (the percentile is a property of the whole frame).
__global__ void __launch_bounds__(1024) k_hist_u16_box(const uint16_t *__restrict__ in, int Y, int X, int z0, int y0, int x0, int bz,
                                                       int by, int bx, int airy, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned int h[32768];
    hist_clear(h);
    const long n = (long)bz * by * bx;
    const long base = (long)blockIdx.x * HIST_PER_BLOCK;
    for (int k = 0; k < HIST_PER_BLOCK / 1024; ++k) {
        const long i = base + (long)k * 1024 + threadIdx.x;
        if (i < n) {
            const int x = (int)(i % bx), y = (int)((i / bx) % by), z = (int)(i / ((long)bx * by));
            hist_bump(h, airy_offset((int)in[((long)(z0 + z) * Y + (y0 + y)) * X + (x0 + x)], airy));
        }
    }
    __syncthreads();
    hist_flush_all(h, hist);
}

// np.percentile(nonzero, 95) with numpy 1.26 arithmetic (see oracle.percentile_linear): one block.
// (with_zero: over all voxels, zeros included -- the second channel of method 'multi_channel', sp.py:46)
__global__ void __launch_bounds__(1024) k_percentile95(const unsigned long long *__restrict__ hist, ClipInfo *out, int with_zero)
{
    // 1024 threads x 64 bins.  Chunk sums -> block-wide scan -> the chunk that holds a rank is the one thread whose
    // [exclusive, inclusive) range contains it -> one wave scans that chunk's 64 bins.
    // (A single thread walking the 1024 chunk sums and the bins took 35 us: the whole projection waits for this value.)
    __shared__ unsigned long long wave_tot[16];
    __shared__ int s_chunk[2];
    __shared__ unsigned long long s_before[2];
    __shared__ int s_val[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long s = 0, n;
    for (int b = t * 64; b < t * 64 + 64; ++b)
        if (b > 0 || with_zero) s += hist[b];
    const unsigned long long exc = block_exclusive_scan<16>(s, wave_tot, n), inc = exc + s;
    if (n == 0) {
        if (t == 0) { out->has = 0; out->p95 = 0.f; out->p95d = 0.0; }
        return;
    }
    const double quant = 95.0 / 100.0;
    const double virt = (double)(n - 1) * quant;  // numpy 'linear': (n - 1) * quantiles
    const double fl = floor(virt);
    const double gamma = virt - fl;
    long long prev = (long long)fl;
    if (prev < 0) prev = 0;
    if (prev > (long long)n - 1) prev = (long long)n - 1;
    long long next = prev + 1;
    if (next > (long long)n - 1) next = (long long)n - 1;
    if (s > 0) {          // the chunk whose cumulative range holds the rank (exactly one thread per rank)
        if (exc <= (unsigned long long)prev && (unsigned long long)prev < inc) { s_chunk[0] = t; s_before[0] = exc; }
        if (exc <= (unsigned long long)next && (unsigned long long)next < inc) { s_chunk[1] = t; s_before[1] = exc; }
    }
    __syncthreads();
    if (wave < 2) {       // wave 0: value at rank prev, wave 1: at rank next
        const unsigned long long k = (unsigned long long)(wave == 0 ? prev : next) - s_before[wave];
        const int b = s_chunk[wave] * 64 + lane;
        const unsigned long long ci = wave_inclusive_scan((b > 0 || with_zero) ? hist[b] : 0ULL);
        // first bin whose inclusive count exceeds k
        const unsigned long long hit = __ballot(ci > k);
        if (lane == 0) s_val[wave] = hit ? s_chunk[wave] * 64 + (__ffsll((long long)hit) - 1) : 65535;
    }
    __syncthreads();
    if (t != 0) return;
    const float lo = (float)s_val[0], hi = (float)s_val[1];
    const double diff = (double)(hi - lo);
    double res = (double)lo + diff * gamma;
    if (gamma >= 0.5) res = (double)hi - diff * (1.0 - gamma);
    out->p95d = res;
    out->p95 = (float)res;  // numpy 1.x value-based casting: compared and assigned as float32 (sp.py:36)
    out->has = 1;
}

// ---- P1+P2 fused reader of the reference channel ----------------------------------------------------------
struct LoadU16Clip {
    const uint16_t *p;
    long sz, sy;
    int airy;
    const ClipInfo *clip;
    __device__ __forceinline__ double operator()(int z, int y, int x) const
    {
        return (double)raw_sample(p[z * sz + y * sy + x], airy, clip->has != 0, clip->p95);
    }
};

// ---- the z-maps of pixel p from its chosen plane index (sp.py:61-62, 68-69) ----------------------------------------
__device__ __forceinline__ void emit_zmaps(long p, int plane, int Z, int min_z, int atoh_shift, int32_t *__restrict__ zsel,
                                           int32_t *__restrict__ zsel_atoh, int64_t *__restrict__ zmap, int *__restrict__ err)
{
    const int cz = min_z + plane;            // sp.py:61
    if (zmap) zmap[p] = cz;
    int ca = cz;
    if (atoh_shift != 0) {                   // sp.py:62 np.clip(chosen_z + shift, 0, Z)  (upper bound Z, sic)
        ca = cz + atoh_shift;
        ca = ca < 0 ? 0 : (ca > Z ? Z : ca);
    }
    if (cz >= Z || ca >= Z) {                // the reference's fancy index would raise IndexError (sp.py:68-69)
        atomicOr(err, 1);
        zsel[p] = cz >= Z ? Z - 1 : cz;
        zsel_atoh[p] = ca >= Z ? Z - 1 : ca;
        return;
    }
    zsel[p] = cz;
    zsel_atoh[p] = ca;
}

// ---- P5: first-maximum argmax over z ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_argmax_z(const float *__restrict__ score, int Z, long P, int min_z,
                                                  int atoh_shift, int32_t *__restrict__ zsel,
                                                  int32_t *__restrict__ zsel_atoh, int64_t *__restrict__ zmap,
                                                  int *__restrict__ err)
{
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    float best = score[p];
    int bi = 0;
    for (int z = 1; z < Z; ++z) {
        const float s = score[(long)z * P + p];
        if (s > best) { best = s; bi = z; }
    }
    emit_zmaps(p, bi, Z, min_z, atoh_shift, zsel, zsel_atoh, zmap, err);
}

__global__ void k_identity(float *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * n) out[i] = (i / n == i % n) ? 1.f : 0.f;
}

// ---- P6/P7: the z pass of a one-hot column is a table lookup -----------------------------------------------------
struct LoadMaskTable {
    const float *T;       // T[z*Zs + z0] = z-blurred one-hot(z0) at z
    const int32_t *zsel;  // (Y,X) chosen plane
    int Zs;
    long X;
    __device__ __forceinline__ double operator()(int z, int y, int x) const
    {
        return (double)T[z * Zs + zsel[(long)y * X + x]];
    }
};

// ---- P7 x pass + P8 weighted z-max, all channels in one sweep ---------------------------------------------------
// ymask: (Zs,Y,X) float32 after the z and y passes.  For every pixel: for each z, finish the x pass (exact
// scipy order), round to float32, multiply with the float32 image value and keep the per-channel maximum.
// chan_mask selects which channels this launch writes (reference vs. atoh-shifted mask, sp.py:75-79).
template <int MAXC>
__global__ void __launch_bounds__(256) k_xpass_wmax(const float *__restrict__ ymask, const uint16_t *__restrict__ img,
                                                    int C, int Zfull, int zlo, int Zs, int Y, int X, int airy,
                                                    unsigned chan_mask, Taps taps, double *__restrict__ proj)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= X) return;
    const int r = taps.n >> 1;
    const long P = (long)Y * X;
    float mx[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) mx[c] = 0.f;
    for (int z = 0; z < Zs; ++z) {
        const float *row = ymask + (long)z * P + (long)y * X;
        const float m = (float)tap_sum(r, [&](int j) { return (double)row[clampi(x - r + j, 0, X - 1)]; }, taps.w);
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (c < C && ((chan_mask >> c) & 1u)) {
                const float v = airy_offset((float)img[((long)c * Zfull + zlo + z) * P + (long)y * X + x], airy);
                const float pr = v * m;
                // np.max over z of a float32 array; first z initialises
                mx[c] = z == 0 ? pr : (pr > mx[c] ? pr : mx[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C && ((chan_mask >> c) & 1u)) proj[(long)c * P + (long)y * X + x] = (double)mx[c];
}

// ---- P7 y + x pass and P8 fused: the blurred one-hot mask never reaches HBM -----------------------------------------------
// The mask is exactly zero more than MASK_ZR = 4 planes away from every chosen plane that feeds it (9 z taps), and adding
// exact zeros changes nothing, so only the planes inside [zmin - 4, zmax + 4] of the 17-wide windows are computed: the same
// arithmetic in the same order as the dense kernels above, bit-identical to them.
// One block = FT_Y x FT_X outputs.  The chosen-plane map of the tile (+ 8-pixel halo, edges replicated) sits in LDS; plane
// by plane the block computes the y pass of the tile's columns into an LDS buffer (exact scipy order, zero outside a
// column's [zmin - 4, zmax + 4] exactly as the dense pass gives) and every thread finishes the x pass for its 8 outputs
// from that buffer, multiplies with the raw stack and keeps the per-channel maximum -- without writing the 503 MB mask
// volume and reading it back.
constexpr int MASK_R = 8, MASK_W = 2 * MASK_R + 1, MASK_ZR = 4;
constexpr int FT_Y = 16, FT_X = 128, FT_W = FT_X + 2 * MASK_R, FT_H = FT_Y + 2 * MASK_R;
template <int MAXC>
__global__ void __launch_bounds__(256) k_mask_wmax_fused(const float *__restrict__ table, const int32_t *__restrict__ zsel,
                                                         const uint16_t *__restrict__ img, int C, int Zfull, int zlo, int Zs, int Y,
                                                         int X, int airy, unsigned chan_mask, Taps taps, double *__restrict__ proj)
{
    extern __shared__ float sT[];                       // Zs * Zs: T[z * Zs + z0]
    __shared__ unsigned char zs[FT_H][FT_W];            // chosen plane, rows y0-8 .. y0+FT_Y+7, columns x0-8 .. x0+FT_X+7
    __shared__ unsigned char cmin[FT_Y][FT_W], cmax[FT_Y][FT_W];   // range of the 17-row window under every (row, column)
    __shared__ __attribute__((aligned(16))) float ybuf[2][FT_Y][FT_W];
    __shared__ int s_lo, s_hi;
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * FT_X, y0 = blockIdx.y * FT_Y;
    const long P = (long)Y * X;
    for (int i = t; i < Zs * Zs; i += 256) sT[i] = table[i];
    for (int i = t; i < FT_H * FT_W; i += 256) {
        const int r = i / FT_W, c = i - r * FT_W;
        zs[r][c] = (unsigned char)zsel[(long)clampi(y0 - MASK_R + r, 0, Y - 1) * X + clampi(x0 - MASK_R + c, 0, X - 1)];
    }
    if (t == 0) { s_lo = Zs; s_hi = -1; }
    __syncthreads();
    int lo = Zs, hi = -1;
    for (int i = t; i < FT_Y * FT_W; i += 256) {
        const int r = i / FT_W, c = i - r * FT_W;
        int a = zs[r][c], b = a;
#pragma unroll
        for (int k = 1; k < MASK_W; ++k) { const int v = zs[r + k][c]; a = min(a, v); b = max(b, v); }
        cmin[r][c] = (unsigned char)a; cmax[r][c] = (unsigned char)b;
        lo = min(lo, a); hi = max(hi, b);
    }
    lo = wave_min(lo); hi = wave_max(hi);
    if ((t & 63) == 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    const int zaB = max(s_lo - MASK_ZR, 0), zbB = min(s_hi + MASK_ZR, Zs - 1);
    // this thread's outputs: row ty, columns cx .. cx+7 of the tile; their z range = the windows cx .. cx+23 of row ty
    const int ty = t >> 4, cx = (t & 15) * 8;
    const int gy = y0 + ty, gx = x0 + cx;
    const bool live = gy < Y && gx < X;
    int za = Zs, zb = -1;
    if (live) {
        for (int c = cx; c < cx + 8 + 2 * MASK_R; ++c) { za = min(za, (int)cmin[ty][c]); zb = max(zb, (int)cmax[ty][c]); }
        za = max(za - MASK_ZR, 0); zb = min(zb + MASK_ZR, Zs - 1);
    }
    float mx[MAXC][8];
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
#pragma unroll
        for (int k = 0; k < 8; ++k) mx[c][k] = 0.f;
    for (int z = zaB; z <= zbB; ++z) {
        float(*yb)[FT_W] = ybuf[(z - zaB) & 1];
        const float *Tz = sT + z * Zs;
        for (int i = t; i < FT_Y * FT_W; i += 256) {     // y pass of plane z for the tile's columns
            const int r = i / FT_W, c = i - r * FT_W;
            float val = 0.f;
            if (z >= (int)cmin[r][c] - MASK_ZR && z <= (int)cmax[r][c] + MASK_ZR)
                val = (float)tap_sum<MASK_R>([&](int j) { return (double)Tz[zs[r + j][c]]; }, taps.w);
            yb[r][c] = val;
        }
        __syncthreads();        // (the buffer of plane z-1 is free again only after the NEXT barrier: two buffers, one barrier per plane)
        if (live && z >= za && z <= zb) {
            float v[8 + 2 * MASK_R];
#pragma unroll
            for (int i = 0; i < (8 + 2 * MASK_R) / 4; ++i) {
                const float4 f = *reinterpret_cast<const float4 *>(&yb[ty][cx + 4 * i]);
                v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
            }
            float m[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) m[k] = (float)tap_sum<MASK_R>([&](int j) { return (double)v[k + j]; }, taps.w);
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                if (c < C && ((chan_mask >> c) & 1u)) {
                    const uint16_t *ip = img + ((long)c * Zfull + zlo + z) * P + (long)gy * X + gx;
                    unsigned short pix[8];
                    if (gx + 8 <= X && (X & 7) == 0) {
                        const uint4 u = *reinterpret_cast<const uint4 *>(ip);
                        pix[0] = u.x & 0xffff; pix[1] = u.x >> 16; pix[2] = u.y & 0xffff; pix[3] = u.y >> 16;
                        pix[4] = u.z & 0xffff; pix[5] = u.z >> 16; pix[6] = u.w & 0xffff; pix[7] = u.w >> 16;
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) pix[k] = gx + k < X ? ip[k] : 0;
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float pr = airy_offset((float)pix[k], airy) * m[k];
                        mx[c][k] = pr > mx[c][k] ? pr : mx[c][k];
                    }
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C && ((chan_mask >> c) & 1u))
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (gx + k < X) proj[(long)c * P + (long)gy * X + gx + k] = (double)mx[c][k];
    }
}

static int cu_count()
{
    static int cus = 0;          // (same device model on every GPU of a node; a benign race writes the same value)
    if (!cus) {
        hipDeviceProp_t prop;
        cus = hipGetDeviceProperties(&prop, ctx().device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return cus;
}

// the float32 copy of n taps (a Taps' table or a caller's array) for the certified fast score passes; zero beyond n
static TapsF taps_f32(const double *w, int n)
{
    TapsF f;
    f.n = n;
    for (int i = 0; i < 256; ++i) f.w[i] = i < n ? (float)w[i] : 0.f;
    return f;
}

// The sigma-30 score pass of the certified argmax on the fp16 matrix cores with split operands (tip_corr_f16.h): radius 120
// (241 taps) only, data bounded by the clip value; err bit 8 (range_flag) reports a sample beyond that range.
template <int AXIS>
static int launch_f16(const float *in, float *out, int Zs, int Y, int X, const TapsF &t, const ClipInfo *clip, int *range_flag)
{
    if (t.n != 241 || !clip || !range_flag) return fail(TIP_ERR_ARG, "f16 score pass: %d taps (241 only) or no clip value / range flag", t.n);
    constexpr int R8 = 15, NPOS = HF_TO + 16 * R8, PITCH = ((NPOS / 8) | 1) * 8, WROWS = 2 * (R8 + 2) + 3;
    const size_t lds = (size_t)2 * HF_LN * PITCH * 2 + (size_t)2 * WROWS * 8 * 16;
    auto k = k_corr_long_f16<AXIS, R8>;
    static std::atomic<unsigned> attr_done[64];
    const int dev = ctx().device >= 0 && ctx().device < 64 ? ctx().device : 0;
    if (!(attr_done[dev].load(std::memory_order_acquire) & (1u << AXIS))) {
        TIP_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done[dev].fetch_or(1u << AXIS, std::memory_order_release);
    }
    const int tiles_ln = cdiv(AXIS == 1 ? X : Y, HF_LN), tiles_pos = cdiv(AXIS == 1 ? Y : X, HF_TO);
    if ((long)tiles_ln * tiles_pos > 0x7fffffffL || Zs > 65535) return fail(TIP_ERR_ARG, "f16 score pass: grid too large");
    const dim3 grid((unsigned)(tiles_ln * tiles_pos), (unsigned)Zs);
    const int xcd_bands = (AXIS == 2 && tiles_ln % 8 == 0) ? 1 : 0;
    TIP_LAUNCH(AXIS == 1 ? "score_fast_y" : "score_fast_x", k, grid, dim3(HF_NW * 64), lds, in, out, Zs, Y, X, t, &clip->p95, &clip->has, range_flag,
               tiles_ln, tiles_pos, xcd_bands);
    return TIP_OK;
}

// ---- certified argmax --------------------------------------------------------------------------------------------------
// The sigma-30 score is used for ONE thing: chosen_z = argmax_z(score) (sp.py:55-61).  So the score itself need not be
// exact -- only the argmax must be.  The fp16 score passes (k_corr_long_f16) give S~ with |S~ - S| <= EPS * S + ABS for the
// exact float32 score S.  By the bound in the header of tip_corr_f16.h (u = 2^-24, all samples and taps non-negative), each pass is
// within 38.2u relative (plus 2^-35 / s absolute) of the real-number sum and scipy's pass within 1.0001u of it; two passes compose
// to < 79u relative and < clip 2^-47 absolute.  EPS = 96u leaves 21 % headroom on the relative part.  (The uncertified pixels --
// and the cost of the exact fix-up -- scale with EPS.)
// A pixel is certified when its best fast score beats every other plane by more than both error bars; the few that
// are not (top two planes closer than ~1.2e-5 relative: the lines where the surface crosses between planes) are
// recomputed in exact scipy arithmetic from the z-passed volume, for the candidate planes only.
#define CERT_EPS (96.0f * 5.9604644775390625e-8f)
// ABS: the fp16 tiles keep 22 bits relative down to 2^-36 of the clip value and are off by at most clip 2^-47 below that
// (tip_corr_f16.h) -- clip 2^-44 here, a factor 8 of headroom
__device__ __forceinline__ float cert_abs(const ClipInfo *clip)
{
    return (clip && clip->has) ? clip->p95 * 5.684341886080802e-14f + 1e-30f : 1e-30f;
}

// four adjacent pixels per thread (one float4 per plane): enough bytes in flight to stream the score volume
__global__ void __launch_bounds__(256) k_argmax_certify(const float *__restrict__ score, int Z, long P, int *__restrict__ best_z,
                                                        int *__restrict__ unc_list, int *__restrict__ unc_count, const ClipInfo *clip)
{
    __shared__ int s_cnt[4], s_base;
    const float dabs = cert_abs(clip);
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const bool vec = p0 + 4 <= P && (P & 3) == 0;
    float b1[4], b2[4];
    int z1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { b1[k] = -1.f; b2[k] = -1.f; z1[k] = 0; }
    if (p0 < P) {
        for (int z = 0; z < Z; ++z) {
            float v[4];
            if (vec) {
                const float4 f = *reinterpret_cast<const float4 *>(score + (long)z * P + p0);
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = p0 + k < P ? score[(long)z * P + p0 + k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {   // scores are >= 0: the -1 start makes plane 0 the first maximum
                if (v[k] > b1[k]) { b2[k] = b1[k]; b1[k] = v[k]; z1[k] = z; }
                else if (v[k] > b2[k]) b2[k] = v[k];
            }
        }
    }
    unsigned unc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (p0 + k >= P) continue;
        best_z[p0 + k] = z1[k];
        // b1 == 0: every plane is exactly zero in the fast pass, hence (no underflow for uint16-derived data) in the exact one
        const bool certain = (b1[k] == 0.f) || (Z == 1) || (b1[k] * (1.f - CERT_EPS) - dabs > b2[k] * (1.f + CERT_EPS) + dabs);
        if (!certain) unc |= 1u << k;
    }
    // append with one atomic per block (not per pixel: same-address atomics serialise in L2)
    const int mine = __popc(unc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_inclusive_scan(mine);
    if (lane == 63) s_cnt[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        s_base = tot ? atomicAdd(unc_count, tot) : 0;
    }
    __syncthreads();
    if (mine) {
        int off = s_base + incl - mine;
        for (int w = 0; w < wave; ++w) off += s_cnt[w];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((unc >> k) & 1u) unc_list[off++] = (int)(p0 + k);
    }
}

constexpr int FIX_UL = 16;
__global__ void __launch_bounds__(256) k_argmax_exact_fix(const float *__restrict__ zvol, const float *__restrict__ score, int Z, int Y,
                                                          int X, Taps taps, const int *__restrict__ unc_list,
                                                          const int *__restrict__ unc_count, int *__restrict__ best_z, const ClipInfo *clip)
{
    const float dabs = cert_abs(clip);
    __shared__ float c[256];
    __shared__ float sfast[64];
    __shared__ float sexact[64];
    __shared__ int s_z;
    const int r = taps.n >> 1;  // 120
    // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  The list is in raster
    // order and neighbouring pixels read almost the same window of the volume, so every XCD gets one contiguous eighth
    // of the list instead of every eighth entry.
    const int total = *unc_count, xcd = blockIdx.x & 7, per = (total + 7) / 8;
    for (int sl = blockIdx.x >> 3; sl < per; sl += gridDim.x >> 3) {
        const int u = xcd * per + sl;
        if (u >= total) break;
        const int p = unc_list[u];
        const int y = p / X, x = p - y * X;
        const long P = (long)Y * X;
        if (threadIdx.x < Z) sfast[threadIdx.x] = score[(long)threadIdx.x * P + p];
        __syncthreads();
        float smax = sfast[0];
        for (int z = 1; z < Z; ++z) smax = fmaxf(smax, sfast[z]);
        const float thr = smax * (1.f - CERT_EPS) - dabs;
        for (int z = 0; z < Z; ++z) {
            const bool cand = sfast[z] * (1.f + CERT_EPS) + dabs >= thr;  // block-uniform
            if (!cand) { if (threadIdx.x == 0) sexact[z] = -1.f; continue; }
            const float *vol = zvol + (long)z * P;
            if (threadIdx.x < 2 * r + 1) {
                const int xx = clampi(x + (int)threadIdx.x - r, 0, X - 1);
                double tmp = (double)vol[(long)y * X + xx] * taps.w[r];
                // tap_sum's contract with the loads batched: the sum is serial (scipy's order) but the loads are not, 2 * FIX_UL per
                // trip in flight (the kernel is bound by global-load latency, not by arithmetic)
                for (int d0 = r; d0 >= 1; d0 -= FIX_UL) {
                    float a[FIX_UL], b[FIX_UL];
#pragma unroll
                    for (int u = 0; u < FIX_UL; ++u) {
                        const int d = max(d0 - u, 1);
                        a[u] = vol[(long)clampi(y - d, 0, Y - 1) * X + xx];
                        b[u] = vol[(long)clampi(y + d, 0, Y - 1) * X + xx];
                    }
#pragma unroll
                    for (int u = 0; u < FIX_UL; ++u)
                        if (d0 - u >= 1) tmp += ((double)a[u] + (double)b[u]) * taps.w[r - (d0 - u)];
                }
                c[threadIdx.x] = (float)tmp;   // exact y pass, rounded to float32 like scipy's intermediate
            }
            __syncthreads();
            if (threadIdx.x == 0) sexact[z] = (float)tap_sum(r, [&](int j) { return (double)c[j]; }, taps.w);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            float b = -2.f; int bz = 0;
            for (int z = 0; z < Z; ++z)
                if (sexact[z] > b) { b = sexact[z]; bz = z; }
            best_z[p] = bz;
        }
        __syncthreads();
    }
}

// writes the z-maps from the certified plane index (same outputs as k_argmax_z)
__global__ void __launch_bounds__(256) k_emit_zmaps(const int *__restrict__ best_z, int Z, long P, int min_z, int atoh_shift,
                                                    int32_t *__restrict__ zsel, int32_t *__restrict__ zsel_atoh,
                                                    int64_t *__restrict__ zmap, int *__restrict__ err)
{
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    emit_zmaps(p, best_z[p], Z, min_z, atoh_shift, zsel, zsel_atoh, zmap, err);
}

static int resolve_taps(const double *given, double sigma, int expect, Taps &t)
{
    double buf[256];
    if (!given) {
        int n = libm_taps(sigma, 4.0, buf, 255);
        if (n != expect) return fail(TIP_ERR_ARG, "internal: tap count %d != %d", n, expect);
        given = buf;
    }
    return make_taps(t, given, expect);
}

// build_continues_manifold on a device score (Zs, Y, X) -> plane index per pixel (int32, device); err bit 2: a pixel without
// a visited neighbour
static int manifold_dev(const float *score, int Zs, int Y, int X, int *bestz, int *err)
{
    Ctx &c = ctx();
    const long P = (long)Y * X, V = (long)Zs * P;
    if (V >= 0xffffffffL || Zs > 144 || Zs < 1) return fail(TIP_ERR_UNSUPPORTED, "build_manifold: stack too large");
    WsGuard ws;
    unsigned long long *key = ws.get<unsigned long long>(1);
    if (!key) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemsetAsync(key, 0, sizeof(unsigned long long), c.stream));
    TIP_HIP(hipMemsetAsync(bestz, 0xff, P * sizeof(int), c.stream));
    TIP_LAUNCH("argmax_first", k_argmax_first_f32, dim3((unsigned)std::min<long>(1024, cdiv(V, 256))), dim3(256), 0, score, V, key);
    int chunk = 1024;
    while (chunk > 64 && (size_t)4 * Zs * chunk > 150000) chunk >>= 1;
    const size_t lds = (size_t)4 * Zs * chunk;
    TIP_HIP(hipFuncSetAttribute((const void *)k_manifold, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TIP_LAUNCH("manifold", k_manifold, dim3(1), dim3(MAN_T), lds, score, Zs, Y, X, (const unsigned long long *)key, (volatile int *)bestz,
               chunk, err);
    return TIP_OK;
}

// ---- the host side: project_dev is a sequence of stages over one ProjJob ---------------------------------------------------
struct ProjJob {
    const uint16_t *czyx, *ref;     // the (C, Z, Y, X) stack; plane zlo of its reference channel
    int C, Z, Y, X, zlo, Zs;        // planes [zlo, zlo + Zs) take part
    long P, V;                      // Y * X, Zs * P
    int min_z, ref_ch, method, bin, airyscan, atoh_shift;   // method: without the manifold flag
    bool manifold;                  // sp.py:56-57: the spiral z-map instead of the argmax
    bool ref_unshifted;             // the reference channel takes the unshifted mask (false: ref_ch was given from the end)
    bool fast;                      // X % 4 == 0 and no TIP_PROJECT_GENERIC: the register-sliding / fused / fp16 kernels
    Taps k05, k1, k2, k30;
    WsGuard ws;                     // a tier takes the buffers only it uses from here
    float *A, *B;                   // two (Zs, Y, X) volumes
    unsigned long long *hist;
    ClipInfo *clip;
    int32_t *zsel, *zsel_a;         // chosen plane per pixel, as it is and atoh-shifted
    float *ident, *table;           // Zs x Zs: identity, and its z pass (the mask's z pass as a lookup)
    int *err;                       // bit 1 plane index beyond the stack, 2 manifold hole, 8 fp16 tile range
    double *proj;
    int64_t *zmap;
    hipStream_t stream;
};

static int check_args(const ProjJob &s, int zhi, bool tile)
{
    if (!s.czyx || !s.proj) return fail(TIP_ERR_ARG, "project: null pointer");
    if (s.C < 1 || s.C > 8) return fail(TIP_ERR_ARG, "project: 1..8 channels supported (got %d)", s.C);
    if (s.ref_ch < 0 || s.ref_ch >= s.C) return fail(TIP_ERR_INDEX, "project: reference_channel %d out of range", s.ref_ch);
    if (s.zlo < 0 || zhi > s.Z || zhi <= s.zlo) return fail(TIP_ERR_ARG, "project: bad z range [%d,%d) of %d", s.zlo, zhi, s.Z);
    if (s.Y < 1 || s.X < 1 || s.Y > 65535) return fail(TIP_ERR_ARG, "project: bad frame size %dx%d", s.Y, s.X);
    if (s.manifold && tile) return fail(TIP_ERR_UNSUPPORTED, "project: build_manifold takes whole frames");
    if (s.manifold && (s.V >= 0xffffffffL || s.Zs > 144)) return fail(TIP_ERR_UNSUPPORTED, "project: build_manifold: stack too large");
    return TIP_OK;
}

static int take_workspace(ProjJob &s)
{
    s.A = s.ws.get<float>(s.V), s.B = s.ws.get<float>(s.V);
    s.hist = s.ws.get<unsigned long long>(65536);
    s.clip = s.ws.get<ClipInfo>(1);
    s.zsel = s.ws.get<int32_t>(s.P), s.zsel_a = s.ws.get<int32_t>(s.P);
    s.ident = s.ws.get<float>((size_t)s.Zs * s.Zs), s.table = s.ws.get<float>((size_t)s.Zs * s.Zs);
    s.err = s.ws.get<int>(1);
    if (!s.A || !s.B || !s.hist || !s.clip || !s.zsel || !s.zsel_a || !s.ident || !s.table || !s.err) return TIP_ERR_NOMEM;
    return TIP_OK;
}

// P2: the clip value of one channel's planes (with_zero: see k_percentile95)
static int clip_of_channel(ProjJob &s, const uint16_t *src, int with_zero, ClipInfo *clip)
{
    TIP_HIP(hipMemsetAsync(s.hist, 0, 65536 * sizeof(unsigned long long), s.stream));
    TIP_LAUNCH("hist_u16", k_hist_u16, dim3((unsigned)std::min<long>(cdiv(s.V, HIST_PER_BLOCK), cu_count())), dim3(1024), 0, src, s.V,
               s.airyscan, s.hist);
    TIP_LAUNCH("percentile95", k_percentile95, dim3(1), dim3(1024), 0, (const unsigned long long *)s.hist, clip, with_zero);
    return TIP_OK;
}

// P3: (0.5, 1, 1) of the clipped channel -> A, then P4's z pass (0.5) of that -> B
static int short_blur(ProjJob &s, const uint16_t *src, ClipInfo *ci)
{
    const int Zs = s.Zs, Y = s.Y, X = s.X;
    if (s.fast && s.bin == 1 && !tuning().project_unfused_preblur) {
        // bin_size == 1 only needs the z-passed blur (B): the four short passes run as one kernel (tip_preblur.h)
        ShortTaps s05, s1;
        for (int i = 0; i < 8; ++i) { s05.w[i] = i < 3 ? s.k05.w[i] : 0.0; s1.w[i] = i < 5 ? s.k1.w[i] : 0.0; }
        TIP_LAUNCH("preblur_fused", k_preblur_fused, dim3(cdiv(X, PB_X), cdiv(Y, PB_Y)), dim3(PB_T), 0, src, s.airyscan,
                   (const float *)&ci->p95, (const int *)&ci->has, s.B, Zs, Y, X, s05, s1);
        return TIP_OK;
    }
    if (s.fast) {   // register-sliding kernels (each input loaded once per thread)
        Src4U16Clip su{src, s.airyscan, &ci->p95, &ci->has};
        TIP_LAUNCH("zpass_u16clip_x4", (k_zpass_r2_x4<Src4U16Clip>), dim3(cdiv(s.P / 4, 256)), dim3(256), 0, su, s.A, Zs, s.P, s.k05);
        // (36-row segments; 72-row segments halve the re-read halo rows but measured slower -- 0.257 against 0.235 ms --
        // and so did four columns per thread with 16-byte accesses: the pass wants many independent row streams)
        TIP_LAUNCH("ypass_slide_r4", (k_ypass_slide<float, 4, 4>), dim3(cdiv(X, 256), cdiv(Y, 36), Zs), dim3(256), 0,
                   (const float *)s.A, s.B, Y, X, s.k1);
        TIP_LAUNCH("xpass_slide_r4", (k_xpass_slide<float, 4>), dim3(cdiv(cdiv(X, 8), 256), Y, Zs), dim3(256), 0, (const float *)s.B,
                   s.A, Y, X, s.k1);
        Src4F32 sf{s.A};
        TIP_LAUNCH("zpass_f32_x4", (k_zpass_r2_x4<Src4F32>), dim3(cdiv(s.P / 4, 256)), dim3(256), 0, sf, s.B, Zs, s.P, s.k05);
        return TIP_OK;
    }
    LoadU16Clip ld{src, s.P, (long)X, s.airyscan, ci};
    dim3 grid(cdiv(X, 256), Y, Zs), block(256);
    TIP_LAUNCH("corr_z_u16clip", (k_corr_generic<float, 0, LoadU16Clip>), grid, block, 0, ld, s.A, Zs, Y, X, s.k05);
    int rc;
    if ((rc = correlate1d_dev(s.A, s.B, 0, Zs, Y, X, 1, s.k1, 0))) return rc;
    if ((rc = correlate1d_dev(s.B, s.A, 0, Zs, Y, X, 2, s.k1, 0))) return rc;
    return correlate1d_dev(s.A, s.B, 0, Zs, Y, X, 0, s.k05, 0);
}

// P4 in exact scipy arithmetic: the sigma-30 y and x passes of B, result in B (A is scratch)
static int score_exact(ProjJob &s)
{
    int rc;
    if ((rc = correlate1d_dev(s.B, s.A, 0, s.Zs, s.Y, s.X, 1, s.k30, 0))) return rc;
    return correlate1d_dev(s.A, s.B, 0, s.Zs, s.Y, s.X, 2, s.k30, 0);
}

static int emit_from_planes(ProjJob &s, const int *bestz, int min_z)
{
    TIP_LAUNCH("emit_zmaps", k_emit_zmaps, dim3(cdiv(s.P, 256)), dim3(256), 0, bestz, s.Zs, s.P, min_z, s.atoh_shift, s.zsel, s.zsel_a,
               s.zmap, s.err);
    return TIP_OK;
}

// P4' (sp.py:39-65): score on bin x bin blocks, resized back to the frame for the argmax
static int zmaps_binned(ProjJob &s)
{
    const int Zs = s.Zs, Y = s.Y, X = s.X, bin = s.bin, Yb = cdiv(Y, bin), Xb = cdiv(X, bin);
    const long nb = (long)Zs * Yb * Xb;
    float *S1 = s.ws.get<float>(nb);
    int *bestz = s.ws.get<int>(s.P);
    if (!S1 || !bestz) return TIP_ERR_NOMEM;
    int rc;
    if (s.method == 0) {          // max_averages: block mean of the (exact) (0.5, 30, 30) blur
        if ((rc = score_exact(s))) return rc;
        TIP_LAUNCH("block_mean", (k_block_reduce<false>), dim3(cdiv(nb, 256)), dim3(256), 0, (const float *)s.B, S1, Zs, Y, X, bin, Yb, Xb);
    } else {                      // max_std / multi_channel: block variance of the (0.5, 1, 1) blur
        TIP_LAUNCH("block_var", (k_block_reduce<true>), dim3(cdiv(nb, 256)), dim3(256), 0, (const float *)s.A, S1, Zs, Y, X, bin, Yb, Xb);
    }
    if (s.method == 2) {          // times the block mean of the next channel's (0.5, 30, 30) blur (sp.py:45-51)
        const uint16_t *other = s.czyx + ((long)((s.ref_ch + 1) % s.C) * s.Z + s.zlo) * s.P;
        float *S2 = s.ws.get<float>(nb);
        ClipInfo *clip2 = s.ws.get<ClipInfo>(1);
        if (!S2 || !clip2) return TIP_ERR_NOMEM;
        if ((rc = clip_of_channel(s, other, 1, clip2)) || (rc = short_blur(s, other, clip2)) || (rc = score_exact(s))) return rc;
        TIP_LAUNCH("block_mean", (k_block_reduce<false>), dim3(cdiv(nb, 256)), dim3(256), 0, (const float *)s.B, S2, Zs, Y, X, bin, Yb, Xb);
        TIP_LAUNCH("mul_f32", k_mul_f32, dim3(cdiv(nb, 256)), dim3(256), 0, S1, (const float *)S2, nb);
    }
    if (!s.manifold) {
        TIP_LAUNCH("resize_argmax", k_resize_argmax, dim3(cdiv(X, 256), Y), dim3(256), 0, (const float *)S1, Zs, Yb, Xb, Y, X, bestz);
        return emit_from_planes(s, bestz, s.min_z);
    }
    // sp.py:56-57, 63-65: the spiral on the BINNED score, then the plane maps resized to the frame and rounded
    int *bz = s.ws.get<int>((size_t)Yb * Xb);
    if (!bz) return TIP_ERR_NOMEM;
    if ((rc = manifold_dev((const float *)S1, Zs, Yb, Xb, bz, s.err))) return rc;
    TIP_LAUNCH("resize_round_zmaps", k_resize_round_zmaps, dim3(cdiv(X, 256), Y), dim3(256), 0, (const int *)bz, Yb, Xb, Y, X, Zs,
               s.atoh_shift, s.zsel, s.zsel_a, s.zmap, s.err);
    return TIP_OK;
}

// P4 + P5 with the certified argmax (see above): fp16 score, certify, exact fix-up of the uncertified pixels
static int zmaps_certified(ProjJob &s)
{
    const int Zs = s.Zs, Y = s.Y, X = s.X;
    const long P = s.P;
    float *D = s.ws.get<float>(s.V);
    int *bestz = s.ws.get<int>(P), *unc = s.ws.get<int>(P), *uncn = s.ws.get<int>(1);
    if (!D || !bestz || !unc || !uncn) return TIP_ERR_NOMEM;
    const TapsF f30 = taps_f32(s.k30.w, s.k30.n);
    // fast y pass B -> A, fast x pass A -> D   (B, the exact z-passed volume, is kept for the exact fix-up).  The fp16 tiles
    // take the clip value: their samples are scaled into fp16's range by it, and the volume B -- convex combinations of
    // clipped voxels -- is bounded by it; err bit 8 would report a sample beyond that range.
    int rc;
    if ((rc = launch_f16<1>((const float *)s.B, s.A, Zs, Y, X, f30, s.clip, s.err))) return rc;
    if ((rc = launch_f16<2>((const float *)s.A, D, Zs, Y, X, f30, s.clip, s.err))) return rc;
    TIP_HIP(hipMemsetAsync(uncn, 0, sizeof(int), s.stream));
    TIP_LAUNCH("argmax_certify", k_argmax_certify, dim3(cdiv(cdiv(P, 4), 256)), dim3(256), 0, (const float *)D, Zs, P, bestz, unc, uncn,
               (const ClipInfo *)s.clip);
    TIP_LAUNCH("argmax_exact_fix", k_argmax_exact_fix, dim3(8192), dim3(256), 0, (const float *)s.B, (const float *)D, Zs, Y, X,
               s.k30, (const int *)unc, (const int *)uncn, bestz, (const ClipInfo *)s.clip);
    if ((rc = emit_from_planes(s, bestz, s.min_z))) return rc;
    if (tuning().project_debug) {
        int hn = 0, he = 0;
        TIP_HIP(hipMemcpyAsync(&hn, uncn, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        TIP_HIP(hipMemcpyAsync(&he, s.err, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        TIP_HIP(hipStreamSynchronize(s.stream));
        fprintf(stderr, "certified argmax: %d of %ld pixels recomputed exactly\n", hn, P);
        if (he & 8) return fail(TIP_ERR_HIP, "score pass: a sample beyond the clip value's range reached the fp16 tiles");
    }
    return TIP_OK;
}

// P4 + P5 at full resolution: (0.5, 30, 30) score and its argmax
static int zmaps_full(ProjJob &s)
{
    if (s.fast && s.Zs <= 64 && !s.manifold && !tuning().project_exact_score) return zmaps_certified(s);
    int rc;
    if ((rc = score_exact(s))) return rc;
    if (!s.manifold) {   // P5
        TIP_LAUNCH("argmax_z", k_argmax_z, dim3(cdiv(s.P, 256)), dim3(256), 0, s.B, s.Zs, s.P, s.min_z, s.atoh_shift, s.zsel, s.zsel_a,
                   s.zmap, s.err);
        return TIP_OK;
    }
    // the spiral reads score VALUES (window argmaxes), so it gets the exact score; min_z is not added (sp.py:57)
    int *bestz = s.ws.get<int>(s.P);
    if (!bestz) return TIP_ERR_NOMEM;
    if ((rc = manifold_dev((const float *)s.B, s.Zs, s.Y, s.X, bestz, s.err))) return rc;
    return emit_from_planes(s, bestz, 0);
}

// (instantiated per channel count: the per-channel running maxima are registers, 8 channels' worth of them cost the
//  two-channel case a third of its occupancy)
template <int MAXC>
static int launch_mask_fused(const ProjJob &s, const int32_t *sel, unsigned cm)
{
    TIP_LAUNCH("mask_wmax_fused", (k_mask_wmax_fused<MAXC>), dim3(cdiv(s.X, FT_X), cdiv(s.Y, FT_Y)), dim3(256),
               (size_t)s.Zs * s.Zs * sizeof(float), (const float *)s.table, sel, s.czyx, s.C, s.Z, s.zlo, s.Zs, s.Y, s.X, s.airyscan, cm,
               s.k2, s.proj);
    return TIP_OK;
}

// P6-P8: one pass over all channels, or (atoh_shift != 0, sp.py:75-79) the reference channel under the chosen planes and
// the others under the shifted ones
static int mask_and_project(ProjJob &s)
{
    const int Zs = s.Zs, Y = s.Y, X = s.X, C = s.C;
    // P6/P7 z pass as a Zs x Zs table (sigma 1 -> 9 taps), built with the same correlate kernel
    TIP_LAUNCH("identity", k_identity, dim3(cdiv((long)Zs * Zs, 256)), dim3(256), 0, s.ident, Zs);
    int rc;
    if ((rc = correlate1d_dev(s.ident, s.table, 0, Zs, Zs, 1, 0, s.k1, 1))) return rc;
    const bool fused = s.fast && Zs <= 64 && !tuning().project_unfused_mask;
    const unsigned all = (1u << C) - 1u;
    for (int pass = 0; pass < (s.atoh_shift != 0 ? 2 : 1); ++pass) {
        const int32_t *sel = pass == 0 ? s.zsel : s.zsel_a;
        const unsigned refbit = s.ref_unshifted ? (1u << s.ref_ch) : 0u;
        const unsigned cm = s.atoh_shift == 0 ? all : (pass == 0 ? refbit : (all & ~refbit));
        if (!cm) continue;
        if (fused) {
            rc = C <= 2 ? launch_mask_fused<2>(s, sel, cm) : C <= 4 ? launch_mask_fused<4>(s, sel, cm) : launch_mask_fused<8>(s, sel, cm);
            if (rc) return rc;
            continue;
        }
        // the dense form in literal scipy order (X % 4 != 0, Zs > 64, TIP_PROJECT_GENERIC, TIP_PROJECT_UNFUSED_MASK)
        LoadMaskTable ld{s.table, sel, Zs, (long)X};
        dim3 grid(cdiv(X, 256), Y, Zs), block(256);
        TIP_LAUNCH("mask_ypass", (k_corr_generic<float, 1, LoadMaskTable>), grid, block, 0, ld, s.A, Zs, Y, X, s.k2);
        TIP_LAUNCH("xpass_wmax", (k_xpass_wmax<8>), dim3(cdiv(X, 256), Y), dim3(256), 0, s.A, s.czyx, C, s.Z, s.zlo, Zs, Y, X, s.airyscan,
                   cm, s.k2, s.proj);
    }
    return TIP_OK;
}

// the read-back costs a synchronise: only for the arguments that can raise err bit 1 or 2
static int read_err(ProjJob &s)
{
    if (!(s.min_z > 0 || s.atoh_shift > 0 || s.manifold)) return TIP_OK;
    int h = 0;
    TIP_HIP(hipMemcpyAsync(&h, s.err, sizeof(int), hipMemcpyDeviceToHost, s.stream));
    TIP_HIP(hipStreamSynchronize(s.stream));
    if (h & 2) return fail(TIP_ERR_HIP, "build_manifold: a pixel without a visited neighbour (upstream raises TypeError here)");
    if (h & 8) return fail(TIP_ERR_HIP, "score pass: a sample beyond the clip value's range reached the fp16 tiles");
    if (h)
        return fail(TIP_ERR_INDEX, "chosen z index out of bounds for the %d-plane mask (min_z=%d, atoh_shift=%d): "
                                   "the reference raises IndexError here (sp.py:62,68-69)", s.Zs, s.min_z, s.atoh_shift);
    return TIP_OK;
}

int project_dev(const uint16_t *czyx, int C, int Z, int Y, int X, int zlo, int zhi, int min_z, int ref_ch, int method, int bin,
                int airyscan, int atoh_shift, const double *t05, const double *t1, const double *t2,
                const double *t30, double *proj, int64_t *zmap, const unsigned long long *hist_in = nullptr)
{
    ProjJob s;
    s.stream = ctx().stream;
    if (!s.stream) return TIP_ERR_HIP;
    s.czyx = czyx; s.C = C; s.Z = Z; s.Y = Y; s.X = X; s.zlo = zlo; s.Zs = zhi - zlo;
    s.P = (long)Y * X; s.V = (long)s.Zs * s.P;
    // ref_ch in [-C, 0) counts from the end, as numpy's image[reference_channel] does (sp.py:32) -- and sp.py:76 then compares
    // the channel NUMBER with it, which never matches: every channel, the reference included, takes the shifted mask
    s.ref_unshifted = ref_ch >= 0;
    if (ref_ch < 0 && C > 0) ref_ch += C;
    s.min_z = min_z; s.ref_ch = ref_ch; s.bin = bin; s.airyscan = airyscan; s.atoh_shift = atoh_shift;
    s.manifold = (method & TIP_PROJECT_MANIFOLD) != 0;
    s.method = method & ~TIP_PROJECT_MANIFOLD;
    s.fast = (X % 4 == 0) && !tuning().project_generic;
    s.proj = proj; s.zmap = zmap;
    int rc;
    if ((rc = check_args(s, zhi, hist_in != nullptr)) || (rc = resolve_taps(t05, 0.5, 5, s.k05)) || (rc = resolve_taps(t1, 1.0, 9, s.k1)) ||
        (rc = resolve_taps(t2, 2.0, 17, s.k2)) || (rc = resolve_taps(t30, 30.0, 241, s.k30)) || (rc = take_workspace(s)))
        return rc;
    s.ref = czyx + ((long)ref_ch * Z + zlo) * s.P;
    TIP_HIP(hipMemsetAsync(s.err, 0, sizeof(int), s.stream));
    if (hist_in) {   // a tile of a larger frame: the caller brings the whole frame's histogram
        if (bin > 1 && s.method == 2) return fail(TIP_ERR_UNSUPPORTED, "project: tiles with method multi_channel");
        TIP_LAUNCH("percentile95", k_percentile95, dim3(1), dim3(1024), 0, hist_in, s.clip, 0);
    } else if ((rc = clip_of_channel(s, s.ref, 0, s.clip))) return rc;
    if ((rc = short_blur(s, s.ref, s.clip))) return rc;
    if ((rc = bin > 1 ? zmaps_binned(s) : zmaps_full(s))) return rc;
    if ((rc = mask_and_project(s))) return rc;
    return read_err(s);
}

}  // namespace tip

using namespace tip;

extern "C" {

static int project_host(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z, int ref_ch, int method,
                        int bin, int airyscan, int atoh_shift, const double *t05, const double *t1, const double *t2,
                        const double *t30, double *proj, int64_t *zmap)
{
    if (!ctx().stream) return TIP_ERR_HIP;
    if (!czyx || !proj) return fail(TIP_ERR_ARG, "tip_project_u16: null pointer");
    if (c < 1 || z < 1 || y < 1 || x < 1) return fail(TIP_ERR_ARG, "tip_project_u16: empty stack");
    const size_t nin = (size_t)c * z * y * x, P = (size_t)y * x;
    Staging st;
    const uint16_t *din = st.in(czyx, nin);
    double *dproj = st.out(proj, (size_t)c * P);
    int64_t *dz = st.out(zmap, P);       // (no zmap asked for: none computed, none copied)
    if (st.rc) return st.rc;
    int rc = project_dev(din, c, z, y, x, zlo, zhi, min_z, ref_ch, method, bin, airyscan, atoh_shift, t05, t1, t2, t30, dproj, dz);
    if (rc) return rc;
    return st.finish();
}

static int check_binned(int method, int bin)
{
    if (method >= 0) method &= ~TIP_PROJECT_MANIFOLD;   // a flag on top of the method, not a method (negative: reported as given)
    if (method < 0 || method > 2) return fail(TIP_ERR_ARG, "projection: method %d (0 max_averages, 1 max_std, 2 multi_channel)", method);
    if (bin < 1 || bin > 128) return fail(TIP_ERR_UNSUPPORTED, "projection: bin_size %d (1..128 supported)", bin);
    return TIP_OK;
}

int tip_project_u16_dev(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z, int ref_ch,
                        int airyscan, int atoh_shift, const double *t05, const double *t1, const double *t2,
                        const double *t30, double *proj, int64_t *zmap)
{
    return project_dev(czyx, c, z, y, x, zlo, zhi, min_z, ref_ch, 0, 1, airyscan, atoh_shift, t05, t1, t2, t30, proj, zmap);
}

int tip_project_u16(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z, int ref_ch,
                    int airyscan, int atoh_shift, const double *t05, const double *t1, const double *t2,
                    const double *t30, double *proj, int64_t *zmap)
{
    return project_host(czyx, c, z, y, x, zlo, zhi, min_z, ref_ch, 0, 1, airyscan, atoh_shift, t05, t1, t2, t30, proj, zmap);
}

int tip_hist_u16_box_dev(const uint16_t *czyx, int c, int z, int y, int x, int ch, int z0, int z1, int y0, int y1, int x0, int x1,
                         int airyscan, unsigned long long *hist_dev)
{
    Ctx &cx = ctx();
    if (!cx.stream) return TIP_ERR_HIP;
    if (!czyx || !hist_dev) return fail(TIP_ERR_ARG, "tip_hist_u16_box_dev: null pointer");
    if (ch < 0 || ch >= c || z0 < 0 || z1 > z || z1 <= z0 || y0 < 0 || y1 > y || y1 <= y0 || x0 < 0 || x1 > x || x1 <= x0)
        return fail(TIP_ERR_ARG, "tip_hist_u16_box_dev: box outside the (%d,%d,%d,%d) stack", c, z, y, x);
    const long n = (long)(z1 - z0) * (y1 - y0) * (x1 - x0);
    const uint16_t *plane = czyx + (long)ch * z * y * x;
    TIP_LAUNCH("hist_u16_box", k_hist_u16_box, dim3(cdiv(n, HIST_PER_BLOCK)), dim3(1024), 0, plane, y, x, z0, y0, x0, z1 - z0, y1 - y0,
               x1 - x0, airyscan, hist_dev);
    return TIP_OK;
}

int tip_project_u16_hist_dev(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z, int ref_ch,
                             int airyscan, int atoh_shift, const double *t05, const double *t1, const double *t2,
                             const double *t30, const unsigned long long *hist_dev, double *proj, int64_t *zmap)
{
    if (!hist_dev) return fail(TIP_ERR_ARG, "tip_project_u16_hist_dev: null histogram");
    return project_dev(czyx, c, z, y, x, zlo, zhi, min_z, ref_ch, 0, 1, airyscan, atoh_shift, t05, t1, t2, t30, proj, zmap, hist_dev);
}

int tip_project_u16_binned_dev(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z, int ref_ch,
                               int method, int bin_size, int airyscan, int atoh_shift, const double *t05, const double *t1,
                               const double *t2, const double *t30, double *proj, int64_t *zmap)
{
    int rc = check_binned(method, bin_size);
    if (rc) return rc;
    return project_dev(czyx, c, z, y, x, zlo, zhi, min_z, ref_ch, method, bin_size, airyscan, atoh_shift, t05, t1, t2, t30, proj, zmap);
}

int tip_project_u16_binned(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z, int ref_ch,
                           int method, int bin_size, int airyscan, int atoh_shift, const double *t05, const double *t1,
                           const double *t2, const double *t30, double *proj, int64_t *zmap)
{
    int rc = check_binned(method, bin_size);
    if (rc) return rc;
    return project_host(czyx, c, z, y, x, zlo, zhi, min_z, ref_ch, method, bin_size, airyscan, atoh_shift, t05, t1, t2, t30, proj, zmap);
}

// ---- diagnostics of the fp16 score tiles (tests) ---------------------------------------------------------------------------------
__global__ void k_set_clip(ClipInfo *c, float v) { c->has = 1; c->p95 = v; c->p95d = (double)v; }

// one sigma-30 pass of tip_corr_f16.h on HOST float32 volumes (z, y, x): axis 1 = along y, 2 = along x; taps = 241 symmetric float64
// weights (radius 120); clip = the bound of the data (the scaling follows from it).  flag: bit 8 = a sample beyond the range.
int tip_score_pass_f16(const float *in, float *out, int z, int y, int x, int axis, const double *taps, int ntaps, float clip, int *flag)
{
    if (!ctx().stream) return TIP_ERR_HIP;
    if (!in || !out || !taps || !flag || z < 1 || y < 1 || x < 1 || (axis != 1 && axis != 2) || ntaps != 241 || !(clip > 0.f))
        return fail(TIP_ERR_ARG, "tip_score_pass_f16: bad arguments (radius 120 only)");
    const size_t V = (size_t)z * y * x;
    Staging st;
    const float *di = st.in(in, V);
    float *dout = st.out(out, V);
    ClipInfo *ci = st.scratch<ClipInfo>(1);
    int *df = st.out(flag, 1, true);
    if (st.rc) return st.rc;
    const TapsF t = taps_f32(taps, ntaps);
    hipLaunchKernelGGL(k_set_clip, dim3(1), dim3(1), 0, ctx().stream, ci, clip);
    int rc = with_axis<1>(axis, [&](auto A) { return launch_f16<decltype(A)::value>(di, dout, z, y, x, t, ci, df); });
    if (rc) return rc;
    return st.finish();
}

// How v_mfma_f32_32x32x16_f16 rounds, on THIS device (the certified bound of tip_corr_f16.h counts two roundings per instruction:
// the sixteen products enter the accumulator as two exactly-summed halves).  Every row of A / column of B is the same; case t has
// C = c[t] and product k = a[t][k] b[t][k]; out[t] = any output element.
__global__ void k_mfma_f16_probe(const float *a, const float *b, const float *c, float *out, int ncase)
{
    const int h = threadIdx.x >> 5;
    for (int t = 0; t < ncase; ++t) {
        f16x8 fa, fb;
        for (int e = 0; e < 8; ++e) { fa[e] = (_Float16)a[t * 16 + 8 * h + e]; fb[e] = (_Float16)b[t * 16 + 8 * h + e]; }
        f32x16 acc;
        for (int q = 0; q < 16; ++q) acc[q] = c[t];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc, 0, 0, 0);
        if (threadIdx.x == 0) out[t] = acc[0];
    }
}
int tip_mfma_f16_probe(const float *a, const float *b, const float *cvals, float *out, int ncase)
{
    if (!ctx().stream) return TIP_ERR_HIP;
    if (!a || !b || !cvals || !out || ncase < 1 || ncase > 256) return fail(TIP_ERR_ARG, "tip_mfma_f16_probe: bad arguments");
    Staging st;
    const float *da = st.in(a, (size_t)ncase * 16), *db = st.in(b, (size_t)ncase * 16), *dc = st.in(cvals, (size_t)ncase);
    float *dout = st.out(out, (size_t)ncase);
    if (st.rc) return st.rc;
    hipLaunchKernelGGL(k_mfma_f16_probe, dim3(1), dim3(64), 0, ctx().stream, da, db, dc, dout, ncase);
    return st.finish();
}

// sp.py:87-165 on its own: score float32 (z, y, x) host -> int64 (y, x) plane map
int tip_build_manifold_f32(const float *score, int z, int y, int x, int64_t *chosen)
{
    if (!ctx().stream) return TIP_ERR_HIP;
    if (!score || !chosen || z < 1 || y < 1 || x < 1) return fail(TIP_ERR_ARG, "tip_build_manifold_f32: bad arguments");
    const size_t P = (size_t)y * x, V = P * z;
    std::vector<int> hb(P);          // the int32 plane map and the error word come down first: `chosen` is written last
    int herr = 0;
    Staging st;
    const float *ds = st.in(score, V);
    int *bz = st.out(hb.data(), P), *err = st.out(&herr, 1, true);
    if (st.rc) return st.rc;
    int rc = manifold_dev(ds, z, y, x, bz, err);
    if (rc) return rc;
    if ((rc = st.finish())) return rc;
    if (herr) return fail(TIP_ERR_HIP, "build_manifold: a pixel without a visited neighbour (upstream raises TypeError here)");
    for (size_t i = 0; i < P; ++i) chosen[i] = hb[i];
    return TIP_OK;
}

}  // extern "C"
