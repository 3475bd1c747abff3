// tip_export.hip -- a frame's resident maps as the uint16 pages of Tissue.export_segmentation_and_cell_types_to_tiff (ti.py:4040-4052):
// plane 0 the tracking labels -- get_trackking_labels' ids[labels - 1], 0 on label 0, cast to uint16 --, plane 1 the type map with
// 0 -> 2 and 255 -> 0.  The pages stay on the device: tip_deflate_strips_dev takes them from here (movie.export_tiff).
//
// k_export_maps_u16: one thread per four pixels -- one 16-byte load of labels, one 4-byte load of types, one 8-byte store per
// plane -- when the pixel count and the addresses allow it, one pixel per thread otherwise.  The ids are a uint16 table of a few
// kilobytes that every wave reads from cache.  A label outside [0, n_ids] becomes 0 and is counted: one sum per wave, and one
// atomic add by the wave's first lane only when the wave saw any.
//
// The projected movie (movie.export_projection): a frame's resident float64 projection planes as the uint16 pages
// save_tiff(..., data_type="uint16") writes (bim.py:183-186), and its int64 z-map as uint16 (sp.py:229-230).
//
// page_sample is the rounding contract, one function for the device kernels and their host twins: u = (uint16) rint((v / m) * 65535)
// with the division and the product rounded separately, to nearest -- the explicit _rn intrinsics on the device, plain operators
// under -ffp-contract=off on the host; no reciprocal, no fused step.  m is the WHOLE movie's maximum (tip_max_f64_dev per frame, the
// maximum of those on the host).  k_projection_pages_u16 is memory-bound, 8 bytes in and 2 out per sample: a thread takes four
// consecutive samples of the flat array -- two 16-byte loads, one 8-byte store -- and what n / 4 leaves over goes one sample per
// thread; so do all samples when an address is not aligned.  Predictor 2 (TIFF horizontal differencing) stores u[x] - u[x - 1]
// modulo 2^16: the thread converts its left neighbour's sample again (one more 8-byte load, a cache hit) instead of a second pass.
#include "tip_internal.h"
#include <cmath>

namespace tip {

// Out of [0, m] the cast goes through int64 and wraps modulo 2^16, as numpy's astype does on x86-64; a NaN, and a quotient no int64
// holds, give 0 on both sides (numpy: the low bits of INT64_MIN).  m == 0: an all-zero movie, 0 / 0 -> NaN -> 0 in numpy.
__host__ __device__ static inline uint16_t page_sample(double v, double m)
{
    if (m == 0.0) return 0;
#ifdef __HIP_DEVICE_COMPILE__
    const double q = rint(__dmul_rn(__ddiv_rn(v, m), 65535.0));
#else
    const double q = rint((v / m) * 65535.0);
#endif
    if (!(q > -9.0e18 && q < 9.0e18)) return 0;
    return (uint16_t)(long long)q;
}

// sample i of pages whose rows hold `cols` samples, as the page stores it under `predictor`
__host__ __device__ static inline uint16_t page_value(const double *__restrict__ src, long i, long cols, double m, int predictor)
{
    const uint16_t u = page_sample(src[i], m);
    return predictor == 2 && i % cols ? (uint16_t)(u - page_sample(src[i - 1], m)) : u;
}

__host__ __device__ static inline double max_f64(double a, double b) { return b > a ? b : a; }      // (a NaN is never taken)

__host__ __device__ static inline uint16_t zmap_sample(int64_t z) { return (uint16_t)(uint64_t)z; }

// groups of V samples from sample `first` on: V == 4 needs src + first on 16 bytes and out + first on 8
template <int V, int PRED>
__global__ __launch_bounds__(256) void k_projection_pages_u16(const double *__restrict__ src, long first, long groups, long cols, double m,
                                                              uint16_t *__restrict__ out)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const long i = first + g * V;
    if constexpr (V == 4) {
        const double2 a = *(const double2 *)(src + i), b = *(const double2 *)(src + i + 2);
        uint32_t u0 = page_sample(a.x, m), u1 = page_sample(a.y, m), u2 = page_sample(b.x, m), u3 = page_sample(b.y, m);
        if constexpr (PRED == 2) {
            // x of the group's first sample: 32-bit arithmetic while the flat index fits
            const uint32_t x = (uint64_t)(i + 3) <= 0xFFFFFFFFull ? (uint32_t)i % (uint32_t)cols : (uint32_t)(i % cols), c = (uint32_t)cols;
            const uint32_t left = x ? page_sample(src[i - 1], m) : 0u;
            const uint32_t d3 = (x + 3) % c ? u3 - u2 : u3, d2 = (x + 2) % c ? u2 - u1 : u2, d1 = (x + 1) % c ? u1 - u0 : u1;
            u0 = x ? u0 - left : u0, u1 = d1, u2 = d2, u3 = d3;
        }
        uint2 o;
        o.x = (u0 & 0xFFFFu) | u1 << 16;
        o.y = (u2 & 0xFFFFu) | u3 << 16;
        *(uint2 *)(out + i) = o;
    } else {
        out[i] = page_value(src, i, cols, m, PRED);
    }
}

constexpr int MAX_BLOCKS = 1024;      // partial maxima of tip_max_f64_dev: one per workgroup, folded on the host

__global__ __launch_bounds__(256) void k_max_f64(const double *__restrict__ src, long n, double *__restrict__ partial)
{
    __shared__ double wave_vals[4];
    double v = -INFINITY;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) v = max_f64(v, src[i]);
    v = block_reduce<4>(v, wave_vals, [](double a, double b) { return max_f64(a, b); });
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

template <int V>
__global__ __launch_bounds__(256) void k_zmap_u16(const int64_t *__restrict__ src, long first, long groups, uint16_t *__restrict__ out)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const long i = first + g * V;
    if constexpr (V == 4) {
        const longlong2 a = *(const longlong2 *)(src + i), b = *(const longlong2 *)(src + i + 2);
        uint2 o;
        o.x = (uint32_t)zmap_sample(a.x) | (uint32_t)zmap_sample(a.y) << 16;
        o.y = (uint32_t)zmap_sample(b.x) | (uint32_t)zmap_sample(b.y) << 16;
        *(uint2 *)(out + i) = o;
    } else {
        out[i] = zmap_sample(src[i]);
    }
}

// the split of n samples into groups of four and a tail of single samples; 0 fours when an address does not allow them
static inline long fours_of(long n, const void *src, const void *out) { return ((uintptr_t)src & 15u) || ((uintptr_t)out & 7u) ? 0 : n / 4; }

static int check_pages(const char *who, const void *src, int64_t n_pages, int64_t rows, int64_t cols, double m, int predictor, const void *out)
{
    if (!src || !out) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (n_pages < 0 || rows < 0 || cols < 0 || cols > 0x7FFFFFFFL || (double)n_pages * (double)rows * (double)cols > 1.0e12)
        return fail(TIP_ERR_ARG, "%s: %ld pages of %ld x %ld", who, (long)n_pages, (long)rows, (long)cols);
    if (!(m >= 0.0) || std::isinf(m)) return fail(TIP_ERR_ARG, "%s: scale_max %g (the movie's maximum: finite, not negative)", who, m);
    if (predictor != 1 && predictor != 2) return fail(TIP_ERR_UNSUPPORTED, "%s: predictor %d (1: none, 2: horizontal differencing)", who, predictor);
    return TIP_OK;
}

__device__ static inline uint32_t export_label(int32_t l, const uint16_t *__restrict__ ids, int n_ids, int &bad)
{
    if (l < 0 || l > n_ids) { ++bad; return 0u; }
    return l ? (uint32_t)ids[l - 1] : 0u;
}

__device__ static inline uint32_t export_type(uint32_t t) { return t == 0u ? 2u : t == 255u ? 0u : t; }

template <int V>      // V pixels per thread: 4 (aligned, n a multiple of 4) or 1
__global__ __launch_bounds__(256) void k_export_maps_u16(const int32_t *__restrict__ labels, const uint8_t *__restrict__ types, long n,
                                                         const uint16_t *__restrict__ ids, int n_ids, uint16_t *__restrict__ out,
                                                         unsigned *__restrict__ n_bad)
{
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    int bad = 0;
    if (i < n) {
        if constexpr (V == 4) {
            const int4 l = *(const int4 *)(labels + i);
            uint2 o;
            o.x = export_label(l.x, ids, n_ids, bad) | export_label(l.y, ids, n_ids, bad) << 16;
            o.y = export_label(l.z, ids, n_ids, bad) | export_label(l.w, ids, n_ids, bad) << 16;
            *(uint2 *)(out + i) = o;
            if (types) {
                const uint32_t t = *(const uint32_t *)(types + i);
                uint2 p;
                p.x = export_type(t & 255u) | export_type((t >> 8) & 255u) << 16;
                p.y = export_type((t >> 16) & 255u) | export_type(t >> 24) << 16;
                *(uint2 *)(out + n + i) = p;
            }
        } else {
            out[i] = (uint16_t)export_label(labels[i], ids, n_ids, bad);
            if (types) out[n + i] = (uint16_t)export_type(types[i]);
        }
    }
    bad = wave_sum(bad);
    if (bad && (threadIdx.x & 63u) == 0) atomicAdd(n_bad, (unsigned)bad);
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_export_maps_u16_dev(const int32_t *labels_dev, const uint8_t *types_dev, int64_t n_pix, const int64_t *ids_host, int64_t n_ids,
                            uint16_t *out_dev, int32_t *n_bad_host)
{
    const char *who = "tip_export_maps_u16_dev";
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!labels_dev || !out_dev || !n_bad_host || (n_ids > 0 && !ids_host)) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (n_pix < 0 || n_ids < 0 || n_ids > 0x7FFFFFFFL) return fail(TIP_ERR_ARG, "%s: %ld pixels, %ld ids", who, (long)n_pix, (long)n_ids);
    for (long k = 0; k < n_ids; ++k)
        if (ids_host[k] < 0 || ids_host[k] > 65535)
            return fail(TIP_ERR_ARG, "%s: id %ld of row %ld does not fit a uint16 page", who, (long)ids_host[k], k);
    *n_bad_host = 0;
    if (n_pix == 0) return TIP_OK;
    const long blocks4 = (n_pix / 4 + 255) / 256, blocks1 = (n_pix + 255) / 256;
    if (blocks1 > 0x7FFFFFFFL) return fail(TIP_ERR_ARG, "%s: %ld pixels (at most 2^39 - 256)", who, (long)n_pix);
    WsGuard ws;
    uint16_t *ids = ws.get<uint16_t>((size_t)n_ids);
    unsigned *bad = ws.get<unsigned>(1);
    const size_t ids_room = ((size_t)n_ids * 2 + 7) & ~(size_t)7;      // the pinned block: the ids, then the count's word
    uint8_t *pin = (uint8_t *)pinned_scratch(ids_room + 8);
    if (!ids || !bad || !pin) return TIP_ERR_NOMEM;
    for (long k = 0; k < n_ids; ++k) ((uint16_t *)pin)[k] = (uint16_t)ids_host[k];
    if (n_ids) TIP_HIP(hipMemcpyAsync(ids, pin, (size_t)n_ids * 2, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemsetAsync(bad, 0, 4, c.stream));
    const bool wide = n_pix % 4 == 0 && ((uintptr_t)labels_dev & 15u) == 0 && ((uintptr_t)out_dev & 7u) == 0 && ((uintptr_t)types_dev & 3u) == 0;
    if (wide)
        TIP_LAUNCH("export_maps_u16", k_export_maps_u16<4>, dim3((unsigned)blocks4), dim3(256), 0, labels_dev, types_dev, (long)n_pix, ids,
                   (int)n_ids, out_dev, bad);
    else
        TIP_LAUNCH("export_maps_u16", k_export_maps_u16<1>, dim3((unsigned)blocks1), dim3(256), 0, labels_dev, types_dev, (long)n_pix, ids,
                   (int)n_ids, out_dev, bad);
    TIP_HIP(hipMemcpyAsync(pin + ids_room, bad, 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    *n_bad_host = (int32_t) * (unsigned *)(pin + ids_room);
    return TIP_OK;
}

int tip_max_f64_dev(const double *src_dev, int64_t n, double *max_host)
{
    const char *who = "tip_max_f64_dev";
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!src_dev || !max_host) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (n < 1) return fail(TIP_ERR_ARG, "%s: %ld values (at least one)", who, (long)n);
    const int blocks = (int)std::min<long>(MAX_BLOCKS, (n + 2047) / 2048);      // at least eight loads a thread before the reduction
    WsGuard ws;
    double *partial = ws.get<double>(MAX_BLOCKS);
    double *pin = (double *)pinned_scratch(MAX_BLOCKS * sizeof(double));
    if (!partial || !pin) return TIP_ERR_NOMEM;
    TIP_LAUNCH("max_f64", k_max_f64, dim3((unsigned)blocks), dim3(256), 0, src_dev, (long)n, partial);
    TIP_HIP(hipMemcpyAsync(pin, partial, (size_t)blocks * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    double m = pin[0];
    for (int b = 1; b < blocks; ++b) m = max_f64(m, pin[b]);
    *max_host = m;
    return TIP_OK;
}

int tip_max_f64(const double *src, int64_t n, double *max_out)
{
    if (!src || !max_out) return fail(TIP_ERR_ARG, "tip_max_f64: null pointer");
    if (n < 1) return fail(TIP_ERR_ARG, "tip_max_f64: %ld values (at least one)", (long)n);
    double m = -INFINITY;
    for (long i = 0; i < n; ++i) m = max_f64(m, src[i]);
    *max_out = m;
    return TIP_OK;
}

int tip_projection_pages_u16_dev(const double *src_dev, int64_t n_pages, int64_t rows, int64_t cols, double scale_max, int predictor,
                                 uint16_t *out_dev)
{
    const char *who = "tip_projection_pages_u16_dev";
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_pages(who, src_dev, n_pages, rows, cols, scale_max, predictor, out_dev)) return rc;
    const long n = n_pages * rows * cols;
    if (n == 0) return TIP_OK;
    const long fours = fours_of(n, src_dev, out_dev), tail = n - 4 * fours;
    if (fours) {
        const dim3 grid((unsigned)((fours + 255) / 256));
        if (predictor == 2)
            TIP_LAUNCH("projection_pages_u16", (k_projection_pages_u16<4, 2>), grid, dim3(256), 0, src_dev, 0L, fours, (long)cols, scale_max, out_dev);
        else
            TIP_LAUNCH("projection_pages_u16", (k_projection_pages_u16<4, 1>), grid, dim3(256), 0, src_dev, 0L, fours, (long)cols, scale_max, out_dev);
    }
    if (tail) {
        const dim3 grid((unsigned)((tail + 255) / 256));
        if (predictor == 2)
            TIP_LAUNCH("projection_pages_u16", (k_projection_pages_u16<1, 2>), grid, dim3(256), 0, src_dev, 4 * fours, tail, (long)cols, scale_max, out_dev);
        else
            TIP_LAUNCH("projection_pages_u16", (k_projection_pages_u16<1, 1>), grid, dim3(256), 0, src_dev, 4 * fours, tail, (long)cols, scale_max, out_dev);
    }
    return TIP_OK;
}

int tip_projection_pages_u16(const double *src, int64_t n_pages, int64_t rows, int64_t cols, double scale_max, int predictor, uint16_t *out)
{
    if (int rc = check_pages("tip_projection_pages_u16", src, n_pages, rows, cols, scale_max, predictor, out)) return rc;
    const long n = n_pages * rows * cols;
    for (long i = 0; i < n; ++i) out[i] = page_value(src, i, cols, scale_max, predictor);
    return TIP_OK;
}

int tip_zmap_u16_dev(const int64_t *src_dev, int64_t n, uint16_t *out_dev)
{
    const char *who = "tip_zmap_u16_dev";
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!src_dev || !out_dev) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (n < 0 || n > 1000000000000L) return fail(TIP_ERR_ARG, "%s: %ld values", who, (long)n);
    if (n == 0) return TIP_OK;
    const long fours = fours_of(n, src_dev, out_dev), tail = n - 4 * fours;
    if (fours) TIP_LAUNCH("zmap_u16", k_zmap_u16<4>, dim3((unsigned)((fours + 255) / 256)), dim3(256), 0, src_dev, 0L, fours, out_dev);
    if (tail) TIP_LAUNCH("zmap_u16", k_zmap_u16<1>, dim3((unsigned)((tail + 255) / 256)), dim3(256), 0, src_dev, 4 * fours, tail, out_dev);
    return TIP_OK;
}

int tip_zmap_u16(const int64_t *src, int64_t n, uint16_t *out)
{
    if (!src || !out) return fail(TIP_ERR_ARG, "tip_zmap_u16: null pointer");
    if (n < 0) return fail(TIP_ERR_ARG, "tip_zmap_u16: %ld values", (long)n);
    for (long i = 0; i < n; ++i) out[i] = zmap_sample(src[i]);
    return TIP_OK;
}

}  // extern "C"
