// tip_export.hip -- a frame's resident maps as the uint16 pages of Tissue.export_segmentation_and_cell_types_to_tiff (ti.py:4040-4052):
// plane 0 the tracking labels -- get_trackking_labels' ids[labels - 1], 0 on label 0, cast to uint16 --, plane 1 the type map with
// 0 -> 2 and 255 -> 0.  The pages stay on the device: tip_deflate_strips_dev takes them from here (movie.export_tiff).
//
// k_export_maps_u16: one thread per four pixels -- one 16-byte load of labels, one 4-byte load of types, one 8-byte store per
// plane -- when the pixel count and the addresses allow it, one pixel per thread otherwise.  The ids are a uint16 table of a few
// kilobytes that every wave reads from cache.  A label outside [0, n_ids] becomes 0 and is counted: one sum per wave, and one
// atomic add by the wave's first lane only when the wave saw any.
#include "tip_internal.h"

namespace tip {

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

}  // extern "C"
