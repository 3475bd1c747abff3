// tip_celltypes.hip -- calc_cell_types (ti.py:2338-2408) for one frame on device buffers, asynchronous on the calling
// thread's stream: the movie driver's per-frame HC/SC typing next to the resident label map and projection.
//
//   per label: count + intensity sum (regionprops_dev with an intensity plane)
//           -> rank of np.percentile(marker[cell], q)'s lower neighbour, computed on the device from the count
//           -> radix select of that order statistic and the next (order_stats_dev, tip_select.hip), per label and, for
//              np.percentile(marker, 99), over the whole frame
//   peak test (peak_window_size > 0): blur sigma 7 (scipy 'nearest', host taps) -> maximum_filter(w, reflect) -> a per-label
//              "holds a pixel with |blur - max| < 1e-6" flag
//   -> per label: numpy's linear interpolation (the host's arithmetic, -ffp-contract=off), cut, peak rule, type / valid / mean
//   -> per pixel: the type map update_cell_types_by_cells_info paints onto an all-255 map.
#include "tip_internal.h"

namespace tip {

// _segmentation.percentile_per_label / percentile_frame: virt = (count - 1) * (q / 100), prev = clip(floor(virt), 0, count - 1)
__device__ __forceinline__ long long ct_prev(long long count, double q, double *gamma)
{
    const double virt = (double)(count - 1) * q;
    const double fl = floor(virt);
    *gamma = virt - fl;
    long long prev = (long long)fl;
    prev = prev < 0 ? 0 : prev;
    const long long top = count - 1 > 0 ? count - 1 : 0;
    return prev > top ? top : prev;
}

// numpy's 'linear' percentile from the two neighbouring order statistics (_segmentation._lerp_percentile)
__device__ __forceinline__ double ct_percentile(double lo, double hi, long long count, double q)
{
    double gamma;
    const long long prev = ct_prev(count, q, &gamma);
    const double h = prev + 1 <= count - 1 ? hi : lo;
    const double diff = h - lo;
    return gamma >= 0.5 ? h - diff * (1 - gamma) : lo + diff * gamma;
}

constexpr double CT_Q99 = 99 / 100.0;   // percentile_frame(img, 99): q / 100.0 as the host computes it

// per label: the select's ranks (-1: absent), and the exact sum of the areas (np.mean of the int64 areas = sum / n);
// thread 0 also sets the whole frame's rank
__global__ void __launch_bounds__(256) k_ct_ranks(const int64_t *__restrict__ area, int n, double q, long long *__restrict__ rank,
                                                  long long *__restrict__ rank0, unsigned long long *__restrict__ area_sum, long long P,
                                                  long long *__restrict__ frank, long long *__restrict__ frank0)
{
    __shared__ unsigned long long part[256];
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    long long a = 0;
    double gamma;
    if (l < n) {
        a = area[l];
        const long long r = a > 0 ? ct_prev(a, q, &gamma) : -1;
        rank[l] = r;
        rank0[l] = r;
    }
    if (l == 0) {
        const long long r = ct_prev(P, CT_Q99, &gamma);
        frank[0] = r;
        frank0[0] = r;
    }
    part[threadIdx.x] = (unsigned long long)a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(area_sum, part[0]);
}

// has_peak[l] = 1 when a pixel of label l + 1 is a local maximum of the blurred marker; lanes of a wave that share a label
// are combined first (wave_combine), so a cell's interior costs one store per wave instead of one per pixel
__global__ void __launch_bounds__(256) k_ct_peak(const int32_t *__restrict__ labels, const double *__restrict__ blur,
                                                 const double *__restrict__ mx, long P, int n, unsigned int *__restrict__ has_peak)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool active = false;
    int l = 0;
    if (i < P) {
        l = labels[i] - 1;
        active = l >= 0 && l < n && fabs(blur[i] - mx[i]) < 1e-6;
    }
    wave_combine(active, l, [&](int ls, int) { has_peak[ls] = 1u; });
}

// per label: validity (ti.py:2360-2367), mean intensity, and the type bit (ti.py:2369-2391)
__global__ void __launch_bounds__(256) k_ct_classify(const int64_t *__restrict__ area, const double *__restrict__ isum,
                                                     const double *__restrict__ lo, const double *__restrict__ hi,
                                                     const double *__restrict__ flo, const double *__restrict__ fhi,
                                                     const unsigned long long *__restrict__ area_sum,
                                                     const unsigned int *__restrict__ has_peak, int n, double q, long long P,
                                                     double threshold, int type_index, double min_cell_area, double max_cell_area,
                                                     uint8_t *__restrict__ out_type, uint8_t *__restrict__ out_valid,
                                                     double *__restrict__ out_mean)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n) return;
    const long long a = area[l];
    const double mean_area = (double)area_sum[0] / (double)n;
    const double smallest = min_cell_area * mean_area, largest = max_cell_area * mean_area;
    const double ad = (double)a;
    out_valid[l] = (ad < largest && ad > smallest) ? 1 : 0;
    if (a <= 0) {                  // labels that do not occur: no mean, never classified
        out_mean[l] = __longlong_as_double(0x7ff8000000000000LL);
        out_type[l] = 0;
        return;
    }
    out_mean[l] = isum[l] / ad;
    const double stat = ct_percentile(lo[l], hi[l], a, q);
    const double cut = threshold * ct_percentile(flo[0], fhi[0], P, CT_Q99);
    bool pos = stat > cut;
    if (has_peak) pos = pos && l > 0 && has_peak[l] != 0u;      // label 1 never counts as holding a peak (ti.py:2377)
    out_type[l] = pos ? (uint8_t)(1u << type_index) : (uint8_t)0;
}

// update_cell_types_by_cells_info on an all-255 map: a valid label's type, 255 elsewhere (label 0, invalid, out of range)
__global__ void __launch_bounds__(256) k_ct_paint(const int32_t *__restrict__ labels, long P, int n, const uint8_t *__restrict__ type,
                                                  const uint8_t *__restrict__ valid, uint8_t *__restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int l = labels[i];
    out[i] = (l >= 1 && l <= n && valid[l - 1]) ? type[l - 1] : (uint8_t)255;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_cell_types_i32_dev(const int32_t *labels, const double *marker, int y, int x, int n, double q_over_100, double threshold,
                           int peak_window_size, const double *peak_taps, int n_peak_taps, int type_index, double min_cell_area,
                           double max_cell_area, uint8_t *out_type, uint8_t *out_valid, double *out_mean, uint8_t *out_type_map)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!labels || !marker || !out_type_map || (n > 0 && (!out_type || !out_valid || !out_mean)))
        return fail(TIP_ERR_ARG, "tip_cell_types_i32_dev: null pointer");
    if (y < 1 || x < 1 || y > 65535 || n < 0) return fail(TIP_ERR_ARG, "tip_cell_types_i32_dev: bad shape");
    if (!(q_over_100 >= 0.0 && q_over_100 <= 1.0))
        return fail(TIP_ERR_ARG, "tip_cell_types_i32_dev: percentile %g outside [0, 100]", q_over_100 * 100.0);
    if (type_index < 0 || type_index > 7) return fail(TIP_ERR_ARG, "tip_cell_types_i32_dev: type_index %d (0..7)", type_index);
    if (peak_window_size < 0 || peak_window_size > 31)
        return fail(TIP_ERR_ARG, "tip_cell_types_i32_dev: peak_window_size %d (0..31)", peak_window_size);
    if (peak_window_size > 0 && (!peak_taps || n_peak_taps < 1))
        return fail(TIP_ERR_ARG, "tip_cell_types_i32_dev: the peak test needs the sigma-7 taps");
    const long P = (long)y * x;
    hipStream_t s = c.stream;
    WsGuard ws;
    if (n > 0) {
        int64_t *area = ws.get<int64_t>(n), *bbox = ws.get<int64_t>((size_t)4 * n), *sy = ws.get<int64_t>(n), *sx = ws.get<int64_t>(n),
                *pc = ws.get<int64_t>((size_t)3 * n);
        double *isum = ws.get<double>(n), *lo = ws.get<double>(n), *hi = ws.get<double>(n), *flo = ws.get<double>(1),
               *fhi = ws.get<double>(1);
        long long *rank = ws.get<long long>(n), *rank0 = ws.get<long long>(n), *frank = ws.get<long long>(1),
                  *frank0 = ws.get<long long>(1);
        unsigned long long *area_sum = ws.get<unsigned long long>(1);
        if (!area || !bbox || !sy || !sx || !pc || !isum || !lo || !hi || !flo || !fhi || !rank || !rank0 || !frank || !frank0 ||
            !area_sum)
            return TIP_ERR_NOMEM;
        int rc = regionprops_dev(labels, marker, y, x, n, area, bbox, sy, sx, pc, isum);
        if (rc) return rc;
        TIP_HIP(hipMemsetAsync(area_sum, 0, 8, s));
        TIP_LAUNCH("ct_ranks", k_ct_ranks, dim3(cdiv(n, 256)), dim3(256), 0, (const int64_t *)area, n, q_over_100, rank, rank0,
                   area_sum, (long long)P, frank, frank0);
        if ((rc = order_stats_dev(labels, marker, P, n, rank, rank0, lo, hi))) return rc;
        if ((rc = order_stats_dev(nullptr, marker, P, 1, frank, frank0, flo, fhi))) return rc;
        unsigned int *has_peak = nullptr;
        if (peak_window_size > 0) {
            has_peak = ws.get<unsigned int>(n);
            double *blur = ws.get<double>(P), *mx = ws.get<double>(P);
            if (!has_peak || !blur || !mx) return TIP_ERR_NOMEM;
            TIP_HIP(hipMemsetAsync(has_peak, 0, (size_t)n * 4, s));
            if ((rc = gaussian3d_dev(marker, blur, 1, 1, y, x, nullptr, 0, peak_taps, n_peak_taps, peak_taps, n_peak_taps))) return rc;
            if ((rc = rankfilter2d_dev(blur, mx, 1, y, x, peak_window_size, peak_window_size, 0, 1, 1))) return rc;
            TIP_LAUNCH("ct_peak", k_ct_peak, dim3(cdiv(P, 256)), dim3(256), 0, labels, (const double *)blur, (const double *)mx, P, n,
                       has_peak);
        }
        TIP_LAUNCH("ct_classify", k_ct_classify, dim3(cdiv(n, 256)), dim3(256), 0, (const int64_t *)area, (const double *)isum,
                   (const double *)lo, (const double *)hi, (const double *)flo, (const double *)fhi,
                   (const unsigned long long *)area_sum, (const unsigned int *)has_peak, n, q_over_100, (long long)P, threshold,
                   type_index, min_cell_area, max_cell_area, out_type, out_valid, out_mean);
    }
    TIP_LAUNCH("ct_paint", k_ct_paint, dim3(cdiv(P, 256)), dim3(256), 0, labels, P, n, (const uint8_t *)out_type,
               (const uint8_t *)out_valid, out_type_map);
    return TIP_OK;
}

}  // extern "C"
