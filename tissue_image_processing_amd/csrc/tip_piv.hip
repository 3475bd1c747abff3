// tip_piv.hip -- the PIV step of the frame-sharded movie tracker (movie.process_movie(use_piv=True)): the TV-L1 flow from
// frame t-1's reference-channel plane to frame t's, sampled at frame t-1's centroids with upstream's transposed indexing
// (ti.py:2061-2070), and the label look-up of the moved centroids in frame t's 3x3-max-filtered label map (ti.py:2081-2090).
//
// Both planes and the label map stay on the device; the flow (2 x Y x X float32) lives in the workspace and never leaves
// it.  Only the per-row centroids go up and the hits plus one error word come back.  DESIGN.md section 9 (movie driver).
#include "tip_internal.h"
#include <cmath>

namespace tip {

namespace {

constexpr unsigned long long PIV_NO_ERROR = ~0ull;

// numpy's astype(int64) of a rounded float64: NaN, infinities and values past int64 become INT64_MIN (x86's cvttsd2si)
__device__ __host__ inline long long as_i64(double r)
{
    return (r >= -9223372036854775808.0 && r < 9223372036854775808.0) ? (long long)r : (long long)(-9223372036854775807LL - 1);
}

// One thread per previous row i:
//   rows = round(cx), cols = round(cy)   (half to even; negative indices in [-n, 0) wrap, anything else outside raises)
//   cx -= flow_row[rows, cols], cy -= flow_col[rows, cols]   (float64)
//   hit = max3(labels)[round(cy), round(cx)], -1 outside the frame or for an absent row
// A row whose index would raise writes key = i (axis 0) or n + i (axis 1 only) to *err with atomicMin: the smallest key is
// numpy's error (every row's axis-0 index is checked before any axis-1 index, each in row order).
__global__ void __launch_bounds__(256) k_piv_sample_max3(const float *__restrict__ flow, const int32_t *__restrict__ lab, int Y,
                                                         int X, const double *__restrict__ cy, const double *__restrict__ cx,
                                                         const uint8_t *__restrict__ present, long n, int32_t *__restrict__ hit,
                                                         unsigned long long *__restrict__ err)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double px = cx[i], py = cy[i];
    long long r = as_i64(rint(px)), c = as_i64(rint(py));
    const bool bad_r = r < -(long long)Y || r >= Y, bad_c = c < -(long long)X || c >= X;
    if (bad_r || bad_c) {
        atomicMin(err, bad_r ? (unsigned long long)i : (unsigned long long)(n + i));
        hit[i] = -1;
        return;
    }
    if (r < 0) r += Y;
    if (c < 0) c += X;
    const long p = (long)r * X + c;
    px = px - (double)flow[p];
    py = py - (double)flow[(long)Y * X + p];
    const double qy = rint(py), qx = rint(px);
    if (!(qy >= 0.0 && qy < (double)Y && qx >= 0.0 && qx < (double)X) || !present[i]) {   // (NaN fails the test: outside)
        hit[i] = -1;
        return;
    }
    const int y = (int)qy, x = (int)qx;
    int32_t best = 0;                                    // maximum_filter(mode='constant'): zeros outside the frame
    for (int j = -1; j <= 1; ++j)
        for (int k = -1; k <= 1; ++k) {
            const int yy = y + j, xx = x + k;
            if (yy >= 0 && yy < Y && xx >= 0 && xx < X) best = max(best, lab[(long)yy * X + xx]);
        }
    hit[i] = best;
}

// numpy's IndexError text for the first failing row (the host recomputes the index from the host copy of the centroids)
int index_error(unsigned long long key, int y, int x, const double *cy_host, const double *cx_host, int64_t n)
{
    const bool axis1 = key >= (unsigned long long)n;
    const int64_t i = axis1 ? (int64_t)(key - n) : (int64_t)key;
    const long long idx = as_i64(std::nearbyint(axis1 ? cy_host[i] : cx_host[i]));
    return fail(TIP_ERR_INDEX, "index %lld is out of bounds for axis %d with size %d", idx, axis1 ? 1 : 0, axis1 ? x : y);
}

int piv_sample(const float *flow, const int32_t *labels, int y, int x, const double *cy_host, const double *cx_host,
               const uint8_t *present_host, int64_t n, int32_t *hit_host)
{
    Ctx &c = ctx();
    WsGuard ws;
    double *dcy = ws.get<double>(n), *dcx = ws.get<double>(n);
    uint8_t *dpres = ws.get<uint8_t>(n);
    int32_t *dhit = ws.get<int32_t>(n);
    unsigned long long *derr = ws.get<unsigned long long>(1);
    if (!dcy || !dcx || !dpres || !dhit || !derr) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(dcy, cy_host, n * 8, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemcpyAsync(dcx, cx_host, n * 8, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemcpyAsync(dpres, present_host, n, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemsetAsync(derr, 0xff, sizeof(unsigned long long), c.stream));
    TIP_LAUNCH("piv_sample_max3", k_piv_sample_max3, dim3(cdiv(n, 256)), dim3(256), 0, flow, labels, y, x, (const double *)dcy,
               (const double *)dcx, (const uint8_t *)dpres, (long)n, dhit, derr);
    unsigned long long key = PIV_NO_ERROR;
    TIP_HIP(hipMemcpyAsync(hit_host, dhit, n * 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipMemcpyAsync(&key, derr, sizeof(key), hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    if (key != PIV_NO_ERROR) return index_error(key, y, x, cy_host, cx_host, n);
    return TIP_OK;
}

}  // namespace

}  // namespace tip

using namespace tip;

extern "C" {

int tip_piv_sample_max3_i32_dev(const float *flow, const int32_t *labels, int y, int x, const double *cy_host,
                                const double *cx_host, const uint8_t *present_host, int64_t n, int32_t *hit_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!flow || !labels || y < 1 || x < 1 || n < 0) return fail(TIP_ERR_ARG, "tip_piv_sample_max3_i32_dev: bad arguments");
    if (n == 0) return TIP_OK;
    if (!cy_host || !cx_host || !present_host || !hit_host) return fail(TIP_ERR_ARG, "tip_piv_sample_max3_i32_dev: null pointer");
    return piv_sample(flow, labels, y, x, cy_host, cx_host, present_host, n, hit_host);
}

int tip_piv_lookup_max3_i32_dev(const double *prev_plane, const double *cur_plane, const int32_t *labels, int y, int x,
                                const double *cy_host, const double *cx_host, const uint8_t *present_host, int64_t n,
                                float attachment, float tightness, int num_warp, int num_iter, double tol, float *flow_dev,
                                int32_t *hit_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!prev_plane || !cur_plane || !labels || y < 2 || x < 2 || n < 0)
        return fail(TIP_ERR_ARG, "tip_piv_lookup_max3_i32_dev: bad arguments");
    if (n > 0 && (!cy_host || !cx_host || !present_host || !hit_host))
        return fail(TIP_ERR_ARG, "tip_piv_lookup_max3_i32_dev: null pointer");
    if (n == 0 && !flow_dev) return TIP_OK;             // nothing to sample: the flow would not be seen
    WsGuard ws;
    float *flow = flow_dev ? flow_dev : ws.get<float>((size_t)2 * y * x);
    if (!flow) return TIP_ERR_NOMEM;
    const int rc = optical_flow_tvl1_dev(prev_plane, cur_plane, OF_F64_AS_U16, y, x, attachment, tightness, num_warp, num_iter,
                                         tol, flow, nullptr, 0);
    if (rc < 0) return rc;
    if (n == 0) return TIP_OK;
    return piv_sample(flow, labels, y, x, cy_host, cx_host, present_host, n, hit_host);
}

}  // extern "C"
