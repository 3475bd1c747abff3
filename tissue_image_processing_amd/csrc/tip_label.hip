// tip_label.hip -- device-wide scan, union-find connected components (raster-order numbering), rank filters.
//
//   label4:      skimage.measure.label(connectivity=1, background=bg)   (ti.py:2922, 3470)
//                == scipy.ndimage.label on a boolean image               (watershed markers, _watershed.py:76)
//   rank filter: scipy.ndimage.maximum_filter / minimum_filter and grey erosion / dilation with a flat
//                footprint (ti.py:1822,2081,2969,4079-4084; pl.py:170-193; bim.py:468-472 via threshold_local)
#include "tip_internal.h"
#include "tip_uf.h"

namespace tip {

// ---------------------------------------------------------------------------------------------------------
// exclusive scan of int32 (three kernels: per-block scan, scan of block sums, add), all on the block scan of tip_wave.h; the scan
// of the block sums alone is scan_i32_dev, the scan of the neighbour graph, the Delaunay rows, the point grid and the track linker
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_block(const int *__restrict__ in, int *__restrict__ out, long n,
                                                             int *__restrict__ bsum)
{
    __shared__ int wsum[SCAN_THREADS / 64];
    const int total = scan_tile_i32(in, out, (long)blockIdx.x * SCAN_BLOCK + (long)threadIdx.x * SCAN_ITEMS, n, wsum);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// out[i] = in[0] + ... + in[i - 1] for i = 0 .. n - 1 and *total = their sum (total may be NULL): one workgroup walks the array in
// chunks of 1024, one block scan per chunk, and every thread carries the sum along.  in == out is allowed -- a thread reads its
// element before the scan's barrier and any thread of the chunk writes behind it -- so neither is __restrict__.  The scan of the
// block sums ("scan_sums") and scan_i32_dev.
__global__ void __launch_bounds__(1024) k_scan_one(const int *in, int *out, int n, int *total)
{
    __shared__ int wsum[16];
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x, v = i < n ? in[i] : 0;
        int sum;
        const int before = block_exclusive_scan<16>(v, wsum, sum);
        if (i < n) out[i] = carry + before;
        carry += sum;
        __syncthreads();                            // (the next chunk writes wsum)
    }
    if (threadIdx.x == 0 && total) *total = carry;
}

// ... with the scan of the block sums folded in (few blocks: every block adds up the sums in front of it itself -- one launch less;
// the last block writes the total)
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_add_own(int *__restrict__ out, long n, const int *__restrict__ bsum, int nb,
                                                               int *__restrict__ total)
{
    __shared__ int wsum[SCAN_THREADS / 64];
    int s = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += SCAN_THREADS) s += bsum[j];
    const int off = block_sum<SCAN_THREADS / 64>(s, wsum);
    if (total && (int)blockIdx.x == nb - 1 && threadIdx.x == 0) *total = off + bsum[nb - 1];
    const long base = (long)blockIdx.x * SCAN_BLOCK + (long)threadIdx.x * SCAN_ITEMS;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < n) out[base + i] += off;
}

__global__ void __launch_bounds__(SCAN_THREADS) k_scan_add(int *__restrict__ out, long n, const int *__restrict__ bsum)
{
    const int off = bsum[blockIdx.x];
    const long base = (long)blockIdx.x * SCAN_BLOCK + (long)threadIdx.x * SCAN_ITEMS;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < n) out[base + i] += off;
}

int exclusive_scan_i32(const int *in, int *out, long n, int *total_dev)
{
    const int nb = cdiv(n, SCAN_BLOCK);
    WsGuard ws;
    int *bsum = ws.get<int>(nb);
    if (!bsum) return TIP_ERR_NOMEM;
    TIP_LAUNCH("scan_block", k_scan_block, dim3(nb), dim3(SCAN_THREADS), 0, in, out, n, bsum);
    if (nb <= 4096) {          // (up to 8.4 M elements: a block reads at most 16 KB of block sums out of L2)
        TIP_LAUNCH("scan_add_own", k_scan_add_own, dim3(nb), dim3(SCAN_THREADS), 0, out, n, (const int *)bsum, nb, total_dev);
        return TIP_OK;
    }
    TIP_LAUNCH("scan_sums", k_scan_one, dim3(1), dim3(1024), 0, (const int *)bsum, bsum, nb, total_dev);
    TIP_LAUNCH("scan_add", k_scan_add, dim3(nb), dim3(SCAN_THREADS), 0, out, n, (const int *)bsum);
    return TIP_OK;
}

// the small tables (cell counts, degrees): the single workgroup alone, out[n] = the total
int scan_i32_dev(const int32_t *in, int32_t *out, int n)
{
    TIP_LAUNCH("csr_scan", k_scan_one, dim3(1), dim3(1024), 0, in, out, n, out + n);
    return TIP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// connected components with raster-order numbering
// ---------------------------------------------------------------------------------------------------------
struct SameI32 {
    const int32_t *in;
    int32_t bg;
    __device__ __forceinline__ bool valid(int i) const { return in[i] != bg; }
    __device__ __forceinline__ bool same(int i, int j) const { return in[i] == in[j]; }
};

__global__ void __launch_bounds__(256) k_root_flags_i32(SameI32 s, const int *__restrict__ parent, int *__restrict__ flag,
                                                        long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (s.valid((int)i) && parent[i] == (int)i) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_relabel_i32(SameI32 s, const int *__restrict__ parent,
                                                     const int *__restrict__ rank, int32_t *__restrict__ out, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = s.valid((int)i) ? rank[parent[i]] + 1 : 0;
}

int label4_dev(const int32_t *in, int32_t bg, int32_t *out, int Y, int X, int32_t *n_labels_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !out) return fail(TIP_ERR_ARG, "label4: null pointer");
    if (Y < 1 || X < 1 || (long)Y * X > 2147483647L) return fail(TIP_ERR_ARG, "label4: bad shape %dx%d", Y, X);
    const long n = (long)Y * X;
    WsGuard ws;
    int *parent = ws.get<int>(n), *flag = ws.get<int>(n), *rank = ws.get<int>(n), *total = ws.get<int>(1);
    if (!parent || !flag || !rank || !total) return TIP_ERR_NOMEM;
    SameI32 s{in, bg};
    int rc = uf_components(s, parent, Y, X);
    if (rc) return rc;
    TIP_LAUNCH("ccl_root_flags", k_root_flags_i32, dim3(cdiv(n, 256)), dim3(256), 0, s, (const int *)parent, flag, n);
    if ((rc = exclusive_scan_i32(flag, rank, n, total))) return rc;
    TIP_LAUNCH("ccl_relabel", k_relabel_i32, dim3(cdiv(n, 256)), dim3(256), 0, s, (const int *)parent,
               (const int *)rank, out, n);
    if (n_labels_host) {
        int h = 0;
        TIP_HIP(hipMemcpyAsync(&h, total, sizeof(int), hipMemcpyDeviceToHost, c.stream));
        TIP_HIP(hipStreamSynchronize(c.stream));
        *n_labels_host = h;
    }
    return TIP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// rank filters
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect_idx(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// footprint_kind 0: ky x kx rectangle (window i-k/2 .. i-k/2+k-1, scipy origin 0); 1: 3x3 cross without centre
template <typename T>
__global__ void __launch_bounds__(256) k_rank2d(const T *__restrict__ in, T *__restrict__ out, int Y, int X, int ky, int kx,
                                                int fp, int reflect, int is_max)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= X) return;
    const int oy = ky / 2, ox = kx / 2;
    bool have = false;
    T best = 0;
    for (int j = 0; j < ky; ++j)
        for (int i = 0; i < kx; ++i) {
            if (fp == 1 && !(((j == 1) ^ (i == 1)))) continue;  // cross: exactly one of (row, col) is the middle
            int yy = y - oy + j, xx = x - ox + i;
            T v;
            if (reflect) {
                v = in[(long)reflect_idx(yy, Y) * X + reflect_idx(xx, X)];
            } else {
                v = (yy < 0 || yy >= Y || xx < 0 || xx >= X) ? (T)0 : in[(long)yy * X + xx];
            }
            if (!have) { best = v; have = true; }
            else if (is_max ? (v > best) : (v < best)) best = v;
        }
    out[(long)y * X + x] = best;
}

// Windows up to RANK_DIRECT_MAX on both sides: one launch that visits all ky * kx pixels (every call site of the reference).
// Wider rectangles run as a row pass and a column pass of the same kernel: a rectangular maximum / minimum is exactly separable
// (reflection acts per axis; the zero padding of 'constant' takes part in both passes, and a window that leaves the frame along
// either axis sees it either way), ky + kx reads per pixel instead of ky * kx and the same bits.
constexpr int RANK_DIRECT_MAX = 31, RANK_MAX = 255;

template <typename T>
static int rank2d_launch(const T *in, T *out, int Y, int X, int ky, int kx, int fp, int border, int is_max)
{
    TIP_LAUNCH(sizeof(T) == 8 ? "rank2d_f64" : "rank2d_i32", k_rank2d<T>, dim3(cdiv(X, 256), Y), dim3(256), 0, in, out, Y, X, ky, kx,
               fp, border, is_max);
    return TIP_OK;
}

template <typename T>
static int rank2d(const T *in, T *out, int Y, int X, int ky, int kx, int fp, int border, int is_max)
{
    if ((ky <= RANK_DIRECT_MAX && kx <= RANK_DIRECT_MAX) || ky == 1 || kx == 1)
        return rank2d_launch(in, out, Y, X, ky, kx, fp, border, is_max);
    WsGuard ws;
    T *rows = ws.get<T>((size_t)Y * X);
    if (!rows) return TIP_ERR_NOMEM;
    int rc = rank2d_launch(in, rows, Y, X, 1, kx, 0, border, is_max);
    if (rc) return rc;
    return rank2d_launch((const T *)rows, out, Y, X, ky, 1, 0, border, is_max);
}

int rankfilter2d_dev(const void *in, void *out, int dtype, int Y, int X, int ky, int kx, int fp, int border, int is_max)
{
    if (!in || !out || in == out) return fail(TIP_ERR_ARG, "rankfilter2d: null or aliased pointers");
    if (Y < 1 || X < 1 || Y > 65535) return fail(TIP_ERR_ARG, "rankfilter2d: bad shape");
    if (ky < 1 || kx < 1 || ky > RANK_MAX || kx > RANK_MAX)
        return fail(TIP_ERR_ARG, "rankfilter2d: window %dx%d (sides 1..%d)", ky, kx, RANK_MAX);
    if (fp == 1 && (ky != 3 || kx != 3)) return fail(TIP_ERR_ARG, "cross footprint is 3x3");
    if (fp != 0 && fp != 1) return fail(TIP_ERR_ARG, "footprint_kind %d", fp);
    if (dtype == 1) return rank2d((const double *)in, (double *)out, Y, X, ky, kx, fp, border, is_max);
    if (dtype == 2) return rank2d((const int32_t *)in, (int32_t *)out, Y, X, ky, kx, fp, border, is_max);
    return fail(TIP_ERR_ARG, "rankfilter2d: dtype %d (1=f64, 2=i32)", dtype);
}

// bim.py:464-473: thr = imgthresh * max(block x block, reflect) (float64); out = img < thr ? 0 : img
__global__ void __launch_bounds__(256) k_local_threshold(const double *__restrict__ img, double *__restrict__ out, int Y, int X,
                                                         double imgthresh, int block)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= X) return;
    const int o = block / 2;
    double best = img[(long)reflect_idx(y - o, Y) * X + reflect_idx(x - o, X)];
    for (int j = 0; j < block; ++j)
        for (int i = 0; i < block; ++i) {
            const double v = img[(long)reflect_idx(y - o + j, Y) * X + reflect_idx(x - o + i, X)];
            if (v > best) best = v;
        }
    const double thr = imgthresh * best;
    const double v = img[(long)y * X + x];
    out[(long)y * X + x] = v < thr ? 0.0 : v;
}

// ... the same from a maximum that the separable rank filter has already formed (blocks wider than RANK_DIRECT_MAX)
__global__ void __launch_bounds__(256) k_threshold_by_max(const double *__restrict__ img, const double *__restrict__ mx,
                                                          double *__restrict__ out, long n, double imgthresh)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double thr = imgthresh * mx[i];
    const double v = img[i];
    out[i] = v < thr ? 0.0 : v;
}

__global__ void __launch_bounds__(256) k_update_labels(const int32_t *__restrict__ in, int32_t *__restrict__ out, int Y, int X)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= X) return;
    int32_t v = in[(long)y * X + x];
    if (v < 0) {
        int32_t best = 0;  // zero padding takes part in the maximum (mode='constant')
        bool have = false;
        for (int j = -1; j <= 1; ++j)
            for (int i = -1; i <= 1; ++i) {
                const int yy = y + j, xx = x + i;
                const int32_t q = (yy < 0 || yy >= Y || xx < 0 || xx >= X) ? 0 : in[(long)yy * X + xx];
                if (!have) { best = q; have = true; }
                else if (q > best) best = q;
            }
        v = best;
    }
    out[(long)y * X + x] = v;
}

__global__ void __launch_bounds__(256) k_lut_gather(const int32_t *__restrict__ labels, const int64_t *__restrict__ lut,
                                                    int64_t n_lut, int64_t *__restrict__ out, long n, int *__restrict__ err)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    if (l < 0 || l >= n_lut) { atomicOr(err, 1); out[i] = 0; return; }
    out[i] = lut[l];
}

// T3 lookup (ti.py:2081-2090): value of maximum_filter(labels, (3,3), mode='constant') at rounded query points
__global__ void __launch_bounds__(256) k_lookup_max3(const int32_t *__restrict__ lab, int Y, int X, const int64_t *__restrict__ qy,
                                                     const int64_t *__restrict__ qx, long n, int32_t *__restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long y = qy[i], x = qx[i];
    if (y < 0 || y >= Y || x < 0 || x >= X) { out[i] = -1; return; }  // invalid location (ti.py:2086-2087)
    int32_t best = 0;
    bool have = false;
    for (int j = -1; j <= 1; ++j)
        for (int k = -1; k <= 1; ++k) {
            const long yy = y + j, xx = x + k;
            const int32_t q = (yy < 0 || yy >= Y || xx < 0 || xx >= X) ? 0 : lab[yy * X + xx];
            if (!have) { best = q; have = true; }
            else if (q > best) best = q;
        }
    out[i] = best;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_label4_i32_dev(const int32_t *in, int32_t bg, int32_t *out, int y, int x, int32_t *n_labels_host)
{
    return label4_dev(in, bg, out, y, x, n_labels_host);
}

int tip_label4_i32(const int32_t *in, int32_t bg, int32_t *out, int y, int x, int32_t *n_labels)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !out) return fail(TIP_ERR_ARG, "tip_label4_i32: null pointer");
    if (y < 1 || x < 1) return fail(TIP_ERR_ARG, "tip_label4_i32: empty image");
    const size_t bytes = (size_t)y * x * 4;
    WsGuard ws;
    int32_t *din = ws.get<int32_t>((size_t)y * x), *dout = ws.get<int32_t>((size_t)y * x);
    if (!din || !dout) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, c.stream));
    int32_t nl = 0;
    int rc = label4_dev(din, bg, dout, y, x, &nl);
    if (rc) return rc;
    TIP_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    if (n_labels) *n_labels = nl;
    return TIP_OK;
}

int tip_rankfilter2d_dev(const void *in, void *out, int dtype, int y, int x, int ky, int kx, int footprint_kind,
                         int border_mode, int is_max)
{
    return rankfilter2d_dev(in, out, dtype, y, x, ky, kx, footprint_kind, border_mode, is_max);
}

int tip_rankfilter2d(const void *in, void *out, int dtype, int y, int x, int ky, int kx, int footprint_kind,
                     int border_mode, int is_max)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !out) return fail(TIP_ERR_ARG, "tip_rankfilter2d: null pointer");
    if (dtype != 1 && dtype != 2) return fail(TIP_ERR_ARG, "tip_rankfilter2d: dtype %d (1=f64, 2=i32)", dtype);
    if (y < 1 || x < 1) return fail(TIP_ERR_ARG, "tip_rankfilter2d: empty image");
    const size_t bytes = (size_t)y * x * (dtype == 1 ? 8 : 4);
    WsGuard ws;
    char *din = ws.get<char>(bytes), *dout = ws.get<char>(bytes);
    if (!din || !dout) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, c.stream));
    int rc = rankfilter2d_dev(din, dout, dtype, y, x, ky, kx, footprint_kind, border_mode, is_max);
    if (rc) return rc;
    TIP_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    return TIP_OK;
}

int tip_local_threshold_f64_dev(const double *img, double *out, int y, int x, double imgthresh, int block)
{
    if (!img || !out || img == out) return fail(TIP_ERR_ARG, "tip_local_threshold_f64_dev: null or aliased pointers");
    if (block < 1 || block > RANK_MAX) return fail(TIP_ERR_ARG, "block size %d (1..%d)", block, RANK_MAX);
    if (block % 2 == 0) block += 1;  // bim.py:466-467
    if (y < 1 || x < 1 || y > 65535) return fail(TIP_ERR_ARG, "bad shape");
    if (block <= RANK_DIRECT_MAX) {
        TIP_LAUNCH("local_threshold", k_local_threshold, dim3(cdiv(x, 256), y), dim3(256), 0, img, out, y, x, imgthresh, block);
        return TIP_OK;
    }
    const long n = (long)y * x;
    WsGuard ws;
    double *mx = ws.get<double>((size_t)n);
    if (!mx) return TIP_ERR_NOMEM;
    int rc = rankfilter2d_dev(img, mx, 1, y, x, block, block, 0, 1, 1);
    if (rc) return rc;
    TIP_LAUNCH("threshold_by_max", k_threshold_by_max, dim3(cdiv(n, 256)), dim3(256), 0, img, (const double *)mx, out, n, imgthresh);
    return TIP_OK;
}

int tip_update_labels_i32(int32_t *labels, int y, int x)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!labels || y < 1 || x < 1 || y > 65535) return fail(TIP_ERR_ARG, "tip_update_labels_i32: bad arguments");
    const size_t bytes = (size_t)y * x * 4;
    WsGuard ws;
    int32_t *din = ws.get<int32_t>((size_t)y * x), *dout = ws.get<int32_t>((size_t)y * x);
    if (!din || !dout) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(din, labels, bytes, hipMemcpyHostToDevice, c.stream));
    TIP_LAUNCH("update_labels", k_update_labels, dim3(cdiv(x, 256), y), dim3(256), 0, (const int32_t *)din, dout, y, x);
    TIP_HIP(hipMemcpyAsync(labels, dout, bytes, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    return TIP_OK;
}

int tip_lookup_max3_i32_dev(const int32_t *labels, int y, int x, const int64_t *qy_host, const int64_t *qx_host, int64_t n,
                            int32_t *out_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!labels || y < 1 || x < 1 || n < 0) return fail(TIP_ERR_ARG, "tip_lookup_max3_i32_dev: bad arguments");
    if (n == 0) return TIP_OK;
    if (!qy_host || !qx_host || !out_host) return fail(TIP_ERR_ARG, "tip_lookup_max3_i32_dev: null pointer");
    WsGuard ws;
    int64_t *dy = ws.get<int64_t>(n), *dx = ws.get<int64_t>(n);
    int32_t *dout = ws.get<int32_t>(n);
    if (!dy || !dx || !dout) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(dy, qy_host, n * 8, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemcpyAsync(dx, qx_host, n * 8, hipMemcpyHostToDevice, c.stream));
    TIP_LAUNCH("lookup_max3", k_lookup_max3, dim3(cdiv(n, 256)), dim3(256), 0, labels, y, x, (const int64_t *)dy,
               (const int64_t *)dx, (long)n, dout);
    TIP_HIP(hipMemcpyAsync(out_host, dout, n * 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    return TIP_OK;
}

int tip_lut_gather_i32(const int32_t *labels, const int64_t *lut, int64_t n_lut, int64_t *out, int64_t n)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!labels || !lut || !out || n < 1 || n_lut < 1) return fail(TIP_ERR_ARG, "tip_lut_gather_i32: bad arguments");
    WsGuard ws;
    int32_t *dl = ws.get<int32_t>(n);
    int64_t *dlut = ws.get<int64_t>(n_lut), *dout = ws.get<int64_t>(n);
    int *err = ws.get<int>(1);
    if (!dl || !dlut || !dout || !err) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(dl, labels, n * 4, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemcpyAsync(dlut, lut, n_lut * 8, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemsetAsync(err, 0, 4, c.stream));
    TIP_LAUNCH("lut_gather", k_lut_gather, dim3(cdiv(n, 256)), dim3(256), 0, (const int32_t *)dl, (const int64_t *)dlut, n_lut,
               dout, (long)n, err);
    int h = 0;
    TIP_HIP(hipMemcpyAsync(out, dout, n * 8, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipMemcpyAsync(&h, err, 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    if (h) return fail(TIP_ERR_INDEX, "label outside the lookup table (index out of bounds)");
    return TIP_OK;
}

}  // extern "C"
