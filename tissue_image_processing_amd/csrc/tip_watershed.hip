// tip_watershed.hip -- skimage.segmentation.watershed(image, markers=None, connectivity=1, watershed_line=True)
// (reference call sites bim.py:475 and pl.py:194) as a data-parallel flood.
//
// The serial algorithm (skimage/segmentation/_watershed_cy.pyx, restated for the tests under oracle/) pops pixels from
// a (value, age) heap.  What decides a pixel's fate is only WHICH OF ITS NEIGHBOURS WERE LABELLED BEFORE IT POPS:
//   * a pixel pops at time T = (value, index) -- or, if every lower neighbour is a watershed line, right after the
//     first neighbour that gets labelled later ("pulled", it then inherits that neighbour's pop time and label);
//   * when it pops, it becomes a line if the neighbours labelled before it carry >= 2 different labels, else it
//     takes their label.
// Mode A ("rounds") evaluates exactly that rule for every undecided pixel in parallel and only commits a pixel when
// the states it read certify the outcome (a not-yet-decided neighbour that could still pop earlier makes the pixel
// wait; a bounded flood of the "pocket" of earlier-keyed undecided pixels proves that nothing can reach it first).
// Decisions are monotone, so stale reads are merely conservative, and tiles iterate to a local fixed point in LDS.
// If the tile rounds, the per-component endgame and the wide pass all stall (plateaus larger than any certificate), the
// rest is one serial dependency chain and is finished by the host stage flood_keyed_finish (tip_ws_serial.hip) with the
// same pop-time rule, which keeps the result identical to the serial flood for any image whose non-marker pixels carry
// DISTINCT values -- that is the guarantee of mode A.  Mode A orders equal values by raster index, the serial heap by push
// age.  Ties are looked for where they can matter locally -- between non-marker pixels that are 4-neighbours or share a
// 4-neighbour (diagonals, distance two: a pulled pixel between them sees one before the other) -- `flags` bit0 reports them,
// and unless the caller chose the fast policy (TIP_WS_TIES=fast) such an image is flooded by the exact serial replay
// flood_exact instead (bit2).  Equal values between pixels further apart can still matter through a CHAIN of pulled pixels
// (a pocket enclosed by lines floods at once); float landscapes do not produce such exact ties away from plateaus, integer
// landscapes trip the local detector everywhere, and no such case is known -- but it is outside the guarantee.
// Mode B handles two-valued images (pl.py:194 floods a {0,255} boundary image) EXACTLY: the pop order of the equal-keyed
// markers follows from the array heap's mechanics (tip_heaporder.hip), everything after it is a FIFO, i.e. a
// breadth-first search in generations whose pixels carry dense ranks (tip_ws_binary.hip; mode A: tip_ws_tiles.hip).
#include "tip_ws.h"
#include "tip_uf.h"
#include <algorithm>

namespace tip {

// Both reductions: 4 independent loads per thread and trip, one atomic per BLOCK (thousands of same-address 64-bit
// atomics serialise in L2 and used to cost more than the 32 MB read itself).
constexpr int WS_RED_BLOCKS = 512;

__global__ void __launch_bounds__(256) k_ws_minmax(const double *__restrict__ v, long n, WsInfo *info)
{
    __shared__ unsigned long long slo[4], shi[4];
    unsigned long long lo = ~0ULL, hi = 0ULL;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += 4 * stride) {
        unsigned long long e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = i + u * stride < n ? enc_f64(v[i + u * stride]) : enc_f64(v[i]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            lo = e[u] < lo ? e[u] : lo;
            hi = e[u] > hi ? e[u] : hi;
        }
    }
    lo = block_reduce<4>(lo, slo, [](unsigned long long a, unsigned long long b) { return b < a ? b : a; });
    hi = block_reduce<4>(hi, shi, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
    if (threadIdx.x == 0) {
        atomicMin(&info->emin, lo);
        atomicMax(&info->emax, hi);
    }
}

__global__ void __launch_bounds__(256) k_ws_count_other(const double *__restrict__ v, long n, WsInfo *info)
{
    __shared__ unsigned long long sc[4];
    const unsigned long long emin = info->emin, emax = info->emax;
    unsigned long long c = 0;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += 4 * stride) {
        unsigned long long e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = i + u * stride < n ? enc_f64(v[i + u * stride]) : emin;
#pragma unroll
        for (int u = 0; u < 4; ++u) c += (e[u] != emin && e[u] != emax);
    }
    c = block_sum<4>(c, sc);
    if (threadIdx.x == 0 && c) atomicAdd(&info->n_other, c);
}

// ---- markers: label(local_minima(image)) ---------------------------------------------------------------------------
// Equal-valued neighbours belong to one plateau.  On a two-valued image (the U-Net tail's boundary map) the plateau of the
// MAXIMUM is one giant network that can never be a minimum (it touches the other value somewhere): its pixels stay out of the
// union-find -- hundreds of thousands of unions onto one root were 0.65 ms of contention -- and k_ws_lower_flags marks every one
// of them as "has a lower neighbour".  Whether the image is two-valued is read from the device-side scalars of the two
// reductions that ran just before (no host round trip).
struct SameF64 {
    const double *v;
    const WsInfo *info;
    __device__ __forceinline__ bool two_valued_max(int i) const
    {
        return info->n_other == 0 && info->emin != info->emax && enc_f64(v[i]) == info->emax;
    }
    __device__ __forceinline__ bool valid(int i) const { return !two_valued_max(i); }
    __device__ __forceinline__ bool same(int i, int j) const { return v[i] == v[j]; }
};

// flag[root] |= 1 when the plateau has a strictly lower 4-neighbour, or equals the global maximum and touches the
// image border (skimage pads with the value no candidate can beat and rejects plateaus that equal it, extrema.py)
__global__ void __launch_bounds__(256) k_ws_lower_flags(const double *__restrict__ v, const int *__restrict__ parent,
                                                        int *__restrict__ flag, int Y, int X, const WsInfo *info)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= X) return;
    const int i = y * X + x;
    const double h = v[i];
    bool bad = false;
    if (y > 0 && v[i - X] < h) bad = true;
    if (x > 0 && v[i - 1] < h) bad = true;
    if (x < X - 1 && v[i + 1] < h) bad = true;
    if (y < Y - 1 && v[i + X] < h) bad = true;
    if ((y == 0 || x == 0 || y == Y - 1 || x == X - 1) && enc_f64(h) == info->emax) bad = true;
    if (info->n_other == 0 && info->emin != info->emax && enc_f64(h) == info->emax) bad = true;   // (see SameF64: left out of the union-find)
    // (one giant plateau -- the boundary network of a two-valued image -- would otherwise take hundreds of thousands of
    // same-address atomics; the flag only ever goes 0 -> 1, so a stale 0 just costs one more atomic)
    if (bad) { const int r = parent[i]; if (flag[r] == 0) atomicOr(&flag[r], 1); }
}

__global__ void __launch_bounds__(256) k_ws_min_roots(const int *__restrict__ parent, const int *__restrict__ flag,
                                                      int *__restrict__ isroot, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) isroot[i] = (parent[i] == (int)i && flag[i] == 0) ? 1 : 0;
}

// st[i] = (marker label, tref = i) or (0, 0); also detects value ties between non-marker neighbours
__global__ void __launch_bounds__(256) k_ws_init_state(const double *__restrict__ v, const int *__restrict__ parent,
                                                       const int *__restrict__ flag, const int *__restrict__ rank,
                                                       unsigned long long *__restrict__ st, int Y, int X, WsInfo *info)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= X) return;
    const int i = y * X + x;
    const int r = parent[i];
    const bool is_min = flag[r] == 0;
    st[i] = is_min ? pack_st(rank[r] + 1, i) : 0ULL;
    if (!is_min) {
        const double h = v[i];
        bool tie = false;
        if (x > 0 && v[i - 1] == h) tie = true;
        if (y > 0 && v[i - X] == h) tie = true;
        // ... and between non-marker pixels that SHARE a neighbour (diagonals, distance two): a lower pixel between them that is
        // enclosed by lines pops right after whichever of the two pops first ("pulled") and is then seen, or not, by the other
        auto nm_eq = [&](int j) { return v[j] == h && flag[parent[j]] != 0; };
        if (y > 0 && x > 0 && nm_eq(i - X - 1)) tie = true;
        if (y > 0 && x + 1 < X && nm_eq(i - X + 1)) tie = true;
        if (y > 1 && nm_eq(i - 2 * X)) tie = true;
        if (x > 1 && nm_eq(i - 2)) tie = true;
        if (tie) info->ties = 1;
    }
}

__global__ void __launch_bounds__(256) k_ws_emit(const unsigned long long *__restrict__ st, int32_t *__restrict__ out, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int l = st_lab(st[i]);
    out[i] = l > 0 ? l : 0;
}

__global__ void k_ws_info_init(WsInfo *info)
{
    info->emin = ~0ULL; info->emax = 0ULL; info->n_other = 0; info->ties = 0; info->n_markers = 0;
    info->changed = 0; info->undecided = 0; info->unfinished = 0;
    for (int q = 0; q < 64; ++q) info->changed_part[q] = 0;
    info->dbg_rounds = 0; info->dbg_tiles = 0; info->dbg_evals = 0; info->dbg_idle = 0; info->dbg_certs = 0;
    info->end_oversize = 0; info->end_unfinished = 0; info->ncomp = 0; info->ncells = 0; info->und_total = 0; info->front_total = 0;
    for (int q = 0; q < 64; ++q) info->end_part[q] = 0;
}

// tie landscapes that are not two-valued: the serial (value, age) heap replay (tip_ws_serial.hip) on the markers of the
// marker stage; one download of image + markers, one upload of the labels
static int flood_serial_exact(const double *img, const unsigned long long *st, int32_t *labels, int Y, int X)
{
    hipStream_t s = ctx().stream;
    const long n = (long)Y * X;
    TIP_LAUNCH("ws_emit", k_ws_emit, dim3(cdiv(n, 256)), dim3(256), 0, st, labels, n);
    std::vector<double> himg((size_t)n);
    std::vector<int32_t> hmark((size_t)n), hlab((size_t)n);
    TIP_HIP(hipMemcpyAsync(himg.data(), img, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    TIP_HIP(hipMemcpyAsync(hmark.data(), labels, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    TIP_HIP(hipStreamSynchronize(s));
    if (int rc = flood_exact(himg.data(), hmark.data(), hlab.data(), Y, X)) return rc;
    TIP_HIP(hipMemcpyAsync(labels, hlab.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    TIP_HIP(hipStreamSynchronize(s));   // the host vectors go out of scope
    return TIP_OK;
}

int watershed_dev(const double *img, int32_t *labels, int Y, int X, int wsl, int32_t *flags_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!img || !labels) return fail(TIP_ERR_ARG, "watershed: null pointer");
    if (!wsl) return fail(TIP_ERR_UNSUPPORTED, "watershed: only watershed_line=True (the reference's call sites)");
    if (Y < 1 || X < 1 || Y > 65535 || (long)Y * X > 2147483647L) return fail(TIP_ERR_ARG, "watershed: bad shape %dx%d", Y, X);
    const long n = (long)Y * X;
    WsScratch w;
    WsInfo *info = w.info = w.ws.get<WsInfo>(1);
    w.parent = w.ws.get<int>(n); w.flag = w.ws.get<int>(n); w.isroot = w.ws.get<int>(n); w.rank = w.ws.get<int>(n);
    w.st = w.ws.get<unsigned long long>(n);
    if (!info || !w.parent || !w.flag || !w.isroot || !w.rank || !w.st) return TIP_ERR_NOMEM;
    hipStream_t s = c.stream;
    TIP_LAUNCH("ws_info_init", k_ws_info_init, dim3(1), dim3(1), 0, info);
    TIP_LAUNCH("ws_minmax", k_ws_minmax, dim3(min(WS_RED_BLOCKS, cdiv(n, 256))), dim3(256), 0, img, n, info);
    TIP_LAUNCH("ws_count_other", k_ws_count_other, dim3(min(WS_RED_BLOCKS, cdiv(n, 256))), dim3(256), 0, img, n, info);
    // markers
    SameF64 same{img, info};
    int rc = uf_components(same, w.parent, Y, X);
    if (rc) return rc;
    TIP_HIP(hipMemsetAsync(w.flag, 0, n * sizeof(int), s));
    TIP_LAUNCH("ws_lower_flags", k_ws_lower_flags, dim3(cdiv(X, 256), Y), dim3(256), 0, img, (const int *)w.parent, w.flag, Y, X,
               (const WsInfo *)info);
    TIP_LAUNCH("ws_min_roots", k_ws_min_roots, dim3(cdiv(n, 256)), dim3(256), 0, (const int *)w.parent, (const int *)w.flag, w.isroot, n);
    if ((rc = exclusive_scan_i32(w.isroot, w.rank, n, &info->n_markers))) return rc;
    TIP_LAUNCH("ws_init_state", k_ws_init_state, dim3(cdiv(X, 256), Y), dim3(256), 0, img, (const int *)w.parent, (const int *)w.flag,
               (const int *)w.rank, w.st, Y, X, info);
    WsInfo h;
    TIP_HIP(hipMemcpyAsync(&h, info, sizeof h, hipMemcpyDeviceToHost, s));
    TIP_HIP(hipStreamSynchronize(s));
    c.last_ws_labels = h.n_markers;
    c.last_ws_other = (long)h.n_other;
    int flags = h.ties ? TIP_WS_FLAG_TIES : 0;
    const bool two_valued = h.n_other == 0 && h.emin != h.emax;
    if (h.n_markers > 0 && h.ties && !two_valued && tuning().ws_ties != 0) {
        flags |= TIP_WS_FLAG_SERIAL_EXACT;      // (writes the labels itself)
        if ((rc = flood_serial_exact(img, w.st, labels, Y, X))) return rc;
        if (flags_host) *flags_host = flags;
        return TIP_OK;
    }
    if (h.n_markers > 0 && two_valued) {
        flags |= TIP_WS_FLAG_TWO_VALUED;
        if ((rc = flood_two_valued(w, Y, X))) return rc;
    } else if (h.n_markers > 0) {
        long finished_serially = -1;
        if ((rc = flood_tiles(img, w, Y, X, &finished_serially))) return rc;
        if (finished_serially >= 0)
            flags |= TIP_WS_FLAG_SERIAL_FINISH | (int)(std::min<long>(finished_serially, 0x7fffff) << TIP_WS_FLAG_COUNT_SHIFT);
    }
    TIP_LAUNCH("ws_emit", k_ws_emit, dim3(cdiv(n, 256)), dim3(256), 0, (const unsigned long long *)w.st, labels, n);
    if (flags_host) *flags_host = flags;
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_last_watershed_labels(void) { return ctx().last_ws_labels; }

int tip_watershed_f64_dev(const double *img, int32_t *labels, int y, int x, int wsl, int32_t *flags_host)
{
    return watershed_dev(img, labels, y, x, wsl, flags_host);
}

int tip_watershed_f64(const double *img, int32_t *labels, int y, int x, int wsl, int32_t *flags)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!img || !labels || y < 1 || x < 1) return fail(TIP_ERR_ARG, "tip_watershed_f64: bad arguments");
    const size_t P = (size_t)y * x;
    WsGuard ws;
    double *di = ws.get<double>(P);
    int32_t *dl = ws.get<int32_t>(P);
    if (!di || !dl) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(di, img, P * 8, hipMemcpyHostToDevice, c.stream));
    int rc = watershed_dev(di, dl, y, x, wsl, flags);
    if (rc) return rc;
    TIP_HIP(hipMemcpyAsync(labels, dl, P * 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    return TIP_OK;
}

int tip_watershed_segmentation_f64_dev(const double *img, int32_t *labels, int y, int x, double imgthresh, const double *taps,
                                       int ntaps, int block, int32_t *flags_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!img || !labels || y < 1 || x < 1) return fail(TIP_ERR_ARG, "tip_watershed_segmentation_f64_dev: bad arguments");
    const size_t P = (size_t)y * x;
    WsGuard ws;
    double *a = ws.get<double>(P), *b = ws.get<double>(P);
    if (!a || !b) return TIP_ERR_NOMEM;
    int rc = tip_local_threshold_f64_dev(img, a, y, x, imgthresh, block);
    if (rc) return rc;
    if (taps && ntaps > 255) {
        // sigma > 31.8: more taps than a Taps holds; blur_image's route for them (taps in device memory, tip_gauss.hip)
        if ((rc = gaussian3d_dev(a, b, 1, 1, y, x, nullptr, 0, taps, ntaps, taps, ntaps))) return rc;
        return watershed_dev(b, labels, y, x, 1, flags_host);
    }
    if (taps && ntaps > 0) {
        Taps t;
        if ((rc = make_taps(t, taps, ntaps))) return rc;
        if ((rc = correlate1d_dev(a, b, 1, 1, y, x, 1, t, 0))) return rc;
        if ((rc = correlate1d_dev(b, a, 1, 1, y, x, 2, t, 0))) return rc;
    }
    return watershed_dev(a, labels, y, x, 1, flags_host);
}

}  // extern "C"
