// tip_hull.hip -- the sensory-region filter (ti.py:614-620 detect_non_sensory_region_cells, 2781-2792
// remove_cells_outside_of_sensory_region): the convex hull of the hair cells' centroids, the rows strictly outside it, and 255 on
// their pixels.  Upstream triangulates (scipy.spatial.Delaunay) and asks find_simplex; the union of a Delaunay triangulation's
// simplices IS the convex hull, so hull + point-in-convex-polygon answers the same question.  Every geometric decision is
// orient() of tip_orient.h (exact sign), so no tolerance enters.  DESIGN.md 5.13 has the argument and the contract with scipy.
//
//   k_hull_extremes  the eight extremes of x, y, x + y, x - y over the points that take part (finite, and selected when a
//                    selection is given): a grid-stride pass, block_reduce of (key, index) per extreme, one partial row per block
//   k_hull_octagon   one workgroup: the partial rows reduced, the extremes' coordinates in counter-clockwise order W, SW, S, SE, E,
//                    NE, N, NW with consecutive coincident corners merged -- a closed chain through input points.  x + y and x - y are
//                    rounded sums, so a corner need not be a true extreme; the filter below does not need it to be.
//   k_hull_filter    a point strictly to the left of EVERY edge of that chain sees each edge under an angle in (0, pi); the angles
//                    add up to a positive multiple of 2 pi, so the chain winds round the point, which therefore lies strictly inside
//                    the hull of the chain's corners and is no vertex: dropped.  Everything else survives and is compacted
//                    (block_exclusive_scan inside the workgroup, one atomic per workgroup for its base -- the order among
//                    workgroups is not fixed, the sort below fixes it).  Fewer than three distinct corners: nothing is dropped.
//   k_hull_pad, k_hull_sort_chunk, k_hull_sort_step
//                    bitonic sort of the survivors by (x, y, index), padded to a power of two with +inf keys: the steps with a
//                    partner inside a 2048-entry chunk run in LDS (one launch for all of them), the others one launch each.
//   k_hull_tangent   one thread per sorted survivor p, the others streamed through LDS tiles.  L = the survivors before p, R = those
//                    after it (coincident ones skipped): each lies in a half-open half-plane of p, where orient(p, ., .) is a total
//                    preorder of directions, so four running tangent points -- upper and lower, left and right -- are a reduction in
//                    any order.  p is a vertex of the lower chain iff orient(l_lo, p, r_lo) > 0, of the upper chain iff
//                    orient(l_up, p, r_up) < 0, both STRICT: a point on an edge is no vertex.  The first survivor, and the first of
//                    the lexicographically largest, have no L or no R and are vertices; a survivor that repeats its predecessor's
//                    coordinates never is (the lowest index stands for all).  Work O(s^2 / lanes) over the s survivors, so
//                    hull_launch refuses s > H_MAX_SURVIVORS (TIP_ERR_UNSUPPORTED) instead of running one launch for seconds.
//   k_hull_emit      one workgroup: counts the flags, then writes the lower chain ascending and the upper chain descending
//                    (block_exclusive_scan per 256 survivors) -- counter-clockwise from the lexicographically smallest vertex.
//                    Nothing is written when the hull has fewer than 3 vertices or more than the caller's capacity.
//   k_hull_outside   one thread per query: the fan from vertex 0 by binary search over orient(v0, v_k, q), then one edge test;
//                    O(log h) exact predicates a query.  Outside means strictly outside.
//   k_hull_invalidate  types[p] = 255 where 1 <= labels[p] <= n and outside[labels[p] - 1].
// Every index read from memory is checked before it is used, every write against its capacity.
#include <cmath>
#include <vector>
#include <algorithm>
#include "tip_internal.h"
#include "tip_orient.h"

namespace tip {

constexpr int H_BLOCK = 256, H_WAVES = H_BLOCK / 64, H_CHUNK = 2048, H_MAX_PARTIAL = 1024;
constexpr long H_MAX_SURVIVORS = 65536;      // k_hull_tangent is quadratic in the survivors: 4.3e9 point pairs at the limit
constexpr double H_INF = __builtin_huge_val();

struct HullSel { const uint8_t *type, *valid, *empty; };      // type NULL: every point takes part
struct HullExt { double v; int idx; int pad; };
struct HullState { int n_surv, n_hull, oct_n, pad; double ox[8], oy[8]; };

TIP_HD inline bool hull_selected(const HullSel &sel, long i)
{
    return !sel.type || (sel.type[i] == 1 && sel.valid[i] == 1 && (!sel.empty || sel.empty[i] == 0));
}
__device__ __forceinline__ bool hull_takes(const HullSel &sel, long i, double x, double y)
{
    return isfinite(x) && isfinite(y) && hull_selected(sel, i);
}
__device__ __forceinline__ HullExt ext_min(HullExt a, HullExt b)
{
    return (b.v < a.v || (b.v == a.v && (unsigned)b.idx < (unsigned)a.idx)) ? b : a;
}

__global__ void __launch_bounds__(H_BLOCK) k_hull_extremes(const double *__restrict__ px, const double *__restrict__ py, long n, HullSel sel,
                                                           HullExt *__restrict__ partial)
{
    __shared__ HullExt wv[8][H_WAVES];
    HullExt best[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) best[e] = {H_INF, -1, 0};
    for (long i = (long)blockIdx.x * H_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * H_BLOCK) {
        const double x = px[i], y = py[i];
        if (!hull_takes(sel, i, x, y)) continue;
        const double s = x + y, d = x - y;
        const double key[8] = {x, s, y, -d, -x, -s, -y, d};      // W, SW, S, SE, E, NE, N, NW as minima
#pragma unroll
        for (int e = 0; e < 8; ++e) best[e] = ext_min(best[e], HullExt{key[e], (int)i, 0});
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const HullExt r = block_reduce<H_WAVES>(best[e], wv[e], ext_min);
        if (threadIdx.x == 0) partial[(long)blockIdx.x * 8 + e] = r;
    }
}

__global__ void __launch_bounds__(H_BLOCK) k_hull_octagon(const HullExt *__restrict__ partial, int nb, const double *__restrict__ px,
                                                          const double *__restrict__ py, long n, HullState *__restrict__ st)
{
    __shared__ HullExt wv[8][H_WAVES];
    __shared__ int corner[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        HullExt b = {H_INF, -1, 0};
        for (int j = threadIdx.x; j < nb; j += H_BLOCK) b = ext_min(b, partial[(long)j * 8 + e]);
        b = block_reduce<H_WAVES>(b, wv[e], ext_min);
        if (threadIdx.x == 0) corner[e] = b.idx;
    }
    if (threadIdx.x != 0) return;
    int m = 0;
    for (int e = 0; e < 8; ++e) {
        const int i = corner[e];
        if (i < 0 || i >= n) continue;
        const double x = px[i], y = py[i];
        if (m && st->ox[m - 1] == x && st->oy[m - 1] == y) continue;
        st->ox[m] = x, st->oy[m] = y, ++m;
    }
    if (m > 1 && st->ox[m - 1] == st->ox[0] && st->oy[m - 1] == st->oy[0]) --m;
    st->oct_n = m >= 3 ? m : 0;
    st->n_surv = 0;
    st->n_hull = 0;
}

__global__ void __launch_bounds__(H_BLOCK) k_hull_filter(const double *__restrict__ px, const double *__restrict__ py, long n, HullSel sel,
                                                         HullState *__restrict__ st, double *__restrict__ sx, double *__restrict__ sy,
                                                         int *__restrict__ si, long cap)
{
    __shared__ int wsum[H_WAVES];
    __shared__ int base;
    const long i = (long)blockIdx.x * H_BLOCK + threadIdx.x;
    const int m = st->oct_n <= 8 ? st->oct_n : 0;
    double x = 0.0, y = 0.0;
    int keep = 0;
    if (i < n) {
        x = px[i], y = py[i];
        if (hull_takes(sel, i, x, y)) {
            bool inside = m >= 3;
            for (int e = 0; e < m && inside; ++e) {
                const int f = e + 1 < m ? e + 1 : 0;
                inside = orient(st->ox[e], st->oy[e], st->ox[f], st->oy[f], x, y) > 0;
            }
            keep = inside ? 0 : 1;
        }
    }
    int total;
    const int before = block_exclusive_scan<H_WAVES>(keep, wsum, total);
    if (threadIdx.x == 0) base = total ? atomicAdd(&st->n_surv, total) : 0;
    __syncthreads();
    const long pos = (long)base + before;
    if (keep && pos < cap) sx[pos] = x, sy[pos] = y, si[pos] = (int)i;
}

__global__ void __launch_bounds__(H_BLOCK) k_hull_pad(double *__restrict__ sx, double *__restrict__ sy, int *__restrict__ si, long s, long s_pad)
{
    const long i = s + (long)blockIdx.x * H_BLOCK + threadIdx.x;
    if (i < s_pad) sx[i] = H_INF, sy[i] = H_INF, si[i] = 0x7fffffff;
}

// every step (k, j) with j < chunk of the bitonic network, k = k_from .. k_to, on one chunk (a power of two <= H_CHUNK) in LDS
__global__ void __launch_bounds__(H_BLOCK) k_hull_sort_chunk(double *__restrict__ sx, double *__restrict__ sy, int *__restrict__ si, int chunk,
                                                             long k_from, long k_to)
{
    __shared__ double lx[H_CHUNK], ly[H_CHUNK];
    __shared__ int li[H_CHUNK];
    const long base = (long)blockIdx.x * chunk;
    for (int t = threadIdx.x; t < chunk; t += H_BLOCK) lx[t] = sx[base + t], ly[t] = sy[base + t], li[t] = si[base + t];
    __syncthreads();
    for (long k = k_from; k <= k_to; k <<= 1)
        for (int j = (int)(k / 2 < chunk / 2 ? k / 2 : chunk / 2); j >= 1; j >>= 1) {
            for (int t = threadIdx.x; t < chunk / 2; t += H_BLOCK) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const bool asc = ((base + a) & k) == 0;
                if (asc ? lex_less(lx[b], ly[b], li[b], lx[a], ly[a], li[a]) : lex_less(lx[a], ly[a], li[a], lx[b], ly[b], li[b])) {
                    const double tx = lx[a], ty = ly[a];
                    const int ti = li[a];
                    lx[a] = lx[b], ly[a] = ly[b], li[a] = li[b];
                    lx[b] = tx, ly[b] = ty, li[b] = ti;
                }
            }
            __syncthreads();
        }
    for (int t = threadIdx.x; t < chunk; t += H_BLOCK) sx[base + t] = lx[t], sy[base + t] = ly[t], si[base + t] = li[t];
}

// one step (k, j) with the partner in another chunk
__global__ void __launch_bounds__(H_BLOCK) k_hull_sort_step(double *__restrict__ sx, double *__restrict__ sy, int *__restrict__ si, long s_pad,
                                                            long k, long j)
{
    const long t = (long)blockIdx.x * H_BLOCK + threadIdx.x;
    if (t >= s_pad / 2) return;
    const long a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
    const bool asc = (a & k) == 0;
    const double ax = sx[a], ay = sy[a], bx = sx[b], by = sy[b];
    const int ai = si[a], bi = si[b];
    if (asc ? lex_less(bx, by, bi, ax, ay, ai) : lex_less(ax, ay, ai, bx, by, bi)) {
        sx[a] = bx, sy[a] = by, si[a] = bi;
        sx[b] = ax, sy[b] = ay, si[b] = ai;
    }
}

__global__ void __launch_bounds__(H_BLOCK) k_hull_tangent(const double *__restrict__ sx, const double *__restrict__ sy, long s,
                                                          uint8_t *__restrict__ lower, uint8_t *__restrict__ upper)
{
    __shared__ double tx[H_BLOCK], ty[H_BLOCK];
    const long i = (long)blockIdx.x * H_BLOCK + threadIdx.x;
    const bool live = i < s;
    const double x = live ? sx[i] : 0.0, y = live ? sy[i] : 0.0;
    bool has_l = false, has_r = false;
    double lux = 0, luy = 0, llx = 0, lly = 0, rux = 0, ruy = 0, rlx = 0, rly = 0;
    for (long t0 = 0; t0 < s; t0 += H_BLOCK) {
        __syncthreads();
        if (t0 + threadIdx.x < s) tx[threadIdx.x] = sx[t0 + threadIdx.x], ty[threadIdx.x] = sy[t0 + threadIdx.x];
        __syncthreads();
        const int cnt = (int)(s - t0 < H_BLOCK ? s - t0 : H_BLOCK);
        if (!live) continue;
        for (int k = 0; k < cnt; ++k) {
            const double qx = tx[k], qy = ty[k];
            if (qx == x && qy == y) continue;
            if (t0 + k < i) {
                if (!has_l) { lux = llx = qx, luy = lly = qy, has_l = true; continue; }
                if (orient(x, y, lux, luy, qx, qy) < 0) lux = qx, luy = qy;
                if (orient(x, y, llx, lly, qx, qy) > 0) llx = qx, lly = qy;
            } else {
                if (!has_r) { rux = rlx = qx, ruy = rly = qy, has_r = true; continue; }
                if (orient(x, y, rux, ruy, qx, qy) > 0) rux = qx, ruy = qy;
                if (orient(x, y, rlx, rly, qx, qy) < 0) rlx = qx, rly = qy;
            }
        }
    }
    if (!live) return;
    const bool dup = i > 0 && sx[i - 1] == x && sy[i - 1] == y;
    bool lo = false, up = false;
    if (!dup) {
        if (!has_l || !has_r) lo = true;
        else {
            lo = orient(llx, lly, x, y, rlx, rly) > 0;
            up = !lo && orient(lux, luy, x, y, rux, ruy) < 0;
        }
    }
    lower[i] = lo ? 1 : 0;
    upper[i] = up ? 1 : 0;
}

__global__ void __launch_bounds__(H_BLOCK) k_hull_emit(const uint8_t *__restrict__ lower, const uint8_t *__restrict__ upper,
                                                       const int *__restrict__ si, long s, int *__restrict__ hull, long cap,
                                                       HullState *__restrict__ st)
{
    __shared__ int wsum[H_WAVES];
    int mine = 0;
    for (long i = threadIdx.x; i < s; i += H_BLOCK) mine += lower[i] + upper[i];
    const int h = block_sum<H_WAVES>(mine, wsum);
    if (threadIdx.x == 0) st->n_hull = h;
    if (h < 3 || h > cap) return;                      // (the same on every thread)
    long at = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const uint8_t *flag = pass ? upper : lower;
        for (long c0 = 0; c0 < s; c0 += H_BLOCK) {
            __syncthreads();                           // (wsum is written again)
            const long k = c0 + threadIdx.x, i = pass ? s - 1 - k : k;
            const int v = k < s ? flag[i] : 0;
            int total;
            const int before = block_exclusive_scan<H_WAVES>(v, wsum, total);
            if (v && at + before < cap) hull[at + before] = si[i];
            at += total;
        }
    }
}

// h: from *h_dev when given (a hull this call has just built: unusable when < 3 or above cap), else h_val
__global__ void __launch_bounds__(H_BLOCK) k_hull_outside(const double *__restrict__ px, const double *__restrict__ py, long n,
                                                          const int *__restrict__ hull, const int *__restrict__ h_dev, long h_val, long cap,
                                                          const double *__restrict__ qx, const double *__restrict__ qy, long m,
                                                          uint8_t *__restrict__ out)
{
    const long q = (long)blockIdx.x * H_BLOCK + threadIdx.x;
    if (q >= m) return;
    const long h = h_dev ? (long)*h_dev : h_val;
    if (h < 3 || h > cap) { out[q] = 0; return; }
    const double x = qx[q], y = qy[q];
    auto vx = [&](long k, double &vx_, double &vy_) {
        const int i = hull[k];
        const bool ok = i >= 0 && i < n;
        vx_ = ok ? px[i] : 0.0, vy_ = ok ? py[i] : 0.0;
        return ok;
    };
    double x0, y0, ax, ay, bx, by;
    bool ok = vx(0, x0, y0) & vx(1, ax, ay) & vx(h - 1, bx, by);
    if (!ok) { out[q] = 0; return; }
    if (orient(x0, y0, ax, ay, x, y) < 0 || orient(x0, y0, bx, by, x, y) > 0) { out[q] = 1; return; }
    long lo = 1, hi = h - 1;
    while (hi - lo > 1) {
        const long mid = lo + (hi - lo) / 2;
        ok &= vx(mid, ax, ay);
        if (orient(x0, y0, ax, ay, x, y) >= 0) lo = mid;
        else hi = mid;
    }
    ok &= vx(lo, ax, ay) & vx(lo + 1, bx, by);
    out[q] = ok && orient(ax, ay, bx, by, x, y) < 0 ? 1 : 0;
}

__global__ void __launch_bounds__(H_BLOCK) k_hull_invalidate(const int32_t *__restrict__ labels, uint8_t *__restrict__ types, long n_pix,
                                                             const uint8_t *__restrict__ outside, long n, const int *__restrict__ h_dev,
                                                             long cap)
{
    const long p = (long)blockIdx.x * H_BLOCK + threadIdx.x;
    if (p >= n_pix) return;
    if (h_dev && (*h_dev < 3 || *h_dev > cap)) return;
    const int l = labels[p];
    if (l >= 1 && l <= n && outside[l - 1]) types[p] = 255;
}

// ---- launches on device arrays --------------------------------------------------------------------------------------------------
// The hull of the n points that take part, into hull (capacity cap) with its size in st->n_hull, all on the device.  Waits for the
// stream ONCE, to size the sort by the survivor count (pin: 4 pinned bytes); the caller waits again for the count.
static int hull_launch(const double *px, const double *py, long n, const HullSel &sel, int *hull, long cap, HullState *st, int *pin)
{
    Ctx &c = ctx();
    WsGuard ws;
    const int nb = (int)std::min<long>(std::max<long>(cdiv(n, 4 * H_BLOCK), 1), H_MAX_PARTIAL);
    long cap_s = 1;
    while (cap_s < n) cap_s <<= 1;
    HullExt *partial = ws.get<HullExt>((size_t)nb * 8);
    double *sx = ws.get<double>((size_t)cap_s), *sy = ws.get<double>((size_t)cap_s);
    int *si = ws.get<int>((size_t)cap_s);
    if (!partial || !sx || !sy || !si) return TIP_ERR_NOMEM;
    TIP_LAUNCH("hull_extremes", k_hull_extremes, dim3(nb), dim3(H_BLOCK), 0, px, py, n, sel, partial);
    TIP_LAUNCH("hull_octagon", k_hull_octagon, dim3(1), dim3(H_BLOCK), 0, (const HullExt *)partial, nb, px, py, n, st);
    TIP_LAUNCH("hull_filter", k_hull_filter, dim3(cdiv(n, H_BLOCK)), dim3(H_BLOCK), 0, px, py, n, sel, st, sx, sy, si, n);
    TIP_HIP(hipMemcpyAsync(pin, &st->n_surv, 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    const long s = *pin;
    if (s < 0 || s > n) return fail(TIP_ERR_HIP, "hull: %ld survivors of %ld points", s, n);
    if (s == 0) return TIP_OK;                          // (st->n_hull is 0)
    if (s > H_MAX_SURVIVORS)
        return fail(TIP_ERR_UNSUPPORTED, "hull: %ld of %ld points survive the octagon filter; the tangent test takes at most %ld", s, n,
                    H_MAX_SURVIVORS);
    long s_pad = 1;
    while (s_pad < s) s_pad <<= 1;
    const int chunk = (int)std::min<long>(s_pad, H_CHUNK);
    if (s_pad > s) TIP_LAUNCH("hull_pad", k_hull_pad, dim3(cdiv(s_pad - s, H_BLOCK)), dim3(H_BLOCK), 0, sx, sy, si, s, s_pad);
    if (s_pad > 1) TIP_LAUNCH("hull_sort_chunk", k_hull_sort_chunk, dim3((unsigned)(s_pad / chunk)), dim3(H_BLOCK), 0, sx, sy, si, chunk, 2L, (long)chunk);
    for (long k = 2L * chunk; k <= s_pad; k <<= 1) {
        for (long j = k / 2; j >= chunk; j >>= 1)
            TIP_LAUNCH("hull_sort_step", k_hull_sort_step, dim3(cdiv(s_pad / 2, H_BLOCK)), dim3(H_BLOCK), 0, sx, sy, si, s_pad, k, j);
        TIP_LAUNCH("hull_sort_chunk", k_hull_sort_chunk, dim3((unsigned)(s_pad / chunk)), dim3(H_BLOCK), 0, sx, sy, si, chunk, k, k);
    }
    uint8_t *lower = ws.get<uint8_t>((size_t)s), *upper = ws.get<uint8_t>((size_t)s);
    if (!lower || !upper) return TIP_ERR_NOMEM;
    TIP_LAUNCH("hull_tangent", k_hull_tangent, dim3(cdiv(s, H_BLOCK)), dim3(H_BLOCK), 0, (const double *)sx, (const double *)sy, s, lower, upper);
    TIP_LAUNCH("hull_emit", k_hull_emit, dim3(1), dim3(H_BLOCK), 0, (const uint8_t *)lower, (const uint8_t *)upper, (const int *)si, s, hull, cap, st);
    return TIP_OK;
}

static int outside_launch(const double *px, const double *py, long n, const int *hull, const int *h_dev, long h, long cap, const double *qx,
                          const double *qy, long m, uint8_t *out)
{
    if (m == 0) return TIP_OK;
    TIP_LAUNCH("hull_outside", k_hull_outside, dim3(cdiv(m, H_BLOCK)), dim3(H_BLOCK), 0, px, py, n, hull, h_dev, h, cap, qx, qy, m, out);
    return TIP_OK;
}

// ---- the same on the host: Andrew's monotone chain and the edge-by-edge test, with the kernels' predicate -----------------------
static void hull_host(const double *px, const double *py, long n, const HullSel &sel, std::vector<int> &hull)
{
    std::vector<int> ord;
    for (long i = 0; i < n; ++i)
        if (std::isfinite(px[i]) && std::isfinite(py[i]) && hull_selected(sel, i)) ord.push_back((int)i);
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return lex_less(px[a], py[a], a, px[b], py[b], b); });
    ord.erase(std::unique(ord.begin(), ord.end(), [&](int a, int b) { return px[a] == px[b] && py[a] == py[b]; }), ord.end());
    hull.clear();
    const long s = (long)ord.size();
    if (s < 3) { hull = ord; return; }
    auto turn = [&](int a, int b, int p) { return orient(px[a], py[a], px[b], py[b], px[p], py[p]); };
    for (long i = 0; i < s; ++i) {                      // lower chain
        while (hull.size() >= 2 && turn(hull[hull.size() - 2], hull.back(), ord[i]) <= 0) hull.pop_back();
        hull.push_back(ord[i]);
    }
    const size_t low = hull.size() + 1;
    for (long i = s - 2; i >= 0; --i) {                 // upper chain
        while (hull.size() >= low && turn(hull[hull.size() - 2], hull.back(), ord[i]) <= 0) hull.pop_back();
        hull.push_back(ord[i]);
    }
    hull.pop_back();                                    // (the start again)
}

static bool outside_host(const double *px, const double *py, const std::vector<int> &hull, double x, double y)
{
    const size_t h = hull.size();
    for (size_t k = 0; k < h; ++k) {
        const int a = hull[k], b = hull[k + 1 < h ? k + 1 : 0];
        if (orient(px[a], py[a], px[b], py[b], x, y) < 0) return true;
    }
    return false;
}

static int check_points(const char *who, const double *px, const double *py, int64_t n, bool host)
{
    if (n < 0 || n > (1L << 30)) return fail(TIP_ERR_ARG, "%s: n = %ld points", who, (long)n);
    if (n > 0 && (!px || !py)) return fail(TIP_ERR_ARG, "%s: the coordinates", who);
    if (host)
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(px[i]) || !std::isfinite(py[i])) return fail(TIP_ERR_ARG, "%s: point %ld has a non-finite coordinate", who, (long)i);
    return TIP_OK;
}

static int hull_verdict(const char *who, long h, long cap)
{
    if (h < 3) return fail(TIP_ERR_DEGENERATE, "%s: no hull -- fewer than three distinct points, or all on one line (%ld vertices)", who, h);
    if (h > cap) return fail(TIP_ERR_OVERFLOW, "%s: the hull has %ld vertices, capacity %ld", who, h, cap);
    return TIP_OK;
}

static int check_hull_list(const char *who, const int32_t *hull, int64_t h, int64_t n)
{
    if (h < 3 || h > n || !hull) return fail(TIP_ERR_ARG, "%s: a hull of %ld vertices over %ld points", who, (long)h, (long)n);
    for (int64_t k = 0; k < h; ++k)
        if (hull[k] < 0 || hull[k] >= n) return fail(TIP_ERR_ARG, "%s: hull[%ld] = %d of %ld points", who, (long)k, hull[k], (long)n);
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_convex_hull_f64_dev(const double *px, const double *py, int64_t n, int32_t *hull, int64_t cap, int64_t *n_hull_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_points("tip_convex_hull_f64_dev", px, py, n, false)) return rc;
    if (cap < 0 || (cap > 0 && !hull) || !n_hull_host) return fail(TIP_ERR_ARG, "tip_convex_hull_f64_dev: the hull list, its capacity, n_hull");
    *n_hull_host = 0;
    if (n == 0) return hull_verdict("tip_convex_hull_f64_dev", 0, cap);
    WsGuard ws;
    HullState *st = ws.get<HullState>(1);
    int *pin = (int *)pinned_scratch(8);
    if (!st || !pin) return TIP_ERR_NOMEM;
    if (int rc = hull_launch(px, py, n, HullSel{nullptr, nullptr, nullptr}, hull, cap, st, pin)) return rc;
    TIP_HIP(hipMemcpyAsync(pin, &st->n_hull, 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    *n_hull_host = *pin;
    return hull_verdict("tip_convex_hull_f64_dev", *pin, cap);
}

int tip_convex_hull_f64(const double *px, const double *py, int64_t n, int32_t *hull, int64_t cap, int64_t *n_hull)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_points("tip_convex_hull_f64", px, py, n, true)) return rc;
    if (cap < 0 || (cap > 0 && !hull) || !n_hull) return fail(TIP_ERR_ARG, "tip_convex_hull_f64: the hull list, its capacity, n_hull");
    *n_hull = 0;
    if (n == 0) return hull_verdict("tip_convex_hull_f64", 0, cap);
    Staging stg;
    const double *dx = stg.in(px, (size_t)n), *dy = stg.in(py, (size_t)n);
    int32_t *dh = stg.scratch<int32_t>((size_t)std::max<int64_t>(cap, 1));
    HullState *st = stg.scratch<HullState>(1);
    int *pin = (int *)pinned_scratch(8);
    if (stg.rc) return stg.rc;
    if (!pin) return TIP_ERR_NOMEM;
    if (int rc = hull_launch(dx, dy, n, HullSel{nullptr, nullptr, nullptr}, dh, cap, st, pin)) return rc;
    TIP_HIP(hipMemcpyAsync(pin, &st->n_hull, 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    const long h = *pin;
    *n_hull = h;
    if (int rc = hull_verdict("tip_convex_hull_f64", h, cap)) return rc;
    TIP_HIP(hipMemcpyAsync(hull, dh, (size_t)h * 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    return TIP_OK;
}

int tip_points_outside_hull_f64_dev(const double *px, const double *py, int64_t n, const int32_t *hull, int64_t h, const double *qx,
                                    const double *qy, int64_t m, uint8_t *outside)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_points("tip_points_outside_hull_f64_dev", px, py, n, false)) return rc;
    if (h < 3 || h > n || !hull) return fail(TIP_ERR_ARG, "tip_points_outside_hull_f64_dev: a hull of %ld vertices over %ld points", (long)h, (long)n);
    if (m < 0 || m > (1L << 40) || (m > 0 && (!qx || !qy || !outside))) return fail(TIP_ERR_ARG, "tip_points_outside_hull_f64_dev: m = %ld queries", (long)m);
    return outside_launch(px, py, n, hull, nullptr, h, h, qx, qy, m, outside);
}

int tip_points_outside_hull_f64(const double *px, const double *py, int64_t n, const int32_t *hull, int64_t h, const double *qx,
                                const double *qy, int64_t m, uint8_t *outside)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_points("tip_points_outside_hull_f64", px, py, n, true)) return rc;
    if (int rc = check_hull_list("tip_points_outside_hull_f64", hull, h, n)) return rc;
    if (m < 0 || (m > 0 && (!qx || !qy || !outside))) return fail(TIP_ERR_ARG, "tip_points_outside_hull_f64: m = %ld queries", (long)m);
    if (int rc = check_points("tip_points_outside_hull_f64", qx, qy, m, true)) return rc;
    if (m == 0) return TIP_OK;
    Staging stg;
    const double *dx = stg.in(px, (size_t)n), *dy = stg.in(py, (size_t)n), *dqx = stg.in(qx, (size_t)m), *dqy = stg.in(qy, (size_t)m);
    const int32_t *dh = stg.in(hull, (size_t)h);
    uint8_t *dout = stg.out(outside, (size_t)m);
    if (stg.rc) return stg.rc;
    if (int rc = outside_launch(dx, dy, n, dh, nullptr, h, h, dqx, dqy, m, dout)) return rc;
    return stg.finish();
}

int tip_invalidate_cells_u8_dev(const int32_t *labels, uint8_t *types, int64_t n_pix, const uint8_t *outside, int64_t n)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (n_pix < 0 || n < 0 || n > 0x7fffffff || (n_pix > 0 && (!labels || !types)) || (n > 0 && !outside))
        return fail(TIP_ERR_ARG, "tip_invalidate_cells_u8_dev: %ld pixels, %ld rows, or a null pointer", (long)n_pix, (long)n);
    if (n_pix == 0 || n == 0) return TIP_OK;
    TIP_LAUNCH("hull_invalidate", k_hull_invalidate, dim3(cdiv(n_pix, H_BLOCK)), dim3(H_BLOCK), 0, labels, types, (long)n_pix, outside, (long)n,
               (const int *)nullptr, 0L);
    return TIP_OK;
}

static int check_rows(const char *who, const double *cx, const double *cy, const uint8_t *type, const uint8_t *valid, int64_t n,
                      const int32_t *hull, int64_t hull_cap, const int64_t *n_hull)
{
    if (int rc = check_points(who, cx, cy, n, true)) return rc;
    if ((type == nullptr) != (valid == nullptr)) return fail(TIP_ERR_ARG, "%s: type and valid come together (both NULL: every row is a hull point)", who);
    if (hull_cap < 0 || (hull_cap > 0 && !hull) || !n_hull) return fail(TIP_ERR_ARG, "%s: the hull list, its capacity, n_hull", who);
    return TIP_OK;
}

int tip_sensory_region_i32_dev(const int32_t *labels, uint8_t *types, int64_t n_pix, const double *cx, const double *cy,
                               const uint8_t *type, const uint8_t *valid, const uint8_t *empty, int64_t n, uint8_t *outside, int32_t *hull,
                               int64_t hull_cap, int64_t *n_hull)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    const char *who = "tip_sensory_region_i32_dev";
    if (int rc = check_rows(who, cx, cy, type, valid, n, hull, hull_cap, n_hull)) return rc;
    if (n_pix < 0 || ((labels == nullptr) != (types == nullptr)) || (n > 0 && !outside))
        return fail(TIP_ERR_ARG, "%s: the label map and the type map come together; outside has n entries", who);
    *n_hull = 0;
    if (n == 0) return hull_verdict(who, 0, hull_cap);
    // one pinned block, one upload [cx | cy | type | valid | empty], one download [n_hull, pad | hull | outside]
    const size_t N = (size_t)n, in_bytes = 16 * N + 3 * N, hull_at = 8, out_at = hull_at + 4 * (size_t)hull_cap, out_bytes = out_at + N;
    const size_t in_room = (in_bytes + 15) & ~(size_t)15;
    uint8_t *pin = (uint8_t *)pinned_scratch(16 + in_room + out_bytes);
    WsGuard ws;
    uint8_t *din = ws.get<uint8_t>(in_bytes), *dout = ws.get<uint8_t>(out_bytes);
    HullState *st = ws.get<HullState>(1);
    if (!pin || !din || !dout || !st) return TIP_ERR_NOMEM;
    uint8_t *hin = pin + 16, *hout = pin + 16 + in_room;
    memcpy(hin, cx, 8 * N);
    memcpy(hin + 8 * N, cy, 8 * N);
    if (type) memcpy(hin + 16 * N, type, N), memcpy(hin + 17 * N, valid, N);
    if (type && empty) memcpy(hin + 18 * N, empty, N);
    TIP_HIP(hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, c.stream));
    const double *dcx = (const double *)din, *dcy = dcx + N;
    const HullSel sel = {type ? din + 16 * N : nullptr, type ? din + 17 * N : nullptr, type && empty ? din + 18 * N : nullptr};
    int *dhull = (int *)(dout + hull_at);
    uint8_t *doutside = dout + out_at;
    if (int rc = hull_launch(dcx, dcy, n, sel, dhull, hull_cap, st, (int *)pin)) return rc;
    if (int rc = outside_launch(dcx, dcy, n, dhull, &st->n_hull, 0, hull_cap, dcx, dcy, n, doutside)) return rc;
    if (labels && n_pix)
        TIP_LAUNCH("hull_invalidate", k_hull_invalidate, dim3(cdiv(n_pix, H_BLOCK)), dim3(H_BLOCK), 0, labels, types, (long)n_pix,
                   (const uint8_t *)doutside, (long)n, (const int *)&st->n_hull, (long)hull_cap);
    TIP_HIP(hipMemcpyAsync(dout, &st->n_hull, 4, hipMemcpyDeviceToDevice, c.stream));
    TIP_HIP(hipMemcpyAsync(hout, dout, out_bytes, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    const long h = *(const int *)hout;
    *n_hull = h;
    if (int rc = hull_verdict(who, h, hull_cap)) return rc;
    memcpy(hull, hout + hull_at, (size_t)h * 4);
    memcpy(outside, hout + out_at, N);
    return TIP_OK;
}

int tip_sensory_region_host(const double *cx, const double *cy, const uint8_t *type, const uint8_t *valid, const uint8_t *empty, int64_t n,
                            uint8_t *outside, int32_t *hull, int64_t hull_cap, int64_t *n_hull)
{
    const char *who = "tip_sensory_region_host";
    if (int rc = check_rows(who, cx, cy, type, valid, n, hull, hull_cap, n_hull)) return rc;
    std::vector<int> hv;
    hull_host(cx, cy, n, HullSel{type, valid, type ? empty : nullptr}, hv);
    *n_hull = (int64_t)hv.size();
    if (int rc = hull_verdict(who, (long)hv.size(), hull_cap)) return rc;
    std::copy(hv.begin(), hv.end(), hull);
    if (outside)
        for (int64_t i = 0; i < n; ++i) outside[i] = outside_host(cx, cy, hv, cx[i], cy[i]) ? 1 : 0;
    return TIP_OK;
}

}  // extern "C"
