// tip_order.hip -- hexatic order: the Delaunay neighbours of the cell centroids (ti.py:2545-2560,
// find_nearest_neighbors_using_voroni_tesselation), psi_n over a list of neighbour sets (ti.py:2563-2583 calc_psin) and the two
// per-row columns behind calculate_neighbors_correlation_function (ti.py:803-843; their kernel, k_neighbor_state, walks the
// neighbour CSR and lives in tip_graph.hip).  DESIGN.md 5.8 has the argument.
//
//   point_grid_launch (tip_grid.h; launched as "order_grid" / "order_count" / "csr_scan" / "order_fill")
//                    the uniform grid over the bounding box of the finite points, first cell side about two points per square
//                    cell; the points (x, y, position) copied cell by cell -- the points of the cells x0 .. x1 of one grid row are
//                    one contiguous range (rect_row).  A point with a non-finite coordinate takes no part.
//   k_delaunay       one wavefront (one 64-thread workgroup) per point i.  Candidates are the points of the cells within r cells
//                    of i's cell (r = 2, 4, 8, ...); the lanes stride over the candidates j, and for each j the interval test
//                    runs over the candidates k:   a = p_j - p_i, b = p_k - p_i,   s = a.x b.y - a.y b.x,
//                    t = (|b|^2 - a.b) / (2 s);   hi = min t over s > 0, lo = max t over s < 0;   s == 0 kills the pair when
//                    |b|^2 - a.b < 0 (k strictly between the two);   (i, j) is an edge iff lo < hi.  Every operation is an
//                    explicitly rounded one (__dsub_rn / __dmul_rn / __dadd_rn / __ddiv_rn), min and max do not depend on the
//                    order of the k, and a lane stops early once lo >= hi -- so the decision is the one the numpy restatement
//                    (tests/order_restate.py) takes over ALL k whenever the ring is certified:  with R the largest distance from
//                    p_i to an end of an accepted edge's interval (the farthest vertex of the cell the candidates leave),
//                    2 R <= r h means no point outside the ring can cut the cell.  Otherwise r doubles; an unbounded cell (a hull
//                    point) ends with the whole grid.  A candidate list of at most O_CAP points is held in LDS; a longer one
//                    streams from global memory, each j first against the last list that did fit (nearly every far j dies there).
//                    The certified sweep is repeated to write the members (two-call convention: sizes, the caller's scan,
//                    members), unsorted into a scratch row that k_rank_sort (tip_csr.h: row_rank; launched as "order_row_sort")
//                    ranks into ascending order.  No degree cap.
//   k_psin           one thread per query row: hypot(sum cos(n theta), sum sin(n theta)) / count over the row's members.
// Every index read from memory is checked before it is used, every write is checked against its capacity.
#include <cmath>
#include "tip_csr.h"
#include "tip_grid.h"

namespace tip {

constexpr int O_CAP = 512;          // candidates held in LDS per wavefront (20 bytes each)
constexpr double O_INF = __builtin_huge_val();

// the interval of pair (i, j), a = p_j - p_i, cut by one point b = p_k - p_i.  k = i (b = 0) and k = j (b = a) give s = 0 and
// |b|^2 - a.b = 0 exactly and cut nothing, so the callers do not single them out.
__device__ __forceinline__ void cut(double ax, double ay, double bx, double by, bool &alive, double &lo, double &hi)
{
    const double s = __dsub_rn(__dmul_rn(ax, by), __dmul_rn(ay, bx));
    const double num = __dsub_rn(__dadd_rn(__dmul_rn(bx, bx), __dmul_rn(by, by)), __dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)));
    if (s == 0.0) {
        if (num < 0.0) alive = false;
    } else {
        const double t = __ddiv_rn(num, __dmul_rn(2.0, s));
        if (s > 0.0) hi = fmin(hi, t);
        else lo = fmax(lo, t);
    }
    if (!(lo < hi)) alive = false;
}

// squared distance from p_i to the farther end of a live pair's interval (the circle's centre is a / 2 + t perp(a))
__device__ __forceinline__ double reach2(double ax, double ay, double lo, double hi)
{
    if (!(lo > -O_INF) || !(hi < O_INF)) return O_INF;
    const double t2 = fmax(lo * lo, hi * hi);
    return (ax * ax + ay * ay) * (0.25 + t2);
}

struct OSweep {
    long total;      // edges found
    double reach;    // this lane's largest reach2
};

// One sweep over the candidates of rectangle rc.  in_lds: the rectangle's points are the n_near points staged in LDS; otherwise
// they stream from the sorted arrays and the staged points are only the first filter.  raw != NULL: the edges' point positions
// go to raw[raw_base ...] (bounded by raw_cap).
__device__ OSweep sweep(const double *__restrict__ kx, const double *__restrict__ ky, const int *__restrict__ ki, int n_near, bool in_lds,
                        const int32_t *__restrict__ start, const PointGrid &g, const CellRect &rc, int n_fin, const double *__restrict__ sx,
                        const double *__restrict__ sy, const int32_t *__restrict__ sidx, double xi, double yi, int i, int lane,
                        int32_t *__restrict__ raw, long raw_base, long raw_cap)
{
    OSweep out = {0, 0.0};
    const unsigned long long below = (1ULL << lane) - 1ULL;
    const int rows = in_lds ? 1 : rc.y1 - rc.y0 + 1;
    for (int rr = 0; rr < rows; ++rr) {
        int jb = 0, je = n_near;
        if (!in_lds) rect_row(start, g, rc, rc.y0 + rr, n_fin, jb, je);
        for (int j0 = jb; j0 < je; j0 += 64) {
            const int j = j0 + lane;
            bool alive = j < je;
            double ax = 0.0, ay = 0.0, lo = -O_INF, hi = O_INF;
            int idx = -1;
            if (alive) {
                if (in_lds) ax = kx[j], ay = ky[j], idx = ki[j];
                else ax = __dsub_rn(sx[j], xi), ay = __dsub_rn(sy[j], yi), idx = sidx[j];
                alive = idx != i;
            }
            for (int k = 0; k < n_near && __any(alive); ++k)
                if (alive) cut(ax, ay, kx[k], ky[k], alive, lo, hi);
            if (!in_lds)
                for (int r2 = rc.y0; r2 <= rc.y1 && __any(alive); ++r2) {
                    int kb, ke;
                    rect_row(start, g, rc, r2, n_fin, kb, ke);
                    for (int k = kb; k < ke && __any(alive); ++k)
                        if (alive) cut(ax, ay, __dsub_rn(sx[k], xi), __dsub_rn(sy[k], yi), alive, lo, hi);
                }
            const unsigned long long mask = __ballot(alive);
            if (alive) {
                out.reach = fmax(out.reach, reach2(ax, ay, lo, hi));
                if (raw) {
                    const long pos = raw_base + out.total + __popcll(mask & below);
                    if (pos >= 0 && pos < raw_cap) raw[pos] = idx;
                }
            }
            out.total += __popcll(mask);
        }
    }
    return out;
}

template <typename OffT>
__global__ __launch_bounds__(64) void k_delaunay(const PointGrid *__restrict__ gp, const int32_t *__restrict__ start, int cell_cap,
                                                 const double *__restrict__ sx, const double *__restrict__ sy,
                                                 const int32_t *__restrict__ sidx, int n, int64_t *__restrict__ sizes,
                                                 int32_t *__restrict__ deg32, const OffT *__restrict__ moff, int32_t *__restrict__ raw,
                                                 int32_t *__restrict__ row_len, long raw_cap)
{
    __shared__ double kx[O_CAP], ky[O_CAP];
    __shared__ int ki[O_CAP];
    const int lane = threadIdx.x;
    const PointGrid g = *gp;
    int n_fin = start[cell_cap];
    if (n_fin > n) n_fin = n;
    const int p = blockIdx.x;                       // the same for every lane: all control flow below is uniform
    if (p >= n_fin || g.gx < 1 || g.gy < 1 || (long)g.gx * g.gy > cell_cap) return;
    const int i = sidx[p];
    if ((unsigned)i >= (unsigned)n) return;
    const double xi = sx[p], yi = sy[p];
    const int cxi = cell_coord(xi, g.minx, g.h, g.gx), cyi = cell_coord(yi, g.miny, g.h, g.gy);
    const long base = raw ? (long)moff[i] : 0;
    int n_near = 0;
    long total = 0;
    for (long r = 2;; r *= 2) {
        CellRect rc;
        rc.x0 = (int)((long)cxi - r > 0 ? (long)cxi - r : 0), rc.x1 = (int)((long)cxi + r < g.gx - 1 ? (long)cxi + r : g.gx - 1);
        rc.y0 = (int)((long)cyi - r > 0 ? (long)cyi - r : 0), rc.y1 = (int)((long)cyi + r < g.gy - 1 ? (long)cyi + r : g.gy - 1);
        const bool whole = rc.x0 == 0 && rc.y0 == 0 && rc.x1 == g.gx - 1 && rc.y1 == g.gy - 1;
        long count = 0;
        for (int row = rc.y0; row <= rc.y1; ++row) {
            int b, e;
            rect_row(start, g, rc, row, n_fin, b, e);
            count += e - b;
        }
        const bool fits = count <= O_CAP;
        if (fits) {
            __syncthreads();                        // (one wavefront: orders the LDS traffic of the previous sweep and this fill)
            int at = 0;
            for (int row = rc.y0; row <= rc.y1; ++row) {
                int b, e;
                rect_row(start, g, rc, row, n_fin, b, e);
                for (int q = b + lane; q < e; q += 64) {
                    const int slot = at + (q - b);
                    if (slot < O_CAP) kx[slot] = __dsub_rn(sx[q], xi), ky[slot] = __dsub_rn(sy[q], yi), ki[slot] = sidx[q];
                }
                at += e - b;
            }
            n_near = (int)count;
            __syncthreads();
        }
        OSweep sw = sweep(kx, ky, ki, n_near, fits, start, g, rc, n_fin, sx, sy, sidx, xi, yi, i, lane, nullptr, 0, 0);
        double reach = wave_reduce(sw.reach, [](double a, double b) { return fmax(a, b); });
        if (sw.total == 0) reach = O_INF;
        const double span = (double)r * g.h;
        if (whole || 4.0 * reach * (1.0 + 1e-9) <= span * span) {
            if (raw) sw = sweep(kx, ky, ki, n_near, fits, start, g, rc, n_fin, sx, sy, sidx, xi, yi, i, lane, raw, base, raw_cap);
            total = sw.total;
            break;
        }
    }
    if (lane == 0) {
        if (sizes) sizes[i] = total;
        if (deg32) deg32[i] = (int32_t)total;
        if (row_len) row_len[i] = (int32_t)total;
    }
}

template <typename OffT>
__global__ void k_psin(const double *__restrict__ cy, const double *__restrict__ cx, int n, const int32_t *__restrict__ query, long m,
                       const OffT *__restrict__ moff, const int32_t *__restrict__ members, long n_members, int order,
                       double *__restrict__ out)
{
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    const long r = query ? (long)query[q] : q;
    if (r < 0 || r >= n) { out[q] = 0.0; return; }
    long b = (long)moff[q], e = (long)moff[q + 1];
    if (b < 0) b = 0;
    if (e > n_members) e = n_members;
    const double y0 = cy[r], x0 = cx[r], nn = (double)order;
    double sc = 0.0, ss = 0.0;
    long cnt = 0;
    for (long a = b; a < e; ++a) {
        const int k = members[a] - 1;
        if ((unsigned)k >= (unsigned)n) continue;
        const double th = __dmul_rn(nn, atan2(__dsub_rn(cy[k], y0), __dsub_rn(cx[k], x0)));
        double sn, cs;
        sincos(th, &sn, &cs);
        sc = __dadd_rn(sc, cs), ss = __dadd_rn(ss, sn);
        ++cnt;
    }
    out[q] = cnt ? __ddiv_rn(hypot(sc, ss), (double)cnt) : 0.0;
}

// ---- launches on device arrays --------------------------------------------------------------------------------------------------
// sizes / deg32 (either may be NULL): the degrees; members (with moff, of OffT): the rows, ascending, each entry + add
template <typename OffT>
static int delaunay_launch(const double *py, const double *px, int64_t n, int64_t *sizes, int32_t *deg32, const OffT *moff, int32_t *members,
                           int64_t members_cap, int add)
{
    Ctx &c = ctx();
    if (sizes && n) TIP_HIP(hipMemsetAsync(sizes, 0, (size_t)n * 8, c.stream));
    if (deg32 && n) TIP_HIP(hipMemsetAsync(deg32, 0, (size_t)n * 4, c.stream));
    if (n < 2) return TIP_OK;
    WsGuard ws;
    static const char *const names[3] = {"order_grid", "order_count", "order_fill"};
    PointGridArrays gr;
    if (int rc = point_grid_launch(ws, PointsYX{py, px}, n, SideTwoPerCell{}, names, gr)) return rc;
    int32_t *raw = members ? ws.get<int32_t>((size_t)members_cap) : nullptr, *row_len = members ? ws.get<int32_t>((size_t)n) : nullptr;
    if (members && (!raw || !row_len)) return TIP_ERR_NOMEM;
    if (row_len) TIP_HIP(hipMemsetAsync(row_len, 0, (size_t)n * 4, c.stream));
    TIP_LAUNCH("delaunay", k_delaunay<OffT>, dim3((unsigned)n), dim3(64), 0, (const PointGrid *)gr.g, (const int32_t *)gr.start, gr.cell_cap,
               (const double *)gr.payload, (const double *)gr.payload + plane_pitch(n), (const int32_t *)gr.sidx, (int)n, sizes, deg32, moff, raw, row_len,
               (long)members_cap);
    if (members)
        TIP_LAUNCH("order_row_sort", k_rank_sort<OffT>, dim3(cdiv(n, CSR_WPB)), dim3(CSR_BLOCK), 0, moff, (const int32_t *)row_len,
                   (const int32_t *)raw, (long)members_cap, members, (int)n, (long)members_cap, add);
    return TIP_OK;
}

template <typename OffT>
static int psin_launch(const double *cy, const double *cx, int64_t n, const int32_t *query, int64_t m, const OffT *moff, const int32_t *members,
                       int64_t n_members, int order, double *out)
{
    if (m == 0) return TIP_OK;
    TIP_LAUNCH("psin", k_psin<OffT>, dim3(cdiv(m, 256)), dim3(256), 0, cy, cx, (int)n, query, (long)m, moff, members, (long)n_members, order, out);
    return TIP_OK;
}

static int check_delaunay_args(const char *who, const double *py, const double *px, int64_t n, const int64_t *sizes, const int64_t *moff,
                               const int32_t *members, int64_t members_cap)
{
    if (n < 0 || n > 0x7ffffff0 - 8) return fail(TIP_ERR_ARG, "%s: n = %ld points", who, (long)n);
    if (n > 0 && (!py || !px)) return fail(TIP_ERR_ARG, "%s: the coordinates (py, px)", who);
    if (n > 0 && !sizes && !members) return fail(TIP_ERR_ARG, "%s: no output", who);
    if (members && (!moff || members_cap < 0 || members_cap > 0x7fffffff)) return fail(TIP_ERR_ARG, "%s: members need member_offsets and a capacity", who);
    return TIP_OK;
}

static int check_psin_args(const char *who, const double *cy, const double *cx, int64_t n, int64_t m, const int64_t *moff, const int32_t *members,
                           int64_t n_members, int order, const double *out)
{
    if (n < 0 || n > 0x7ffffffe || m < 0 || n_members < 0 || n_members > 0x7fffffff)
        return fail(TIP_ERR_ARG, "%s: n = %ld rows, m = %ld queries, %ld members", who, (long)n, (long)m, (long)n_members);
    if (order < 1 || order > 64) return fail(TIP_ERR_ARG, "%s: order %d (1..64)", who, order);
    if ((n > 0 && (!cy || !cx)) || !moff || (n_members > 0 && !members) || (m > 0 && !out)) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_delaunay_neighbors_f64_dev(const double *py, const double *px, int64_t n, int64_t *sizes, const int64_t *member_offsets,
                                   int32_t *members, int64_t members_cap)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_delaunay_args("tip_delaunay_neighbors_f64_dev", py, px, n, sizes, member_offsets, members, members_cap)) return rc;
    return delaunay_launch<int64_t>(py, px, n, sizes, nullptr, member_offsets, members, members_cap, 0);
}

int tip_delaunay_neighbors_f64(const double *py, const double *px, int64_t n, int64_t *sizes, const int64_t *member_offsets, int32_t *members,
                               int64_t members_cap)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_delaunay_args("tip_delaunay_neighbors_f64", py, px, n, sizes, member_offsets, members, members_cap)) return rc;
    for (int64_t p = 0; p < n; ++p) {
        if (!std::isfinite(py[p]) || !std::isfinite(px[p]))
            return fail(TIP_ERR_ARG, "tip_delaunay_neighbors_f64: point %ld has a non-finite coordinate", (long)p);
        if (members && (member_offsets[p] < 0 || member_offsets[p] > members_cap))
            return fail(TIP_ERR_ARG, "tip_delaunay_neighbors_f64: member_offsets[%ld] = %ld, capacity %ld", (long)p, (long)member_offsets[p],
                        (long)members_cap);
    }
    if (n == 0) return TIP_OK;
    Staging st;
    const double *dy = st.in(py, (size_t)n), *dx = st.in(px, (size_t)n);
    const int64_t *dmoff = members ? st.in(member_offsets, (size_t)n) : nullptr;
    int64_t *dsizes = st.out(sizes, (size_t)n);
    int32_t *dmem = st.out(members, (size_t)members_cap, true);
    if (st.rc) return st.rc;
    if (int rc = delaunay_launch<int64_t>(dy, dx, n, dsizes, nullptr, dmoff, dmem, members_cap, 0)) return rc;
    return st.finish();
}

int tip_psin_f64_dev(const double *cy, const double *cx, int64_t n, const int32_t *query, int64_t m, const int64_t *member_offsets,
                     const int32_t *members, int64_t n_members, int order, double *out)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_psin_args("tip_psin_f64_dev", cy, cx, n, m, member_offsets, members, n_members, order, out)) return rc;
    return psin_launch<int64_t>(cy, cx, n, query, m, member_offsets, members, n_members, order, out);
}

int tip_psin_f64(const double *cy, const double *cx, int64_t n, const int32_t *query, int64_t m, const int64_t *member_offsets,
                 const int32_t *members, int64_t n_members, int order, double *out)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_psin_args("tip_psin_f64", cy, cx, n, m, member_offsets, members, n_members, order, out)) return rc;
    if (!query && m > n) return fail(TIP_ERR_ARG, "tip_psin_f64: %ld queries of %ld rows", (long)m, (long)n);
    for (int64_t q = 0; q < m; ++q) {
        if (query && (query[q] < 0 || query[q] >= n)) return fail(TIP_ERR_ARG, "tip_psin_f64: query %ld is row %d of %ld", (long)q, query[q], (long)n);
        if (member_offsets[q] < 0 || member_offsets[q + 1] < member_offsets[q] || member_offsets[q + 1] > n_members)
            return fail(TIP_ERR_ARG, "tip_psin_f64: member_offsets[%ld .. %ld] = %ld, %ld with %ld members", (long)q, (long)q + 1,
                        (long)member_offsets[q], (long)member_offsets[q + 1], (long)n_members);
    }
    for (int64_t a = 0; a < n_members; ++a)
        if (members[a] < 1 || members[a] > n) return fail(TIP_ERR_ARG, "tip_psin_f64: member %ld is label %d (1..%ld)", (long)a, members[a], (long)n);
    if (m == 0) return TIP_OK;
    Staging st;
    const double *dy = st.in(cy, (size_t)n), *dx = st.in(cx, (size_t)n);
    const int32_t *dq = st.in(query, (size_t)m), *dmem = st.in(members, (size_t)n_members);
    const int64_t *dmoff = st.in(member_offsets, (size_t)m + 1);
    double *dout = st.out(out, (size_t)m);
    if (st.rc) return st.rc;
    if (int rc = psin_launch<int64_t>(dy, dx, n, dq, m, dmoff, dmem, n_members, order, dout)) return rc;
    return st.finish();
}

int tip_order_features_f64_dev(const double *py, const double *px, int64_t n, int order, double *psi, int64_t *degree)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (n < 0 || n > 0x7ffffff0 - 8 || order < 1 || order > 64) return fail(TIP_ERR_ARG, "tip_order_features_f64_dev: n = %ld points, order %d", (long)n, order);
    if (n > 0 && (!py || !px || !psi || !degree)) return fail(TIP_ERR_ARG, "tip_order_features_f64_dev: null pointer");
    if (n == 0) return TIP_OK;
    WsGuard ws;
    int32_t *deg32 = ws.get<int32_t>((size_t)n), *off32 = ws.get<int32_t>((size_t)n + 1);
    if (!deg32 || !off32) return TIP_ERR_NOMEM;
    if (int rc = delaunay_launch<int32_t>(py, px, n, degree, deg32, nullptr, nullptr, 0, 0)) return rc;
    if (int rc = scan_i32_dev(deg32, off32, (int)n)) return rc;
    int32_t total = 0;
    TIP_HIP(hipMemcpyAsync(&total, off32 + n, 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    if (total < 0) return fail(TIP_ERR_OVERFLOW, "tip_order_features_f64_dev: the neighbour lists overflow int32");
    int32_t *mem = ws.get<int32_t>((size_t)total);
    if (!mem) return TIP_ERR_NOMEM;
    if (total) TIP_HIP(hipMemsetAsync(mem, 0, (size_t)total * 4, c.stream));
    if (total)
        if (int rc = delaunay_launch<int32_t>(py, px, n, nullptr, nullptr, (const int32_t *)off32, mem, total, 1)) return rc;
    return psin_launch<int32_t>(py, px, n, nullptr, n, (const int32_t *)off32, (const int32_t *)mem, total, order, psi);
}

}  // extern "C"
