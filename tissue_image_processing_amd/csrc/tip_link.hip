// tip_link.hip -- frame-to-frame track linking (linking.FrameLinker's link finding; Tissue.track_cells_iterator_with_trackpy,
// ti.py:1881-1938, and movie.process_movie's linker stitchers).  The model is linking.link_candidates + _solve_subnet; DESIGN.md
// 5.10 has the argument why the ids are the host's.
//
//   point_grid_launch (tip_grid.h; launched as "link_grid" / "link_cell_count" / "csr_scan" / "link_cell_fill")
//                    the uniform grid over the (cy, cx) bounding box of the finite features, cells of side h >= search_range (h
//                    doubles until the grid has at most n + 4 cells: coordinates may be far apart after cumulative drift); the
//                    features (cy, cx, a, position) copied cell by cell, so the cells x0 .. x1 of one grid row are one contiguous
//                    range (rect_row).
//   k_link_candidates<false / true> / (scan_i32_dev)
//                    one thread per track: the features of the cells within one cell of the track's (h >= search_range, so nothing
//                    in reach lies further; the cell range is taken with a 1e-6 cell margin against the rounding of the division),
//                    d = sqrt(dy dy + dx dx + da da) left to right in explicitly rounded operations, a link iff d <= search_range.
//                    First the count per track, then -- after the scan and ONE look at the total -- (track, feature, d) at the
//                    track's offset: the links of one track are one contiguous range.
//   per round:       k_link_round_init, k_link_unite (union-find of tip_uf.h over the live links; node = track, or n_tracks +
//                    feature), k_link_nodes (every node finds its root -- the smallest index, so the root of a component with a
//                    link is a track -- and takes a member slot there: the slot counters are the component's sizes),
//                    k_link_solve (one wavefront per root: a component that fits is solved, one that does not is counted),
//                    k_link_prune (the links of solved components die, and so do those longer than the next round's range).
//                    The host looks at (oversized components, live links) once per round and multiplies the range itself, in
//                    double, as linking.link_candidates does.
//   k_link_solve     the subnet's augmented cost matrix in LDS, exactly _solve_subnet's: rows = tracks + one row per feature,
//                    columns = features + one column per track, d d on links, range^2 on "track lost" / "feature is new", 0 in the
//                    dummy block, 1e18 elsewhere (60 x 60 doubles = 28.8 KB: five subnets per CU), members ranked into ascending
//                    order first (np.unique's, by row_rank of tip_csr.h; the order in which the atomics handed out the slots leaves no trace).  The
//                    assignment is scipy's linear_sum_assignment step for step -- shortest augmenting paths with potentials, one
//                    lane per column, the minimum by a wave reduction, scipy's arithmetic and scipy's choice among equal
//                    candidates -- so that a subnet with several optimal assignments (cells on a lattice: exact ties do occur)
//                    gets the one the host linker gets.
// Every index read from memory is checked before it is used, every write is checked against its capacity.
#include <cmath>
#include "tip_csr.h"
#include "tip_grid.h"
#include "tip_uf.h"

namespace tip {

constexpr int L_MAX = 30, L_N = 2 * L_MAX;          // linking.MAX_SUBNET and the side of the augmented matrix
constexpr double L_BIG = 1e18, L_INF = __builtin_huge_val();
enum { LS_OVER = 0, LS_LIVE = 1, LS_SUBNETS = 2, LS_LARGEST = 3, LS_WORDS = 4 };

__device__ __forceinline__ bool finite3(const double *__restrict__ p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the cells [lo, hi] of one axis that can hold a feature within one cell side of position c (in cells); false: none
__device__ __forceinline__ bool cell_reach(double c, int g, int &lo, int &hi)
{
    const double a = floor(c - 1.000001), b = floor(c + 1.000001);
    if (!(b >= 0.0) || !(a <= (double)(g - 1))) return false;
    lo = a > 0.0 ? (int)a : 0;
    hi = b < (double)(g - 1) ? (int)b : g - 1;
    return true;
}

// FILL false: deg[s] = the links of track s, *total += them.  FILL true: the links at lstart[s] ...
template <bool FILL>
__global__ void k_link_candidates(const double *__restrict__ trk, int nt, const PointGrid *__restrict__ gp, const int32_t *__restrict__ start,
                                  int cell_cap, const double *__restrict__ spt, const int32_t *__restrict__ sidx, int n, double range,
                                  int32_t *__restrict__ deg, unsigned long long *__restrict__ total, const int32_t *__restrict__ lstart,
                                  int32_t *__restrict__ les, int32_t *__restrict__ led, double *__restrict__ lev, long n_links)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nt) return;
    const PointGrid g = *gp;
    const double *t = trk + 3 * (long)s;
    int n_fin = start[cell_cap];
    if (n_fin > n) n_fin = n;
    const long base = FILL ? (long)lstart[s] : 0;
    int found = 0;
    CellRect rc;
    if (finite3(t) && g.gx >= 1 && g.gy >= 1 && (long)g.gx * g.gy <= cell_cap && cell_reach(cell_pos(t[0], g.miny, g.h), g.gy, rc.y0, rc.y1) &&
        cell_reach(cell_pos(t[1], g.minx, g.h), g.gx, rc.x0, rc.x1)) {
        for (int row = rc.y0; row <= rc.y1; ++row) {
            int b, e;
            rect_row(start, g, rc, row, n_fin, b, e);
            for (int j = b; j < e; ++j) {
                const double dy = __dsub_rn(t[0], spt[3 * (long)j]), dx = __dsub_rn(t[1], spt[3 * (long)j + 1]);
                const double da = __dsub_rn(t[2], spt[3 * (long)j + 2]);
                const double d = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dy, dy), __dmul_rn(dx, dx)), __dmul_rn(da, da)));
                if (!(d <= range)) continue;
                if (FILL) {
                    const long pos = base + found;
                    const int f = sidx[j];
                    if (pos >= 0 && pos < n_links && (unsigned)f < (unsigned)n) les[pos] = s, led[pos] = f, lev[pos] = d;
                }
                ++found;
            }
        }
    }
    if (!FILL) {
        deg[s] = found;
        if (found) atomicAdd(total, (unsigned long long)found);
    }
}

// ---- one round ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_link_round_init(int *__restrict__ parent, long nodes, int32_t *__restrict__ status)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nodes) parent[i] = (int)i;
    if (i == 0) status[LS_OVER] = 0, status[LS_LIVE] = 0;
}

__global__ __launch_bounds__(256) void k_link_unite(const int32_t *__restrict__ les, const int32_t *__restrict__ led,
                                                    const uint8_t *__restrict__ alive, long n_links, int nt, int n, int *__restrict__ parent)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_links || !alive[k]) return;
    const int s = les[k], f = led[k];
    if ((unsigned)s >= (unsigned)nt || (unsigned)f >= (unsigned)n) return;
    uf_unite(parent, s, nt + f);
}

// parent[i] = root; a node whose root is a track (every component with a link) takes slot cnt[root]++ of the root's member row
__global__ __launch_bounds__(256) void k_link_nodes(int *__restrict__ parent, int nt, int n, int32_t *__restrict__ cnt_t,
                                                    int32_t *__restrict__ cnt_f, int32_t *__restrict__ memb_t, int32_t *__restrict__ memb_f)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)nt + n) return;
    const int r = uf_find(parent, (int)i);
    parent[i] = r;
    if ((unsigned)r >= (unsigned)nt) return;
    if (i < nt) {
        const int k = atomicAdd(&cnt_t[r], 1);
        if (k < L_MAX) memb_t[(long)r * L_MAX + k] = (int)i;
    } else {
        const int k = atomicAdd(&cnt_f[r], 1);
        if (k < L_MAX) memb_f[(long)r * L_MAX + k] = (int)(i - nt);
    }
}

__global__ __launch_bounds__(64) void k_link_solve(const int *__restrict__ parent, const int32_t *__restrict__ cnt_t,
                                                   const int32_t *__restrict__ cnt_f, const int32_t *__restrict__ memb_t,
                                                   const int32_t *__restrict__ memb_f, int nt, int n, int max_subnet,
                                                   const int32_t *__restrict__ lstart, const int32_t *__restrict__ led,
                                                   const double *__restrict__ lev, const uint8_t *__restrict__ alive, long n_links,
                                                   double null_cost, int32_t *__restrict__ track_of_feature, int32_t *__restrict__ status)
{
    __shared__ double cost[L_N * L_N];
    __shared__ int st[L_MAX], sf[L_MAX], raw_t[L_MAX], raw_f[L_MAX];
    const int r = blockIdx.x, lane = threadIdx.x;   // r is the same for every lane: all control flow below is uniform
    if (r >= nt || parent[r] != r) return;
    const int ct = cnt_t[r], cf = cnt_f[r];
    if (ct <= 0 || cf <= 0) return;                 // a track without a live link
    if (ct > max_subnet || cf > max_subnet || ct > L_MAX || cf > L_MAX) {
        if (lane == 0) atomicAdd(&status[LS_OVER], 1);
        return;
    }
    int mt = lane < ct ? memb_t[(long)r * L_MAX + lane] : 0, mf = lane < cf ? memb_f[(long)r * L_MAX + lane] : 0;
    if (__any((unsigned)mt >= (unsigned)nt || (unsigned)mf >= (unsigned)n)) return;
    if (lane < ct) raw_t[lane] = mt;
    if (lane < cf) raw_f[lane] = mf;
    __syncthreads();
    if (lane < ct) st[row_rank(raw_t, 0, ct, mt, lane)] = mt;
    if (lane < cf) sf[row_rank(raw_f, 0, cf, mf, lane)] = mf;
    const int N = ct + cf;
    for (int e = lane; e < N * N; e += 64) {
        const int i = e / N, j = e - i * N;
        double c = L_BIG;
        if (i < ct ? j == cf + i : j == i - ct) c = null_cost;   // track i lost / feature j starts a new track
        if (i >= ct && j >= cf) c = 0.0;
        cost[i * L_N + j] = c;
    }
    __syncthreads();
    for (int i = 0; i < ct; ++i) {
        const int s = st[i];
        long b = lstart[s], e = lstart[s + 1];
        if (b < 0) b = 0;
        if (e > n_links) e = n_links;
        for (long k = b + lane; k < e; k += 64) {
            if (!alive[k]) continue;
            const int f = led[k];
            const double d = lev[k];
            for (int j = 0; j < cf; ++j)
                if (sf[j] == f) cost[i * L_N + j] = __dmul_rn(d, d);
        }
    }
    __syncthreads();
    // scipy's linear_sum_assignment on the N x N matrix, step for step (rectangular_lsap: for every row a shortest augmenting
    // path over the columns not yet scanned, then the dual update, then the augmentation).  Lane l is column l in the search
    // and row l in the dual update.  scipy keeps the unscanned columns in a list, filled N - 1 .. 0, from which a scanned column
    // is removed by moving the last one into its place; among columns of equal lowest cost it takes the first of the list, or
    // the last unmatched one if there is any.  pos is a column's place in that list, so the choice -- and with it the result on
    // tied optima -- is scipy's.  The arithmetic is scipy's too: (min + c - u) - v, u += min - spc, v -= min - spc.
    const bool active = lane < N;
    double ul = 0.0, vl = 0.0;
    int col4row = -1, row4col = -1, path = -1;
    for (int cur = 0; cur < N; ++cur) {
        int pos = N - 1 - lane, n_rem = N, i = cur, sink = -1;
        bool scanned = false, reached = false;      // this lane's column is scanned (SC) / this lane's row is reached (SR)
        double spc = L_INF, min_val = 0.0;          // shortest path cost to this lane's column
        for (int it = 0; it < N && sink < 0; ++it) {
            if (lane == i) reached = true;
            const double ui = __shfl(ul, i);
            const bool rem = active && !scanned;
            if (rem) {
                const double c = __dsub_rn(__dsub_rn(__dadd_rn(min_val, cost[i * L_N + lane]), ui), vl);
                if (c < spc) path = i, spc = c;
            }
            const double lowest = wave_reduce(rem ? spc : L_INF, [](double a, double b) { return fmin(a, b); });
            if (!(lowest < L_INF)) return;          // (an infeasible matrix: every row here has a finite entry)
            const bool tie = rem && spc == lowest;
            const bool any_free = __any(tie && row4col < 0);
            const int key = wave_max(tie && (!any_free || row4col < 0) ? (any_free ? pos : -pos) : -0x7fffffff);
            const int index = any_free ? key : -key;
            const unsigned long long pick = __ballot(rem && pos == index);
            if (!pick) return;
            const int jsel = __ffsll((long long)pick) - 1;
            min_val = lowest;
            const int owner = __shfl(row4col, jsel);
            if (owner < 0) sink = jsel;
            else i = owner;
            if (lane == jsel) scanned = true;
            --n_rem;
            if (active && !scanned && pos == n_rem) pos = index;
        }
        if (sink < 0) return;
        int src = reached && lane != cur ? col4row : 0;
        if ((unsigned)src >= 64u) src = 0;
        const double through = __shfl(spc, src);    // spc of the column this lane's row is matched to
        if (lane == cur) ul = __dadd_rn(ul, min_val);
        else if (reached) ul = __dadd_rn(ul, __dsub_rn(min_val, through));
        if (scanned) vl = __dsub_rn(vl, __dsub_rn(min_val, spc));
        int j = sink;
        for (int it = 0; it <= N; ++it) {
            const int i2 = __shfl(path, j);
            if ((unsigned)i2 >= (unsigned)N) return;
            if (lane == j) row4col = i2;
            const int before = __shfl(col4row, i2);
            if (lane == i2) col4row = j;
            j = before;
            if (i2 == cur) break;
            if ((unsigned)j >= (unsigned)N) return;
        }
    }
    if (lane < ct && col4row >= 0 && col4row < cf && cost[lane * L_N + col4row] < L_BIG) track_of_feature[sf[col4row]] = st[lane];
    if (lane == 0) {
        atomicAdd(&status[LS_SUBNETS], 1);
        atomicMax(&status[LS_LARGEST], ct > cf ? ct : cf);
    }
}

// the links of the components that were solved die; the others stay when d <= next_range
__global__ __launch_bounds__(256) void k_link_prune(const int32_t *__restrict__ les, const double *__restrict__ lev, uint8_t *__restrict__ alive,
                                                    long n_links, const int *__restrict__ parent, const int32_t *__restrict__ cnt_t,
                                                    const int32_t *__restrict__ cnt_f, int nt, int max_subnet, double next_range,
                                                    int32_t *__restrict__ status)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = false;
    if (k < n_links && alive[k]) {
        const int s = les[k];
        const int r = (unsigned)s < (unsigned)nt ? parent[s] : -1;
        if ((unsigned)r < (unsigned)nt) live = (cnt_t[r] > max_subnet || cnt_f[r] > max_subnet) && lev[k] <= next_range;
        if (!live) alive[k] = 0;
    }
    const unsigned long long mask = __ballot(live);
    if (mask && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)mask) - 1)) atomicAdd(&status[LS_LIVE], __popcll(mask));
}

static int64_t bits_of(double v)
{
    int64_t b;
    memcpy(&b, &v, 8);
    return b;
}

// the whole call on device arrays; stats_host: 6 entries.  Waits for the stream (once for the link total, once per round).
static int link_frame_launch(const double *trk, int64_t nt, const double *pts, int64_t n, double search_range, double adaptive_stop,
                             double adaptive_step, int max_subnet, int32_t *track_of_feature, int64_t *stats_host)
{
    Ctx &c = ctx();
    for (int k = 0; k < 6; ++k) stats_host[k] = 0;
    stats_host[4] = bits_of(search_range);
    if (n) TIP_HIP(hipMemsetAsync(track_of_feature, 0xff, (size_t)n * 4, c.stream));
    if (n == 0 || nt == 0) return TIP_OK;
    WsGuard ws;
    static const char *const names[3] = {"link_grid", "link_cell_count", "link_cell_fill"};
    PointGridArrays gr;
    if (int rc = point_grid_launch(ws, PointsRows3{pts}, n, SideGiven{search_range}, names, gr)) return rc;
    const int cell_cap = gr.cell_cap;
    const PointGrid *g = gr.g;
    const int32_t *start = gr.start, *sidx = gr.sidx;
    const double *spt = gr.payload;
    int32_t *deg = ws.get<int32_t>((size_t)nt), *lstart = ws.get<int32_t>((size_t)nt + 1);
    unsigned long long *total = ws.get<unsigned long long>(1);
    if (!deg || !lstart || !total) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemsetAsync(total, 0, 8, c.stream));
    TIP_LAUNCH("link_count", k_link_candidates<false>, dim3(cdiv(nt, 64)), dim3(64), 0, trk, (int)nt, g, start, cell_cap, spt, sidx, (int)n,
               search_range, deg, total, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (double *)nullptr, 0L);
    if (int rc = scan_i32_dev(deg, lstart, (int)nt)) return rc;
    unsigned long long n_links_host = 0;
    TIP_HIP(hipMemcpyAsync(&n_links_host, total, 8, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    if (n_links_host > 0x7fffffffULL) return fail(TIP_ERR_OVERFLOW, "tip_link_frame_f64: %llu candidate links overflow int32", n_links_host);
    const long n_links = (long)n_links_host;
    stats_host[0] = n_links;
    if (n_links == 0) return TIP_OK;

    const long nodes = (long)nt + n;
    int32_t *les = ws.get<int32_t>((size_t)n_links), *led = ws.get<int32_t>((size_t)n_links);
    double *lev = ws.get<double>((size_t)n_links);
    uint8_t *alive = ws.get<uint8_t>((size_t)n_links);
    int *parent = ws.get<int>((size_t)nodes);
    int32_t *cnts = ws.get<int32_t>((size_t)nt * 2), *memb = ws.get<int32_t>((size_t)nt * 2 * L_MAX), *status = ws.get<int32_t>(LS_WORDS);
    if (!les || !led || !lev || !alive || !parent || !cnts || !memb || !status) return TIP_ERR_NOMEM;
    int32_t *cnt_t = cnts, *cnt_f = cnts + nt, *memb_t = memb, *memb_f = memb + (size_t)nt * L_MAX;
    TIP_HIP(hipMemsetAsync(les, 0xff, (size_t)n_links * 4, c.stream));      // (a slot the fill does not reach names no track)
    TIP_HIP(hipMemsetAsync(led, 0xff, (size_t)n_links * 4, c.stream));
    TIP_HIP(hipMemsetAsync(lev, 0, (size_t)n_links * 8, c.stream));
    TIP_HIP(hipMemsetAsync(alive, 1, (size_t)n_links, c.stream));
    TIP_HIP(hipMemsetAsync(status, 0, LS_WORDS * 4, c.stream));
    TIP_LAUNCH("link_fill", k_link_candidates<true>, dim3(cdiv(nt, 64)), dim3(64), 0, trk, (int)nt, g, start, cell_cap, spt, sidx, (int)n,
               search_range, (int32_t *)nullptr, (unsigned long long *)nullptr, (const int32_t *)lstart, les, led, lev, n_links);
    double rng = search_range;
    volatile double two = 2.0;      // the null cost is Python's `rng ** 2`: libm's pow at run time, which is not always rng * rng
    for (;;) {
        const double next = rng * adaptive_step, null_cost = std::pow(rng, two);
        ++stats_host[1];
        TIP_HIP(hipMemsetAsync(cnts, 0, (size_t)nt * 2 * 4, c.stream));
        TIP_LAUNCH("link_round_init", k_link_round_init, dim3(cdiv(nodes, 256)), dim3(256), 0, parent, nodes, status);
        TIP_LAUNCH("link_unite", k_link_unite, dim3(cdiv(n_links, 256)), dim3(256), 0, (const int32_t *)les, (const int32_t *)led,
                   (const uint8_t *)alive, n_links, (int)nt, (int)n, parent);
        TIP_LAUNCH("link_nodes", k_link_nodes, dim3(cdiv(nodes, 256)), dim3(256), 0, parent, (int)nt, (int)n, cnt_t, cnt_f, memb_t, memb_f);
        TIP_LAUNCH("link_solve", k_link_solve, dim3((unsigned)nt), dim3(64), 0, (const int *)parent, (const int32_t *)cnt_t, (const int32_t *)cnt_f,
                   (const int32_t *)memb_t, (const int32_t *)memb_f, (int)nt, (int)n, max_subnet, (const int32_t *)lstart, (const int32_t *)led,
                   (const double *)lev, (const uint8_t *)alive, n_links, null_cost, track_of_feature, status);
        TIP_LAUNCH("link_prune", k_link_prune, dim3(cdiv(n_links, 256)), dim3(256), 0, (const int32_t *)les, (const double *)lev, alive, n_links,
                   (const int *)parent, (const int32_t *)cnt_t, (const int32_t *)cnt_f, (int)nt, max_subnet, next, status);
        int32_t hs[LS_WORDS] = {0, 0, 0, 0};
        TIP_HIP(hipMemcpyAsync(hs, status, LS_WORDS * 4, hipMemcpyDeviceToHost, c.stream));
        TIP_HIP(hipStreamSynchronize(c.stream));
        stats_host[2] = hs[LS_SUBNETS], stats_host[3] = hs[LS_LARGEST], stats_host[4] = bits_of(rng);
        if (hs[LS_OVER] == 0) break;
        if (adaptive_stop < 0.0) { stats_host[5] = 1; break; }
        rng = next;
        stats_host[4] = bits_of(rng);
        if (rng < adaptive_stop || rng == 0.0) { stats_host[5] = 2; break; }      // (rng == 0: coincident points can never split)
        if (hs[LS_LIVE] == 0) break;
    }
    return TIP_OK;
}

static int check_link_args(const char *who, const double *trk, int64_t nt, const double *pts, int64_t n, double search_range,
                           double adaptive_stop, double adaptive_step, int max_subnet, const int32_t *track_of_feature)
{
    if (n < 0 || nt < 0 || n > 0x7ffffff0 - 8 || nt > 0x7ffffff0 - 8 || n + nt > 0x7ffffff0 - 8)
        return fail(TIP_ERR_ARG, "%s: %ld tracks, %ld features", who, (long)nt, (long)n);
    if ((nt > 0 && !trk) || (n > 0 && (!pts || !track_of_feature))) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (!(search_range > 0.0) || !std::isfinite(search_range)) return fail(TIP_ERR_ARG, "%s: search_range %g", who, search_range);
    if (!(adaptive_step > 0.0 && adaptive_step < 1.0)) return fail(TIP_ERR_ARG, "%s: adaptive_step %g outside (0, 1)", who, adaptive_step);
    if (std::isnan(adaptive_stop)) return fail(TIP_ERR_ARG, "%s: adaptive_stop is not a number", who);
    if (max_subnet < 1 || max_subnet > L_MAX) return fail(TIP_ERR_UNSUPPORTED, "%s: max_subnet %d (1..%d)", who, max_subnet, L_MAX);
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_link_frame_f64_dev(const double *track_pos, int64_t n_tracks, const double *points, int64_t n, double search_range,
                           double adaptive_stop, double adaptive_step, int max_subnet, int32_t *track_of_feature, int64_t *stats)
{
    if (int rc = check_link_args("tip_link_frame_f64_dev", track_pos, n_tracks, points, n, search_range, adaptive_stop, adaptive_step,
                                 max_subnet, track_of_feature))
        return rc;
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    int64_t hs[6];
    if (int rc = link_frame_launch(track_pos, n_tracks, points, n, search_range, adaptive_stop, adaptive_step, max_subnet, track_of_feature, hs))
        return rc;
    if (stats) {
        TIP_HIP(hipMemcpyAsync(stats, hs, sizeof hs, hipMemcpyHostToDevice, c.stream));
        TIP_HIP(hipStreamSynchronize(c.stream));
    }
    return TIP_OK;
}

int tip_link_frame_f64(const double *track_pos, int64_t n_tracks, const double *points, int64_t n, double search_range,
                       double adaptive_stop, double adaptive_step, int max_subnet, int32_t *track_of_feature, int64_t *stats)
{
    const char *who = "tip_link_frame_f64";
    if (int rc = check_link_args(who, track_pos, n_tracks, points, n, search_range, adaptive_stop, adaptive_step, max_subnet, track_of_feature))
        return rc;
    for (int64_t k = 0; k < 3 * n_tracks; ++k)
        if (!std::isfinite(track_pos[k])) return fail(TIP_ERR_ARG, "%s: track %ld has a non-finite coordinate", who, (long)(k / 3));
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(points[k])) return fail(TIP_ERR_ARG, "%s: feature %ld has a non-finite coordinate", who, (long)(k / 3));
    int64_t hs[6] = {0, 0, 0, 0, bits_of(search_range), 0};
    if (n > 0 && n_tracks == 0) {
        for (int64_t k = 0; k < n; ++k) track_of_feature[k] = -1;
    } else if (n > 0) {
        Ctx &c = ctx();
        if (!c.stream) return TIP_ERR_HIP;
        Staging st;
        const double *dt = st.in(track_pos, (size_t)n_tracks * 3), *dp = st.in(points, (size_t)n * 3);
        int32_t *dout = st.out(track_of_feature, (size_t)n);
        if (st.rc) return st.rc;
        if (int rc = link_frame_launch(dt, n_tracks, dp, n, search_range, adaptive_stop, adaptive_step, max_subnet, dout, hs)) return rc;
        if (int rc = st.finish()) return rc;
    }
    if (stats) memcpy(stats, hs, sizeof hs);
    return TIP_OK;
}

}  // extern "C"
