// tip_spatial.hip -- window statistics over a cell table and the spatial feature map built from them (ti.py:1200-1266,
// Tissue.calculate_spatial_data and the per-cell windows of get_frame_data): for M centres (grid points or cell centroids) and
// N table rows, which rows lie strictly inside the circle of squared radius r2 around each centre, and per centre their
// count, their exact area sum, the count of those that also pass a cell-type selector and the sum of one feature column over
// the selected ones.  The reference answers every centre with a pandas query over the whole table; here it is M x N distance
// tests in one launch.
//
//   k_window_stats   one thread per centre, SP_TILE centres per workgroup (two waves).  The table streams through LDS in chunks
//                    of SP_CHUNK rows: the workgroup loads a chunk together (coalesced; the selector is applied once per row
//                    there and kept as a byte), and after the barrier every lane walks the chunk -- all lanes read the SAME LDS
//                    address, a broadcast, no bank conflict.  16.5 KiB of LDS per workgroup, no atomics: a thread owns its
//                    centre's four accumulators in registers.
//                    The inclusion test rounds as numpy evaluates `(cx - x)**2 + (cy - y)**2 < r2`: two subtractions, two
//                    squarings, one addition, each rounded to float64 (__dsub_rn / __dmul_rn / __dadd_rn: never contracted
//                    into an FMA, whatever the build flags), then a strict <.  A NaN coordinate is outside every circle, and
//                    r2 = +inf takes every finite row.
//   k_window_value   the per-centre value from the four statistics: density, type fraction or mean.
//   k_spatial_fill   the (Y, X) map: pixel (py, px) belongs to grid point (py / s, px / s) when its offset inside that cell of
//                    the grid is below 2 (s / 2) -- upstream's block [y - s/2, y + s/2) around y = s/2 + k s -- and the grid
//                    point exists (s/2 + k s < extent); every other pixel is 0.  An odd s leaves one-pixel seams, s = 1 an empty
//                    map, and the frame clips the last block, as upstream.
#include "tip_typesel.h"   // sp_selected / parse_selector: the type selector, shared with tip_graph.hip

namespace tip {

constexpr int SP_TILE = 128, SP_CHUNK = 512;
constexpr int SP_DENSITY = 0, SP_TYPE_FRACTION = 1, SP_MEAN = 2;

__global__ __launch_bounds__(SP_TILE) void k_window_stats(const double *__restrict__ qy, const double *__restrict__ qx, long M,
                                                          int grid_x, int step, double r2, const double *__restrict__ cy,
                                                          const double *__restrict__ cx, const int64_t *__restrict__ area,
                                                          const uint8_t *__restrict__ type, const double *__restrict__ feat, long N,
                                                          int sel_kind, int sel_bit, int64_t *__restrict__ n_in,
                                                          int64_t *__restrict__ area_in, int64_t *__restrict__ n_sel,
                                                          double *__restrict__ sum_sel)
{
    __shared__ double2 s_pos[SP_CHUNK];      // (cy, cx)
    __shared__ int64_t s_area[SP_CHUNK];
    __shared__ double s_feat[SP_CHUNK];
    __shared__ uint8_t s_sel[SP_CHUNK];
    const long m = (long)blockIdx.x * SP_TILE + threadIdx.x;
    const bool live = m < M;                 // (a thread without a centre still loads chunks and meets the barriers)
    double y = 0.0, x = 0.0;
    if (live) {
        if (qy) {
            y = qy[m];
            x = qx[m];
        } else {                             // the map's grid: point (gy, gx) sits at step / 2 + g * step
            y = (double)(step / 2 + (m / grid_x) * step);
            x = (double)(step / 2 + (m % grid_x) * step);
        }
    }
    int64_t a_n = 0, a_area = 0, a_sel = 0;
    double a_sum = 0.0;
    for (long base = 0; base < N; base += SP_CHUNK) {
        const int cnt = (int)(N - base < SP_CHUNK ? N - base : SP_CHUNK);
        __syncthreads();                     // the previous chunk has been read by every lane
        for (int i = threadIdx.x; i < cnt; i += SP_TILE) {
            s_pos[i] = make_double2(cy[base + i], cx[base + i]);
            s_area[i] = area[base + i];
            s_feat[i] = feat ? feat[base + i] : 0.0;
            s_sel[i] = sp_selected(type[base + i], sel_kind, sel_bit) ? 1 : 0;
        }
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int i = 0; i < cnt; ++i) {
                const double2 p = s_pos[i];
                const double dx = __dsub_rn(p.y, x), dy = __dsub_rn(p.x, y);
                const bool in = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) < r2;
                const bool sel = in && s_sel[i];
                a_n += in ? 1 : 0;
                a_area += in ? s_area[i] : 0;
                a_sel += sel ? 1 : 0;
                a_sum = __dadd_rn(a_sum, sel ? s_feat[i] : 0.0);
            }
        }
    }
    if (live) {
        n_in[m] = a_n;
        area_in[m] = a_area;
        n_sel[m] = a_sel;
        sum_sel[m] = a_sum;
    }
}

__global__ void k_window_value(const int64_t *__restrict__ n_in, const int64_t *__restrict__ area_in, const int64_t *__restrict__ n_sel,
                               const double *__restrict__ sum_sel, long M, int mode, double *__restrict__ val)
{
    const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int64_t k = n_sel[m];
    double v;
    if (mode == SP_DENSITY)
        v = (k == 0 || area_in[m] <= 0) ? 0.0 : (double)k / (double)area_in[m];
    else if (mode == SP_TYPE_FRACTION)
        v = k == 0 ? 0.0 : (double)k / (double)n_in[m];
    else
        v = sum_sel[m] / (double)k;           // NaN where no cell is selected: the caller reads n_sel and reports it
    val[m] = v;
}

__global__ void k_spatial_fill(const double *__restrict__ val, int Y, int X, int step, int grid_y, int grid_x, double *__restrict__ map)
{
    const int px = blockIdx.x * blockDim.x + threadIdx.x, py = blockIdx.y;
    if (px >= X || py >= Y) return;
    const int gy = py / step, gx = px / step, span = 2 * (step / 2);
    double v = 0.0;
    if (gy < grid_y && gx < grid_x && py - gy * step < span && px - gx * step < span) v = val[(long)gy * grid_x + gx];
    map[(long)py * X + px] = v;
}

static inline int grid_points(int extent, int step) { return extent > step / 2 ? (extent - step / 2 + step - 1) / step : 0; }

static int check_table(const char *who, const double *cy, const double *cx, const int64_t *area, const uint8_t *type, int64_t n,
                       int sel_bit, int sel_positive, double r2, Selector &sel)
{
    if (n < 0 || (n > 0 && (!cy || !cx || !area || !type))) return fail(TIP_ERR_ARG, "%s: the table's columns (n = %ld)", who, (long)n);
    if (int rc = parse_selector(who, sel_bit, sel_positive, true, sel)) return rc;
    if (r2 != r2) return fail(TIP_ERR_ARG, "%s: r2 is NaN", who);
    return TIP_OK;
}

// the arguments of tip_window_stats_f64[_dev] / tip_spatial_map_f64[_dev], checked once for both forms under the entry's own name
static int check_stats_args(const char *who, const double *qy, const double *qx, int64_t m, double r2, const double *cy, const double *cx,
                            const int64_t *area, const uint8_t *type, int64_t n, int sel_bit, int sel_positive, const int64_t *n_in,
                            const int64_t *area_in, const int64_t *n_sel, const double *sum_sel, Selector &sel)
{
    if (int rc = check_table(who, cy, cx, area, type, n, sel_bit, sel_positive, r2, sel)) return rc;
    if (m < 0 || (m > 0 && (!qy || !qx || !n_in || !area_in || !n_sel || !sum_sel)))
        return fail(TIP_ERR_ARG, "%s: the centres or the outputs (m = %ld)", who, (long)m);
    return TIP_OK;
}

static int check_map_args(const char *who, int y, int x, int step, double r2, const double *cy, const double *cx, const int64_t *area,
                          const uint8_t *type, const double *feat, int64_t n, int sel_bit, int sel_positive, int mode, const double *map,
                          Selector &sel)
{
    if (int rc = check_table(who, cy, cx, area, type, n, sel_bit, sel_positive, r2, sel)) return rc;
    if (!map || y < 1 || x < 1 || step < 1) return fail(TIP_ERR_ARG, "%s: map %d x %d, step %d", who, y, x, step);
    if (mode < SP_DENSITY || mode > SP_MEAN) return fail(TIP_ERR_ARG, "%s: mode %d (0 density, 1 type fraction, 2 mean)", who, mode);
    if (mode == SP_MEAN && n > 0 && !feat) return fail(TIP_ERR_ARG, "%s: the mean needs a feature column", who);
    return TIP_OK;
}

// the statistics of M centres (qy / qx device arrays, or NULL: the (grid_y x grid_x) grid of `step`) over device columns
static int window_stats_launch(const double *qy, const double *qx, long M, int grid_x, int step, double r2, const double *cy,
                               const double *cx, const int64_t *area, const uint8_t *type, const double *feat, long N, Selector sel,
                               int64_t *n_in, int64_t *area_in, int64_t *n_sel, double *sum_sel)
{
    if (M <= 0) return TIP_OK;
    TIP_LAUNCH("window_stats", k_window_stats, dim3(cdiv(M, SP_TILE)), dim3(SP_TILE), 0, qy, qx, M, grid_x, step, r2, cy, cx, area,
               type, feat, N, sel.kind, sel.bit, n_in, area_in, n_sel, sum_sel);
    return TIP_OK;
}

// grid, statistics, values and fill on device columns (arguments checked by the entry point)
static int spatial_map_launch(int y, int x, int step, double r2, const double *cy, const double *cx, const int64_t *area, const uint8_t *type,
                              const double *feat, long n, Selector sel, int mode, double *map, int64_t *n_sel_grid)
{
    const int gy = grid_points(y, step), gx = grid_points(x, step);
    const long M = (long)gy * gx;
    WsGuard ws;
    int64_t *stats = ws.get<int64_t>((size_t)3 * M);
    double *sum = ws.get<double>((size_t)M), *val = ws.get<double>((size_t)M);
    if (!stats || !sum || !val) return TIP_ERR_NOMEM;
    int64_t *nsel = n_sel_grid ? n_sel_grid : stats + 2 * M;
    if (int rc = window_stats_launch(nullptr, nullptr, M, gx, step, r2, cy, cx, area, type, feat, n, sel, stats,
                                     stats + M, nsel, sum))
        return rc;
    if (M > 0)
        TIP_LAUNCH("window_value", k_window_value, dim3(cdiv(M, 256)), dim3(256), 0, (const int64_t *)stats, (const int64_t *)(stats + M),
                   (const int64_t *)nsel, (const double *)sum, M, mode, val);
    TIP_LAUNCH("spatial_fill", k_spatial_fill, dim3(cdiv(x, 256), y), dim3(256), 0, (const double *)val, y, x, step, gy, gx, map);
    return TIP_OK;
}

// the device copies of a host table's five columns (feat may be NULL)
struct DevTable {
    const double *cy, *cx, *feat;
    const int64_t *area;
    const uint8_t *type;
};

static DevTable upload_table(Staging &st, const double *cy, const double *cx, const int64_t *area, const uint8_t *type, const double *feat, size_t n)
{
    return {st.in(cy, n), st.in(cx, n), st.in(feat, n), st.in(area, n), st.in(type, n)};
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_window_stats_f64_dev(const double *qy, const double *qx, int64_t m, double r2, const double *cy, const double *cx,
                             const int64_t *area, const uint8_t *type, const double *feat, int64_t n, int sel_bit, int sel_positive,
                             int64_t *n_in, int64_t *area_in, int64_t *n_sel, double *sum_sel)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_stats_args("tip_window_stats_f64_dev", qy, qx, m, r2, cy, cx, area, type, n, sel_bit, sel_positive, n_in, area_in, n_sel, sum_sel,
                                  sel))
        return rc;
    return window_stats_launch(qy, qx, (long)m, 1, 1, r2, cy, cx, area, type, feat, (long)n, sel, n_in, area_in, n_sel, sum_sel);
}

int tip_window_stats_f64(const double *qy, const double *qx, int64_t m, double r2, const double *cy, const double *cx,
                         const int64_t *area, const uint8_t *type, const double *feat, int64_t n, int sel_bit, int sel_positive,
                         int64_t *n_in, int64_t *area_in, int64_t *n_sel, double *sum_sel)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_stats_args("tip_window_stats_f64", qy, qx, m, r2, cy, cx, area, type, n, sel_bit, sel_positive, n_in, area_in, n_sel, sum_sel,
                                  sel))
        return rc;
    if (m == 0) return TIP_OK;
    const size_t M = (size_t)m;
    Staging st;
    const double *dqy = st.in(qy, M), *dqx = st.in(qx, M);
    const DevTable t = upload_table(st, cy, cx, area, type, feat, (size_t)n);
    int64_t *dn_in = st.out(n_in, M), *darea_in = st.out(area_in, M), *dn_sel = st.out(n_sel, M);
    double *dsum = st.out(sum_sel, M);
    if (st.rc) return st.rc;
    if (int rc = window_stats_launch(dqy, dqx, (long)m, 1, 1, r2, t.cy, t.cx, t.area, t.type, t.feat, (long)n, sel, dn_in, darea_in, dn_sel, dsum))
        return rc;
    return st.finish();
}

int tip_spatial_map_f64_dev(int y, int x, int step, double r2, const double *cy, const double *cx, const int64_t *area,
                            const uint8_t *type, const double *feat, int64_t n, int sel_bit, int sel_positive, int mode, double *map,
                            int64_t *n_sel_grid)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_map_args("tip_spatial_map_f64_dev", y, x, step, r2, cy, cx, area, type, feat, n, sel_bit, sel_positive, mode, map, sel))
        return rc;
    return spatial_map_launch(y, x, step, r2, cy, cx, area, type, feat, (long)n, sel, mode, map, n_sel_grid);
}

int tip_spatial_map_f64(int y, int x, int step, double r2, const double *cy, const double *cx, const int64_t *area,
                        const uint8_t *type, const double *feat, int64_t n, int sel_bit, int sel_positive, int mode, double *map,
                        int64_t *n_sel_grid)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_map_args("tip_spatial_map_f64", y, x, step, r2, cy, cx, area, type, feat, n, sel_bit, sel_positive, mode, map, sel))
        return rc;
    Staging st;
    const DevTable t = upload_table(st, cy, cx, area, type, feat, (size_t)n);
    double *dmap = st.out(map, (size_t)y * x);
    int64_t *dnsel = st.out(n_sel_grid, (size_t)grid_points(y, step) * grid_points(x, step));
    if (st.rc) return st.rc;
    if (int rc = spatial_map_launch(y, x, step, r2, t.cy, t.cx, t.area, t.type, t.feat, (long)n, sel, mode, dmap, dnsel)) return rc;
    return st.finish();
}

}  // extern "C"
