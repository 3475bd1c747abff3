// tip_grid.h -- the uniform point grid shared by the Delaunay rows (tip_order.hip) and the track linker (tip_link.hip): the
// finite points of a table sorted into the square cells of side h of a grid over their bounding box, so that the points of the
// cells x0 .. x1 of one grid row are one contiguous range of the sorted arrays.
//
//   k_grid_shape     one workgroup: the (y, x) bounding box of the finite points by a 256-thread LDS reduction, then the cell side.
//                    The first h is the caller's (H0: about two points per cell for the Delaunay sweep, the search range for
//                    the linker); h doubles until the grid has at most cell_cap = n + 4 cells -- a thin box, or coordinates far
//                    apart after cumulative drift, would otherwise give more cells than points.  At most 2200 doublings (beyond
//                    them a double has overflowed): then one cell of side inf.  No finite point: a 1 x 1 grid at the origin.
//   k_grid_count     one thread per point: its cell (or -1: a non-finite point takes no part) and the cell's count, atomicAdd.
//   (scan_i32_dev)   the exclusive scan of the counts: start[c], and start[cell_cap] = the number of finite points.
//   k_grid_fill      one thread per point: a slot of its cell handed out with atomicAdd, the source's payload and the point's
//                    position copied there.  The order inside a cell is the atomics'; the consumers do not depend on it.
//   point_grid_launch  the sequence on the context stream, under the launch names of its caller.
//
// A point source answers: finite(p), y(p), x(p), payload_doubles(n) (the size of its payload) and copy(p, pos, n, out).  The cell of a
// coordinate is floor((v - lo) / h) in explicitly rounded operations, clamped to the grid: the consumers recompute it from the
// sorted copy and must get the same cell.  Every cell index is checked against cell_cap and every slot against n.
#pragma once
#include <cmath>
#include "tip_internal.h"

namespace tip {

constexpr double GRID_INF = __builtin_huge_val();

struct PointGrid {
    double miny, minx, h;
    int gy, gx;
};

// the pitch of one plane of a planar payload of n points: whole 256-byte lines, so that every plane starts on one (measured: the
// Delaunay sweep is 1 % slower when the sorted y start at the odd offset 8 n)
__host__ __device__ __forceinline__ long plane_pitch(long n) { return (n + 31) & ~31L; }

// (py[p], px[p]); the payload is two planes, the sorted x at out[0] and the sorted y at out[plane_pitch(n)]
struct PointsYX {
    static size_t payload_doubles(int64_t n) { return 2 * (size_t)plane_pitch(n); }
    const double *__restrict__ py, *__restrict__ px;
    __device__ __forceinline__ bool finite(int p) const
    {
        const double x = px[p], y = py[p];          // (both loads in flight before either test)
        return isfinite(x) && isfinite(y);
    }
    __device__ __forceinline__ double y(int p) const { return py[p]; }
    __device__ __forceinline__ double x(int p) const { return px[p]; }
    __device__ __forceinline__ void copy(int p, long pos, int n, double *__restrict__ out) const
    {
        const double x = px[p], y = py[p];
        out[pos] = x, out[plane_pitch(n) + pos] = y;
    }
};

// rows (y, x, a) of pts, finite on all three; the payload is the row
struct PointsRows3 {
    static size_t payload_doubles(int64_t n) { return 3 * (size_t)n; }
    const double *__restrict__ pts;
    __device__ __forceinline__ bool finite(int p) const
    {
        const double *q = pts + 3 * (long)p;
        return isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
    }
    __device__ __forceinline__ double y(int p) const { return pts[3 * (long)p]; }
    __device__ __forceinline__ double x(int p) const { return pts[3 * (long)p + 1]; }
    __device__ __forceinline__ void copy(int p, long pos, int, double *__restrict__ out) const
    {
        const double *q = pts + 3 * (long)p;
        const double y = q[0], x = q[1], a = q[2];  // (the loads first: the compiler cannot tell that out is another array)
        out[3 * pos] = y, out[3 * pos + 1] = x, out[3 * pos + 2] = a;
    }
};

// the first cell side: the caller's value, or about two points per square cell of the W x H box
struct SideGiven {
    double h;
    __device__ __forceinline__ double operator()(double, double, int) const { return h; }
};
struct SideTwoPerCell {
    __device__ __forceinline__ double operator()(double W, double H, int n) const
    {
        const double target = n / 2 > 1 ? (double)(n / 2) : 1.0;
        const double h = W > 0.0 && H > 0.0 ? sqrt(W / target * H) : (W > 0.0 || H > 0.0 ? fmax(W, H) / target : 1.0);
        return !(h > 0.0) || !isfinite(h) ? 1.0 : h;
    }
};

// position along one axis in cells, unclamped, and the cell it falls into
__device__ __forceinline__ double cell_pos(double v, double lo, double h) { return __ddiv_rn(__dsub_rn(v, lo), h); }

__device__ __forceinline__ int cell_coord(double v, double lo, double h, int g)
{
    const double c = floor(cell_pos(v, lo, h));
    if (!(c >= 0.0)) return 0;
    return c > (double)(g - 1) ? g - 1 : (int)c;
}

struct CellRect { int x0, x1, y0, y1; };

// the sorted points of the cells x0 .. x1 of grid row `row`: [b, e), clamped to the n_fin points that were sorted
__device__ __forceinline__ void rect_row(const int32_t *__restrict__ start, const PointGrid &g, const CellRect &rc, int row, int n_fin, int &b,
                                         int &e)
{
    b = start[row * g.gx + rc.x0];
    e = start[row * g.gx + rc.x1 + 1];
    if (b < 0) b = 0;
    if (e > n_fin) e = n_fin;
    if (e < b) e = b;
}

template <typename Src, typename H0>
__global__ __launch_bounds__(256) void k_grid_shape(Src src, int n, H0 h0, int cell_cap, PointGrid *__restrict__ g)
{
    __shared__ double s[4][256];
    double y0 = GRID_INF, y1 = -GRID_INF, x0 = GRID_INF, x1 = -GRID_INF;
    for (int p = threadIdx.x; p < n; p += 256) {
        if (!src.finite(p)) continue;
        const double y = src.y(p), x = src.x(p);
        y0 = fmin(y0, y), y1 = fmax(y1, y), x0 = fmin(x0, x), x1 = fmax(x1, x);
    }
    s[0][threadIdx.x] = y0, s[1][threadIdx.x] = y1, s[2][threadIdx.x] = x0, s[3][threadIdx.x] = x1;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s[0][threadIdx.x] = fmin(s[0][threadIdx.x], s[0][threadIdx.x + off]);
            s[1][threadIdx.x] = fmax(s[1][threadIdx.x], s[1][threadIdx.x + off]);
            s[2][threadIdx.x] = fmin(s[2][threadIdx.x], s[2][threadIdx.x + off]);
            s[3][threadIdx.x] = fmax(s[3][threadIdx.x], s[3][threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    y0 = s[0][0], y1 = s[1][0], x0 = s[2][0], x1 = s[3][0];
    if (!(y0 <= y1)) y0 = y1 = x0 = x1 = 0.0;      // no finite point
    const double H = y1 - y0, W = x1 - x0;
    double h = h0(W, H, n), fy = 1.0, fx = 1.0;
    bool ok = false;
    for (int it = 0; it < 2200 && !ok; ++it) {     // (cells of side h would outnumber the points: h doubles)
        fy = floor(H / h) + 1.0, fx = floor(W / h) + 1.0;
        ok = fy * fx <= (double)cell_cap;
        if (!ok) h *= 2.0;
    }
    if (!ok) fy = fx = 1.0, h = GRID_INF;
    g->miny = y0, g->minx = x0, g->h = h, g->gy = (int)fy, g->gx = (int)fx;
}

template <typename Src>
__global__ void k_grid_count(Src src, int n, const PointGrid *__restrict__ gp, int cell_cap, int32_t *__restrict__ cell_of,
                             int32_t *__restrict__ cnt)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const PointGrid g = *gp;
    int c = -1;
    if (src.finite(p)) c = cell_coord(src.y(p), g.miny, g.h, g.gy) * g.gx + cell_coord(src.x(p), g.minx, g.h, g.gx);
    if (c >= cell_cap) c = -1;
    cell_of[p] = c;
    if (c >= 0) atomicAdd(&cnt[c], 1);
}

template <typename Src>
__global__ void k_grid_fill(Src src, int n, const int32_t *__restrict__ cell_of, const int32_t *__restrict__ start,
                            int32_t *__restrict__ cursor, double *__restrict__ payload, int32_t *__restrict__ sidx)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int c = cell_of[p];
    if (c < 0) return;
    const long pos = (long)start[c] + atomicAdd(&cursor[c], 1);
    if (pos < 0 || pos >= n) return;
    src.copy(p, pos, n, payload);
    sidx[pos] = p;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// what the sequence leaves on the device (workspaces of the caller's guard): the grid, start[cell_cap + 1], and the sorted points'
// positions sidx[n] and payload[Src::payload_doubles(n)]
struct PointGridArrays {
    int cell_cap;
    PointGrid *g;
    int32_t *start, *sidx;
    double *payload;
};

// names: the launch names of the caller's grid, count and fill kernels
template <typename Src, typename H0>
int point_grid_launch(WsGuard &ws, Src src, int64_t n, H0 h0, const char *const names[3], PointGridArrays &a)
{
    Ctx &c = ctx();
    a.cell_cap = (int)(n < 0x7ffffff0 - 4 ? n + 4 : 0x7ffffff0);
    a.g = ws.get<PointGrid>(1);
    int32_t *cell_of = ws.get<int32_t>((size_t)n), *cnt = ws.get<int32_t>((size_t)a.cell_cap);
    a.start = ws.get<int32_t>((size_t)a.cell_cap + 1), a.sidx = ws.get<int32_t>((size_t)n);
    a.payload = ws.get<double>(Src::payload_doubles(n));
    if (!a.g || !cell_of || !cnt || !a.start || !a.sidx || !a.payload) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemsetAsync(cnt, 0, (size_t)a.cell_cap * 4, c.stream));
    TIP_LAUNCH(names[0], (k_grid_shape<Src, H0>), dim3(1), dim3(256), 0, src, (int)n, h0, a.cell_cap, a.g);
    TIP_LAUNCH(names[1], k_grid_count<Src>, dim3(cdiv(n, 256)), dim3(256), 0, src, (int)n, (const PointGrid *)a.g, a.cell_cap, cell_of, cnt);
    if (int rc = scan_i32_dev(cnt, a.start, a.cell_cap)) return rc;
    TIP_HIP(hipMemsetAsync(cnt, 0, (size_t)a.cell_cap * 4, c.stream));
    TIP_LAUNCH(names[2], k_grid_fill<Src>, dim3(cdiv(n, 256)), dim3(256), 0, src, (int)n, (const int32_t *)cell_of, (const int32_t *)a.start, cnt,
               a.payload, a.sidx);
    return TIP_OK;
}

}  // namespace tip
