// tip_events.hip -- the device side of the movie driver's event detection (ti.py:609-789, Tissue.find_events_iterator): the border
// cells of a label map, the exact label under a point, and the per-row classification of one frame pair.  The reference walks the
// candidate ids with one pandas query each; here the two frames' tables are row arrays (track id, selected = valid and not empty,
// positive for the type, a CSR of the neighbour sets) and one launch answers every row.  DESIGN.md 5.11 states the rules.
//
//   k_border_rows    one thread per border pixel (2 (y + x) of them: first and last row, first and last column): flags[l - 1] = 1.
//                    Several pixels of one cell store the same byte; the interior of the map is never read.
//   k_lookup_exact   one thread per query point: labels[qy, qx], -1 outside the frame (tip_lookup_max3_i32_dev without the 3x3
//                    maximum: the events code reads the raw previous map).
//   k_ev_init / k_ev_insert / k_ev_classify
//                    ids are matched across the two frames through one open-addressing hash table over the ids of both frames
//                    and of the first frame's border rows: capacity a power of two of at least twice the entries, 64-bit keys
//                    claimed with atomicCAS, linear probing bounded by the capacity.  A slot carries the id's set bits -- in P (a
//                    selected previous row), in C (a selected current row), in F (first frame's border ids), in E (the current
//                    frame's border ids, selected or not, as upstream's table.label[edge rows]), positive in the previous /
//                    current frame -- and the lowest selected previous row that holds it.  k_ev_classify then runs one thread per
//                    row of either frame: the row's own slot, a loop over its CSR row, one probe per neighbour.  No pass is
//                    quadratic in the rows, and a row with hundreds of neighbours is only a longer loop.
// A neighbour label n is a ROW INDEX (no minus one, upstream's quirk): the row test is 0 <= n < rows and sel[n].  Every read of adj is
// clamped to n_adj (row_of), so a malformed device CSR gives wrong flags, never an access outside the caller's arrays.  The id
// INT64_MIN marks an empty slot: a row that carries it is in no set (the host form rejects it).
#include "tip_csr.h"

namespace tip {

constexpr unsigned long long EV_EMPTY = 0x8000000000000000ULL;
constexpr int EV_P = 1, EV_C = 2, EV_F = 4, EV_E = 8, EV_PPOS = 16, EV_CPOS = 32;
constexpr int EV_BLOCK = 256, EV_MAX_BLOCKS = 1024;

__global__ void k_border_rows(const int32_t *__restrict__ labels, int Y, int X, long n, uint8_t *__restrict__ flags)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2L * X + 2L * Y) return;
    long py, px;
    if (i < X) { py = 0; px = i; }
    else if (i < 2L * X) { py = Y - 1; px = i - X; }
    else if (i < 2L * X + Y) { py = i - 2L * X; px = 0; }
    else { py = i - 2L * X - Y; px = X - 1; }
    const long l = labels[py * X + px];
    if (l >= 1 && l <= n) flags[l - 1] = 1;
}

__global__ void k_lookup_exact(const int32_t *__restrict__ labels, int Y, int X, const int64_t *__restrict__ qy, const int64_t *__restrict__ qx,
                               long n, int32_t *__restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t py = qy[i], px = qx[i];
    out[i] = (py < 0 || py >= Y || px < 0 || px >= X) ? -1 : labels[py * X + px];
}

__device__ __forceinline__ unsigned ev_hash(unsigned long long k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return (unsigned)k;
}

// the slot of id, claimed when the id is new; -1 for the empty marker (and for a full table, which the capacity rules out)
__device__ __forceinline__ int ev_claim(unsigned long long *keys, unsigned mask, int64_t id)
{
    const unsigned long long k = (unsigned long long)id;
    if (k == EV_EMPTY) return -1;
    unsigned h = ev_hash(k) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
        const unsigned long long old = atomicCAS(&keys[h], EV_EMPTY, k);
        if (old == EV_EMPTY || old == k) return (int)h;
    }
    return -1;
}

// the set bits of id (0: in no set) and the previous row that holds it
__device__ __forceinline__ int ev_find(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ info,
                                       const int32_t *__restrict__ prow, unsigned mask, int64_t id, int &row)
{
    const unsigned long long k = (unsigned long long)id;
    row = -1;
    if (k == EV_EMPTY) return 0;
    unsigned h = ev_hash(k) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
        const unsigned long long at = keys[h];
        if (at == k) { row = prow[h]; return info[h]; }
        if (at == EV_EMPTY) return 0;
    }
    return 0;
}

__global__ void k_ev_init(unsigned long long *__restrict__ keys, int32_t *__restrict__ info, int32_t *__restrict__ prow, long cap)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (long)gridDim.x * blockDim.x) {
        keys[i] = EV_EMPTY;
        info[i] = 0;
        prow[i] = 0x7fffffff;
    }
}

__global__ void k_ev_insert(const int64_t *__restrict__ id_prev, const uint8_t *__restrict__ sel_prev, const uint8_t *__restrict__ pos_prev, long n_prev,
                            const int64_t *__restrict__ id_cur, const uint8_t *__restrict__ sel_cur, const uint8_t *__restrict__ pos_cur,
                            const uint8_t *__restrict__ edge_cur, long n_cur, const int64_t *__restrict__ first_edge_ids, long n_first,
                            unsigned long long *keys, int32_t *info, int32_t *prow, unsigned mask)
{
    const long total = n_prev + n_cur + n_first;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int64_t id;
        int bits = 0, row = -1;
        if (i < n_prev) {
            if (!sel_prev[i]) continue;
            id = id_prev[i];
            bits = EV_P | (pos_prev[i] ? EV_PPOS : 0);
            row = (int)i;
        } else if (i < n_prev + n_cur) {
            const long r = i - n_prev;
            id = id_cur[r];
            if (sel_cur[r]) bits = EV_C | (pos_cur[r] ? EV_CPOS : 0);
            if (edge_cur[r]) bits |= EV_E;
            if (!bits) continue;
        } else {
            id = first_edge_ids[i - n_prev - n_cur];
            bits = EV_F;
        }
        const int h = ev_claim(keys, mask, id);
        if (h < 0) continue;
        atomicOr(&info[h], bits);
        if (row >= 0) atomicMin(&prow[h], row);
    }
}

// every neighbour of previous row r is a selected row whose id neither vanished nor sits on the first frame's border
__device__ __forceinline__ bool ev_neighbourhood_stays(const int32_t *__restrict__ off, const int32_t *__restrict__ adj, long n_adj, int r, long n_rows,
                                                       const int64_t *__restrict__ id, const uint8_t *__restrict__ sel,
                                                       const unsigned long long *__restrict__ keys, const int32_t *__restrict__ info,
                                                       const int32_t *__restrict__ prow, unsigned mask)
{
    int b, e, unused;
    row_of(off, r, n_adj, b, e);
    for (int a = b; a < e; ++a) {
        const long n = adj[a];
        if (n < 0 || n >= n_rows || !sel[n]) return false;
        const int g = ev_find(keys, info, prow, mask, id[n], unused);
        if (!(g & EV_C) || (g & EV_F)) return false;
    }
    return true;
}

__global__ void k_ev_classify(const int64_t *__restrict__ id_prev, const uint8_t *__restrict__ sel_prev, const int32_t *__restrict__ off_prev,
                              const int32_t *__restrict__ adj_prev, long n_prev, long n_adj_prev, const int64_t *__restrict__ id_cur,
                              const uint8_t *__restrict__ sel_cur, const int32_t *__restrict__ off_cur, const int32_t *__restrict__ adj_cur, long n_cur,
                              long n_adj_cur, const int32_t *__restrict__ under, const unsigned long long *__restrict__ keys,
                              const int32_t *__restrict__ info, const int32_t *__restrict__ prow, unsigned mask, uint8_t *__restrict__ delam,
                              uint8_t *__restrict__ diff, uint8_t *__restrict__ division, int32_t *__restrict__ n_match, int32_t *__restrict__ mother_row)
{
    const long total = n_prev + n_cur;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        if (i < n_prev) {
            const int r = (int)i;
            bool is_delam = false, is_diff = false;
            if (sel_prev[r]) {
                int holder;
                const int f = ev_find(keys, info, prow, mask, id_prev[r], holder);
                is_delam = (f & EV_P) && !(f & EV_C) && !(f & EV_F);
                is_diff = (f & EV_P) && (f & EV_C) && (f & EV_CPOS) && !(f & EV_PPOS) && holder == r;
                if ((is_delam || is_diff) &&
                    !ev_neighbourhood_stays(off_prev, adj_prev, n_adj_prev, r, n_prev, id_prev, sel_prev, keys, info, prow, mask))
                    is_delam = is_diff = false;
            }
            delam[r] = is_delam ? 1 : 0;
            diff[r] = is_diff ? 1 : 0;
        } else {
            const int r = (int)(i - n_prev);
            int matches = 0, mother = -1;
            bool ok = false;
            if (sel_cur[r] && under[r] != -1) {
                int unused;
                const int f = ev_find(keys, info, prow, mask, id_cur[r], unused);
                ok = (f & EV_C) && !(f & EV_P) && !(f & EV_E);
                if (ok) {
                    const int mine = under[r];
                    int b, e;
                    row_of(off_cur, r, n_adj_cur, b, e);
                    for (int a = b; a < e; ++a) {
                        const long n = adj_cur[a];
                        if (n < 0 || n >= n_cur || !sel_cur[n]) { ok = false; break; }
                        const int g = ev_find(keys, info, prow, mask, id_cur[n], unused);
                        if ((g & EV_P) && (g & EV_C) && !(g & EV_E) && under[n] != -1 && under[n] == mine) {
                            ++matches;
                            if ((int)n > mother) mother = (int)n;
                        }
                    }
                    ok = ok && matches > 0;
                }
            }
            division[r] = ok ? 1 : 0;
            n_match[r] = ok ? matches : 0;
            mother_row[r] = ok ? mother : -1;
        }
    }
}

struct EventArgs {
    const int64_t *id_prev; const uint8_t *sel_prev, *pos_prev; const int32_t *off_prev, *adj_prev; int64_t n_prev, n_adj_prev;
    const int64_t *id_cur; const uint8_t *sel_cur, *pos_cur; const int32_t *off_cur, *adj_cur; int64_t n_cur, n_adj_cur;
    const uint8_t *edge_cur; const int32_t *under_cur; const int64_t *first_edge_ids; int64_t n_first_edge;
    uint8_t *delam, *diff, *division; int32_t *n_match, *mother_row;
};

static int check_event_args(const char *who, const EventArgs &a)
{
    if (int rc = check_graph(who, a.off_prev, a.adj_prev, a.n_prev, a.n_adj_prev, 0)) return rc;
    if (int rc = check_graph(who, a.off_cur, a.adj_cur, a.n_cur, a.n_adj_cur, 0)) return rc;
    if (a.n_first_edge < 0 || a.n_first_edge > 0x7fffffff || (a.n_first_edge > 0 && !a.first_edge_ids))
        return fail(TIP_ERR_ARG, "%s: first_edge_ids (%ld)", who, (long)a.n_first_edge);
    if (a.n_prev + a.n_cur + a.n_first_edge > 0x1fffffff) return fail(TIP_ERR_ARG, "%s: too many ids for one table", who);
    if (a.n_prev > 0 && (!a.id_prev || !a.sel_prev || !a.pos_prev || !a.delam || !a.diff))
        return fail(TIP_ERR_ARG, "%s: the previous frame's rows or flags are NULL", who);
    if (a.n_cur > 0 && (!a.id_cur || !a.sel_cur || !a.pos_cur || !a.edge_cur || !a.under_cur || !a.division || !a.n_match || !a.mother_row))
        return fail(TIP_ERR_ARG, "%s: the current frame's rows or outputs are NULL", who);
    return TIP_OK;
}

// a HOST CSR before it is uploaded: offsets that rise from 0 to n_adj (a label is only ever compared, so any value may stand in adj)
static int check_host_rows(const char *who, const char *which, const int32_t *off, int64_t n, int64_t n_adj)
{
    if (off[0] != 0 || off[n] != n_adj) return fail(TIP_ERR_ARG, "%s: %s offsets run from %d to %d, adj has %ld entries", who, which, off[0], off[n], (long)n_adj);
    for (int64_t r = 0; r < n; ++r)
        if (off[r + 1] < off[r]) return fail(TIP_ERR_ARG, "%s: %s offsets decrease at row %ld", who, which, (long)r);
    return TIP_OK;
}

static int event_flags_launch(const EventArgs &a)
{
    const long entries = (long)(a.n_prev + a.n_cur + a.n_first_edge), rows = (long)(a.n_prev + a.n_cur);
    if (rows == 0) return TIP_OK;
    long cap = 64;
    while (cap < 2 * entries) cap <<= 1;
    WsGuard ws;
    unsigned long long *keys = ws.get<unsigned long long>((size_t)cap);
    int32_t *info = ws.get<int32_t>((size_t)cap), *prow = ws.get<int32_t>((size_t)cap);
    if (!keys || !info || !prow) return TIP_ERR_NOMEM;
    const unsigned mask = (unsigned)(cap - 1);
    auto blocks = [](long n) { const int b = cdiv(n, EV_BLOCK); return b < 1 ? 1 : (b > EV_MAX_BLOCKS ? EV_MAX_BLOCKS : b); };
    TIP_LAUNCH("events_init", k_ev_init, dim3(blocks(cap)), dim3(EV_BLOCK), 0, keys, info, prow, cap);
    TIP_LAUNCH("events_insert", k_ev_insert, dim3(blocks(entries)), dim3(EV_BLOCK), 0, a.id_prev, a.sel_prev, a.pos_prev, (long)a.n_prev, a.id_cur,
               a.sel_cur, a.pos_cur, a.edge_cur, (long)a.n_cur, a.first_edge_ids, (long)a.n_first_edge, keys, info, prow, mask);
    TIP_LAUNCH("events_classify", k_ev_classify, dim3(blocks(rows)), dim3(EV_BLOCK), 0, a.id_prev, a.sel_prev, a.off_prev, a.adj_prev, (long)a.n_prev,
               (long)a.n_adj_prev, a.id_cur, a.sel_cur, a.off_cur, a.adj_cur, (long)a.n_cur, (long)a.n_adj_cur, a.under_cur,
               (const unsigned long long *)keys, (const int32_t *)info, (const int32_t *)prow, mask, a.delam, a.diff, a.division, a.n_match,
               a.mother_row);
    return TIP_OK;
}

static int check_border_args(const char *who, const int32_t *labels, int y, int x, int64_t n, const uint8_t *flags)
{
    if (!labels || y < 1 || x < 1 || n < 0 || n > 0x7fffffff) return fail(TIP_ERR_ARG, "%s: bad arguments", who);
    if (n > 0 && !flags) return fail(TIP_ERR_ARG, "%s: flags is NULL", who);
    return TIP_OK;
}

static int border_rows_launch(const int32_t *labels, int y, int x, int64_t n, uint8_t *flags)
{
    if (n == 0) return TIP_OK;
    TIP_HIP(hipMemsetAsync(flags, 0, (size_t)n, ctx().stream));
    TIP_LAUNCH("border_rows", k_border_rows, dim3(cdiv(2L * x + 2L * y, EV_BLOCK)), dim3(EV_BLOCK), 0, labels, y, x, (long)n, flags);
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_border_rows_i32_dev(const int32_t *labels, int y, int x, int64_t n, uint8_t *flags)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_border_args("tip_border_rows_i32_dev", labels, y, x, n, flags)) return rc;
    return border_rows_launch(labels, y, x, n, flags);
}

int tip_border_rows_i32(const int32_t *labels, int y, int x, int64_t n, uint8_t *flags)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_border_args("tip_border_rows_i32", labels, y, x, n, flags)) return rc;
    if (n == 0) return TIP_OK;
    Staging st;
    const int32_t *dl = st.in(labels, (size_t)y * x);
    uint8_t *df = st.out(flags, (size_t)n);
    if (st.rc) return st.rc;
    if (int rc = border_rows_launch(dl, y, x, n, df)) return rc;
    return st.finish();
}

int tip_lookup_i32_dev(const int32_t *labels, int y, int x, const int64_t *qy_host, const int64_t *qx_host, int64_t n, int32_t *out_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!labels || y < 1 || x < 1 || n < 0) return fail(TIP_ERR_ARG, "tip_lookup_i32_dev: bad arguments");
    if (n == 0) return TIP_OK;
    if (!qy_host || !qx_host || !out_host) return fail(TIP_ERR_ARG, "tip_lookup_i32_dev: null pointer");
    Staging st;
    const int64_t *dy = st.in(qy_host, (size_t)n), *dx = st.in(qx_host, (size_t)n);
    int32_t *dout = st.out(out_host, (size_t)n);
    if (st.rc) return st.rc;
    TIP_LAUNCH("lookup_exact", k_lookup_exact, dim3(cdiv(n, EV_BLOCK)), dim3(EV_BLOCK), 0, labels, y, x, dy, dx, (long)n, dout);
    return st.finish();
}

int tip_event_flags_i32_dev(const int64_t *id_prev, const uint8_t *sel_prev, const uint8_t *pos_prev, const int32_t *off_prev,
                            const int32_t *adj_prev, int64_t n_prev, int64_t n_adj_prev, const int64_t *id_cur, const uint8_t *sel_cur,
                            const uint8_t *pos_cur, const int32_t *off_cur, const int32_t *adj_cur, int64_t n_cur, int64_t n_adj_cur,
                            const uint8_t *edge_cur, const int32_t *under_cur, const int64_t *first_edge_ids, int64_t n_first_edge,
                            uint8_t *delam, uint8_t *diff, uint8_t *division, int32_t *n_match, int32_t *mother_row)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    const EventArgs a = {id_prev, sel_prev, pos_prev, off_prev, adj_prev, n_prev, n_adj_prev, id_cur, sel_cur, pos_cur, off_cur, adj_cur, n_cur,
                         n_adj_cur, edge_cur, under_cur, first_edge_ids, n_first_edge, delam, diff, division, n_match, mother_row};
    if (int rc = check_event_args("tip_event_flags_i32_dev", a)) return rc;
    return event_flags_launch(a);
}

int tip_event_flags_i32(const int64_t *id_prev, const uint8_t *sel_prev, const uint8_t *pos_prev, const int32_t *off_prev,
                        const int32_t *adj_prev, int64_t n_prev, int64_t n_adj_prev, const int64_t *id_cur, const uint8_t *sel_cur,
                        const uint8_t *pos_cur, const int32_t *off_cur, const int32_t *adj_cur, int64_t n_cur, int64_t n_adj_cur,
                        const uint8_t *edge_cur, const int32_t *under_cur, const int64_t *first_edge_ids, int64_t n_first_edge,
                        uint8_t *delam, uint8_t *diff, uint8_t *division, int32_t *n_match, int32_t *mother_row)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    const char *who = "tip_event_flags_i32";
    EventArgs a = {id_prev, sel_prev, pos_prev, off_prev, adj_prev, n_prev, n_adj_prev, id_cur, sel_cur, pos_cur, off_cur, adj_cur, n_cur,
                   n_adj_cur, edge_cur, under_cur, first_edge_ids, n_first_edge, delam, diff, division, n_match, mother_row};
    if (int rc = check_event_args(who, a)) return rc;
    if (int rc = check_host_rows(who, "the previous frame's", off_prev, n_prev, n_adj_prev)) return rc;
    if (int rc = check_host_rows(who, "the current frame's", off_cur, n_cur, n_adj_cur)) return rc;
    for (int64_t r = 0; r < n_prev + n_cur; ++r)
        if ((unsigned long long)(r < n_prev ? id_prev[r] : id_cur[r - n_prev]) == EV_EMPTY) return fail(TIP_ERR_ARG, "%s: id INT64_MIN is reserved", who);
    if (n_prev + n_cur == 0) return TIP_OK;
    Staging st;
    a.id_prev = st.in(id_prev, (size_t)n_prev), a.sel_prev = st.in(sel_prev, (size_t)n_prev), a.pos_prev = st.in(pos_prev, (size_t)n_prev);
    a.off_prev = st.in(off_prev, (size_t)n_prev + 1), a.adj_prev = st.in(adj_prev, (size_t)n_adj_prev);
    a.id_cur = st.in(id_cur, (size_t)n_cur), a.sel_cur = st.in(sel_cur, (size_t)n_cur), a.pos_cur = st.in(pos_cur, (size_t)n_cur);
    a.off_cur = st.in(off_cur, (size_t)n_cur + 1), a.adj_cur = st.in(adj_cur, (size_t)n_adj_cur);
    a.edge_cur = st.in(edge_cur, (size_t)n_cur), a.under_cur = st.in(under_cur, (size_t)n_cur);
    a.first_edge_ids = st.in(first_edge_ids, (size_t)n_first_edge);
    a.delam = st.out(delam, (size_t)n_prev), a.diff = st.out(diff, (size_t)n_prev), a.division = st.out(division, (size_t)n_cur);
    a.n_match = st.out(n_match, (size_t)n_cur), a.mother_row = st.out(mother_row, (size_t)n_cur);
    if (st.rc) return st.rc;
    if (int rc = event_flags_launch(a)) return rc;
    return st.finish();
}

}  // extern "C"
