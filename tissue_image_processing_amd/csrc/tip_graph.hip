// tip_graph.hip -- the per-cell features that walk the cell neighbour graph (ti.py:1752-1791 calculate_n_neighbors_from_type,
// 2513-2543 find_second_order_neighbors, 1065-1096 / 1844-1872 the contact-length loop, 803-843 the neighbour sums behind
// calculate_neighbors_correlation_function).  The reference answers every table row with pandas look-ups over Python sets; here
// the graph is a CSR adjacency (offsets int32[n + 1], adj int32[...] of 1-based labels, ASCENDING within a row) and every feature
// is one launch over the query rows.  tip_csr.h has the pieces shared with tip_order.hip: label_ok / row_of / row_find, the
// rank rule and its sort kernel and the host checks of a CSR; the scan is scan_i32_dev (tip_label.hip, launched as "csr_scan").
//
//   k_csr_count / (scan_i32_dev) / k_csr_fill / k_rank_sort ("csr_sort")
//                    the CSR from the unique (hi, lo) pairs of tip_neighbor_pairs_i32: a pair gives both directions when
//                    working[hi - 1] is set (or working is NULL) -- upstream's find_neighbors visits working cells only and finds
//                    a pair from its larger label (ti.py:1827-1838).  Degrees with atomicAdd, one workgroup's exclusive scan,
//                    slots handed out with atomicAdd into a scratch copy, then one wavefront per row ranks the row's entries
//                    and writes them in ascending order.  A pair with a label outside 1..n takes no part.
//   k_graph_counts   one thread per query row: degree, or the neighbours that pass valid / empty / type tests.
//   k_graph_second   one wavefront per query row i: for every intermediate j in N(i) with valid[j] == 1 the lanes stride over
//                    N(j); a candidate k counts when k != i, valid[k] == 1, it passes the selector and NO earlier qualifying
//                    intermediate j' of the row holds it (binary search in the sorted row N(j')).  Exact de-duplication without a
//                    hash or atomics and without a degree cap; positions inside the wavefront come from __ballot, so a second
//                    call (after the caller's scan of the sizes) writes the members in the same deterministic order.
//   k_edge_weights   one thread per contact triple (hi, lo, pixels): the pixel count goes to the two edges hi -> lo and lo -> hi
//                    of the CSR (binary search of the neighbour in the row); an edge without a triple keeps 0, a triple whose
//                    pair is no edge is dropped (upstream asks about members of `neighbors` only).
//   k_contact_sums   one thread per query row: the sum of the weights of the selected neighbours, their number and, for the
//                    histogram, the per-edge values in CSR form.
//   k_neighbor_state one thread per query row: sum of state[j] (__dadd_rn, in row order) and number of the neighbours j with
//                    member[j].  It searches no row, so its host form does not ask for ascending rows.
// Every read of adj is clamped to n_adj and every label is checked against 1..n, so a malformed device CSR gives wrong numbers,
// never an access outside the caller's arrays; the host forms check their CSR before it is uploaded (Staging, tip_internal.h).
#include "tip_csr.h"
#include "tip_typesel.h"

namespace tip {

constexpr int G_ALL = TIP_GRAPH_ALL, G_VALID = TIP_GRAPH_VALID, G_INVALID = TIP_GRAPH_INVALID, G_TYPE = TIP_GRAPH_TYPE;

__device__ __forceinline__ bool pair_takes_part(const int32_t *__restrict__ pairs, long p, int n, const uint8_t *__restrict__ working,
                                                int &hi, int &lo)
{
    hi = pairs[2 * p];
    lo = pairs[2 * p + 1];
    if (!label_ok(hi, n) || !label_ok(lo, n) || hi == lo) return false;
    return !working || working[hi - 1];
}

__global__ void k_csr_count(const int32_t *__restrict__ pairs, long np, int n, const uint8_t *__restrict__ working, int32_t *__restrict__ deg)
{
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int hi, lo;
    if (p >= np || !pair_takes_part(pairs, p, n, working, hi, lo)) return;
    atomicAdd(&deg[hi - 1], 1);
    atomicAdd(&deg[lo - 1], 1);
}

__global__ void k_csr_fill(const int32_t *__restrict__ pairs, long np, int n, const uint8_t *__restrict__ working,
                           const int32_t *__restrict__ offsets, int32_t *__restrict__ cursor, int32_t *__restrict__ raw, long raw_cap)
{
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int hi, lo;
    if (p >= np || !pair_takes_part(pairs, p, n, working, hi, lo)) return;
    const long a = (long)offsets[hi - 1] + atomicAdd(&cursor[hi - 1], 1);
    const long b = (long)offsets[lo - 1] + atomicAdd(&cursor[lo - 1], 1);
    if (a >= 0 && a < raw_cap) raw[a] = lo;
    if (b >= 0 && b < raw_cap) raw[b] = hi;
}

__global__ void k_graph_counts(const int32_t *__restrict__ offsets, const int32_t *__restrict__ adj, int n, long n_adj,
                               const uint8_t *__restrict__ valid, const uint8_t *__restrict__ empty, const uint8_t *__restrict__ type,
                               const int32_t *__restrict__ query, long m, int mode, int sel_kind, int bit, int64_t *__restrict__ out)
{
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    const long r = query ? (long)query[q] : q;
    if (r < 0 || r >= n) { out[q] = -1; return; }
    int b, e;
    row_of(offsets, (int)r, n_adj, b, e);
    int64_t cnt = 0;
    if (mode == G_ALL) cnt = e - b;
    else
        for (int a = b; a < e; ++a) {
            const int k = adj[a] - 1;
            if ((unsigned)k >= (unsigned)n || (empty && empty[k] != 0)) continue;
            if (mode == G_INVALID) cnt += valid[k] == 0 ? 1 : 0;
            else cnt += (valid[k] == 1 && (mode == G_VALID || sp_selected(type[k], sel_kind, bit))) ? 1 : 0;
        }
    out[q] = cnt;
}

__global__ __launch_bounds__(CSR_BLOCK) void k_graph_second(const int32_t *__restrict__ offsets, const int32_t *__restrict__ adj, int n, long n_adj,
                                                          const uint8_t *__restrict__ valid, const uint8_t *__restrict__ type,
                                                          const int32_t *__restrict__ query, long m, int sel_kind, int bit,
                                                          int64_t *__restrict__ sizes, const int64_t *__restrict__ member_offsets,
                                                          int32_t *__restrict__ members, long members_cap)
{
    const long q = (long)blockIdx.x * CSR_WPB + (threadIdx.x >> 6);      // the same for every lane of a wavefront
    const int lane = threadIdx.x & (CSR_WAVE - 1);
    if (q >= m) return;
    const long r = query ? (long)query[q] : q;
    if (r < 0 || r >= n) {
        if (lane == 0 && sizes) sizes[q] = -1;
        return;
    }
    int ib, ie;
    row_of(offsets, (int)r, n_adj, ib, ie);
    const long base = members ? member_offsets[q] : 0;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    long total = 0;
    for (int pj = ib; pj < ie; ++pj) {
        const int j = adj[pj] - 1;
        if ((unsigned)j >= (unsigned)n || valid[j] != 1) continue;
        int jb, je;
        row_of(offsets, j, n_adj, jb, je);
        for (int kb = jb; kb < je; kb += CSR_WAVE) {
            const int a = kb + lane;
            bool take = false;
            int k = 0;
            if (a < je) {
                k = adj[a];
                const int kk = k - 1;
                take = (unsigned)kk < (unsigned)n && kk != (int)r && valid[kk] == 1 && (sel_kind == 0 || sp_selected(type[kk], sel_kind, bit));
                for (int pe = ib; take && pe < pj; ++pe) {          // already reached through an earlier intermediate?
                    const int je2 = adj[pe] - 1;
                    if ((unsigned)je2 >= (unsigned)n || valid[je2] != 1) continue;
                    int eb, ee;
                    row_of(offsets, je2, n_adj, eb, ee);
                    if (row_find(adj, eb, ee, k) >= 0) take = false;
                }
            }
            const unsigned long long mask = __ballot(take);
            if (take && members) {
                const long pos = base + total + __popcll(mask & below);
                if (pos >= 0 && pos < members_cap) members[pos] = k;
            }
            total += __popcll(mask);
        }
    }
    if (lane == 0 && sizes) sizes[q] = total;
}

__global__ void k_edge_weights(const int32_t *__restrict__ pairs, const int64_t *__restrict__ counts, long nt,
                               const int32_t *__restrict__ offsets, const int32_t *__restrict__ adj, int n, long n_adj,
                               int64_t *__restrict__ weight)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int hi = pairs[2 * t], lo = pairs[2 * t + 1];
    if (!label_ok(hi, n) || !label_ok(lo, n) || hi <= lo) return;   // upstream asks for (larger label, smaller label) only
    int b, e;
    row_of(offsets, hi - 1, n_adj, b, e);
    int pos = row_find(adj, b, e, lo);
    if (pos >= 0) weight[pos] = counts[t];
    row_of(offsets, lo - 1, n_adj, b, e);
    pos = row_find(adj, b, e, hi);
    if (pos >= 0) weight[pos] = counts[t];
}

__global__ void k_contact_sums(const int32_t *__restrict__ offsets, const int32_t *__restrict__ adj, const int64_t *__restrict__ weight, int n,
                               long n_adj, const uint8_t *__restrict__ valid, const uint8_t *__restrict__ type,
                               const int32_t *__restrict__ query, long m, int mode, int sel_kind, int bit, int64_t *__restrict__ sums,
                               int64_t *__restrict__ n_sel, const int64_t *__restrict__ value_offsets, int64_t *__restrict__ values,
                               int32_t *__restrict__ value_labels, long values_cap)
{
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    const long r = query ? (long)query[q] : q;
    if (r < 0 || r >= n) {
        if (sums) sums[q] = -1;
        if (n_sel) n_sel[q] = -1;
        return;
    }
    int b, e;
    row_of(offsets, (int)r, n_adj, b, e);
    const long base = values ? value_offsets[q] : 0;
    int64_t sum = 0, cnt = 0;
    for (int a = b; a < e; ++a) {
        const int k = adj[a] - 1;
        if ((unsigned)k >= (unsigned)n) continue;
        const bool sel = mode == G_ALL || (mode == G_VALID ? valid[k] == 1 : sp_selected(type[k], sel_kind, bit));
        if (!sel) continue;
        const int64_t w = weight[a];
        sum += w;
        if (values) {
            const long pos = base + cnt;
            if (pos >= 0 && pos < values_cap) {
                values[pos] = w;
                if (value_labels) value_labels[pos] = k + 1;
            }
        }
        ++cnt;
    }
    if (sums) sums[q] = sum;
    if (n_sel) n_sel[q] = cnt;
}

__global__ void k_neighbor_state(const int32_t *__restrict__ offsets, const int32_t *__restrict__ adj, int n, long n_adj,
                                 const uint8_t *__restrict__ member, const double *__restrict__ state, const int32_t *__restrict__ query,
                                 long m, double *__restrict__ nb_sum, int64_t *__restrict__ nb_cnt)
{
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    const long r = query ? (long)query[q] : q;
    double sum = 0.0;
    int64_t cnt = 0;
    if (r >= 0 && r < n) {
        int b, e;
        row_of(offsets, (int)r, n_adj, b, e);
        for (int a = b; a < e; ++a) {
            const int j = adj[a] - 1;
            if ((unsigned)j >= (unsigned)n || member[j] == 0) continue;
            sum = __dadd_rn(sum, state[j]);
            ++cnt;
        }
    } else cnt = -1;
    nb_sum[q] = sum;
    nb_cnt[q] = cnt;
}

// ---- CSR ------------------------------------------------------------------------------------------------------------------------
static int check_csr_args(const char *who, const int32_t *pairs, int64_t np, int64_t n, const int32_t *offsets, const int32_t *adj, int64_t cap)
{
    if (n < 0 || n > 0x7ffffffe || np < 0 || np > 0x3fffffff || cap < 0 || cap > 0x7fffffff)
        return fail(TIP_ERR_ARG, "%s: n = %ld rows, %ld pairs, capacity %ld", who, (long)n, (long)np, (long)cap);
    if (!offsets || (np > 0 && !pairs) || (cap > 0 && !adj)) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    return TIP_OK;
}

static int neighbor_csr_dev(const char *who, const int32_t *pairs, int64_t np, int64_t n, const uint8_t *working, int32_t *offsets,
                            int32_t *adj, int64_t cap, int64_t *n_adj_host)
{
    Ctx &c = ctx();
    WsGuard ws;
    const size_t raw_cap = (size_t)2 * np;
    int32_t *deg = ws.get<int32_t>((size_t)n), *raw = ws.get<int32_t>(raw_cap);
    if (!deg || !raw) return TIP_ERR_NOMEM;
    if (n) TIP_HIP(hipMemsetAsync(deg, 0, (size_t)n * 4, c.stream));
    if (np && n) TIP_LAUNCH("csr_count", k_csr_count, dim3(cdiv(np, 256)), dim3(256), 0, pairs, (long)np, (int)n, working, deg);
    if (int rc = scan_i32_dev(deg, offsets, (int)n)) return rc;
    if (n_adj_host) {
        int32_t total = 0;
        TIP_HIP(hipMemcpyAsync(&total, offsets + n, 4, hipMemcpyDeviceToHost, c.stream));
        TIP_HIP(hipStreamSynchronize(c.stream));
        *n_adj_host = total;
        if (total > cap) return fail(TIP_ERR_OVERFLOW, "%s: the adjacency has %ld entries, capacity %ld", who, (long)total, (long)cap);
    }
    if (np && n) {
        TIP_HIP(hipMemsetAsync(deg, 0, (size_t)n * 4, c.stream));
        TIP_LAUNCH("csr_fill", k_csr_fill, dim3(cdiv(np, 256)), dim3(256), 0, pairs, (long)np, (int)n, working, (const int32_t *)offsets, deg,
                   raw, (long)raw_cap);
        TIP_LAUNCH("csr_sort", k_rank_sort<int32_t>, dim3(cdiv(n, CSR_WPB)), dim3(CSR_BLOCK), 0, (const int32_t *)offsets, (const int32_t *)nullptr,
                   (const int32_t *)raw, (long)raw_cap, adj, (int)n, (long)cap, 0);
    }
    return TIP_OK;
}

// ---- launches on device arrays (arguments checked by the entry points) ------------------------------------------------------------
static int graph_counts_launch(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *empty,
                               const uint8_t *type, const int32_t *query, int64_t m, int mode, Selector sel, int64_t *out)
{
    if (m == 0) return TIP_OK;
    TIP_LAUNCH("graph_counts", k_graph_counts, dim3(cdiv(m, 256)), dim3(256), 0, offsets, adj, (int)n, (long)n_adj, valid, empty, type, query,
               (long)m, mode, sel.kind, sel.bit, out);
    return TIP_OK;
}

static int graph_second_launch(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *type,
                               const int32_t *query, int64_t m, Selector sel, int64_t *sizes, const int64_t *member_offsets,
                               int32_t *members, int64_t members_cap)
{
    if (m == 0) return TIP_OK;
    TIP_LAUNCH("graph_second", k_graph_second, dim3(cdiv(m, CSR_WPB)), dim3(CSR_BLOCK), 0, offsets, adj, (int)n, (long)n_adj, valid, type, query,
               (long)m, sel.kind, sel.bit, sizes, member_offsets, members, (long)members_cap);
    return TIP_OK;
}

static int contact_sums_launch(const int32_t *pairs, const int64_t *counts, int64_t nt, const int32_t *offsets, const int32_t *adj, int64_t n,
                               int64_t n_adj, const uint8_t *valid, const uint8_t *type, const int32_t *query, int64_t m, int mode,
                               Selector sel, int64_t *sums, int64_t *n_sel, const int64_t *value_offsets, int64_t *values,
                               int32_t *value_labels, int64_t values_cap)
{
    if (m == 0) return TIP_OK;
    WsGuard ws;
    int64_t *weight = ws.get<int64_t>((size_t)n_adj);
    if (!weight) return TIP_ERR_NOMEM;
    if (n_adj) TIP_HIP(hipMemsetAsync(weight, 0, (size_t)n_adj * 8, ctx().stream));
    if (nt && n_adj)
        TIP_LAUNCH("edge_weights", k_edge_weights, dim3(cdiv(nt, 256)), dim3(256), 0, pairs, counts, (long)nt, offsets, adj, (int)n, (long)n_adj,
                   weight);
    TIP_LAUNCH("contact_sums", k_contact_sums, dim3(cdiv(m, 256)), dim3(256), 0, offsets, adj, (const int64_t *)weight, (int)n, (long)n_adj, valid,
               type, query, (long)m, mode, sel.kind, sel.bit, sums, n_sel, value_offsets, values, value_labels, (long)values_cap);
    return TIP_OK;
}

static int neighbor_state_launch(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *member, const double *state,
                                 const int32_t *query, int64_t m, double *nb_sum, int64_t *nb_cnt)
{
    if (m == 0) return TIP_OK;
    TIP_LAUNCH("neighbor_state", k_neighbor_state, dim3(cdiv(m, 256)), dim3(256), 0, offsets, adj, (int)n, (long)n_adj, member, state, query, (long)m,
               nb_sum, nb_cnt);
    return TIP_OK;
}

// ---- argument checks shared by the host and the device forms -----------------------------------------------------------------
static int check_counts_args(const char *who, const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid,
                             const uint8_t *type, int64_t m, int mode, int sel_bit, int sel_positive, const int64_t *out, Selector &sel)
{
    if (int rc = check_graph(who, offsets, adj, n, n_adj, m)) return rc;
    if (mode < G_ALL || mode > G_TYPE) return fail(TIP_ERR_ARG, "%s: mode %d (0 all, 1 valid, 2 invalid, 3 type)", who, mode);
    if (mode == G_TYPE)
        if (int rc = parse_selector(who, sel_bit, sel_positive, false, sel)) return rc;
    if (n > 0 && ((mode != G_ALL && !valid) || (mode == G_TYPE && !type))) return fail(TIP_ERR_ARG, "%s: mode %d needs the valid / type bytes", who, mode);
    if (m > 0 && !out) return fail(TIP_ERR_ARG, "%s: no output", who);
    return TIP_OK;
}

static int check_second_args(const char *who, const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid,
                             const uint8_t *type, int64_t m, int sel_bit, int sel_positive, const int64_t *sizes, const int64_t *member_offsets,
                             const int32_t *members, int64_t members_cap, Selector &sel)
{
    if (int rc = check_graph(who, offsets, adj, n, n_adj, m)) return rc;
    if (int rc = parse_selector(who, sel_bit, sel_positive, true, sel)) return rc;
    if (n > 0 && (!valid || (sel.kind && !type))) return fail(TIP_ERR_ARG, "%s: the valid / type bytes", who);
    if (m > 0 && !sizes && !members) return fail(TIP_ERR_ARG, "%s: no output", who);
    if (members && (!member_offsets || members_cap < 0)) return fail(TIP_ERR_ARG, "%s: members need member_offsets and a capacity", who);
    return TIP_OK;
}

static int check_contact_args(const char *who, const int32_t *pairs, const int64_t *counts, int64_t nt, const int32_t *offsets, const int32_t *adj,
                              int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *type, int64_t m, int mode, int sel_bit,
                              int sel_positive, const int64_t *sums, const int64_t *n_sel, const int64_t *value_offsets, const int64_t *values,
                              const int32_t *value_labels, int64_t values_cap, Selector &sel)
{
    if (int rc = check_graph(who, offsets, adj, n, n_adj, m)) return rc;
    if (nt < 0 || nt > 0x7fffffff || (nt > 0 && (!pairs || !counts))) return fail(TIP_ERR_ARG, "%s: the contact triples (%ld)", who, (long)nt);
    if (mode != G_ALL && mode != G_VALID && mode != G_TYPE) return fail(TIP_ERR_ARG, "%s: mode %d (0 all, 1 valid, 3 type)", who, mode);
    if (mode == G_TYPE)
        if (int rc = parse_selector(who, sel_bit, sel_positive, false, sel)) return rc;
    if (n > 0 && ((mode == G_VALID && !valid) || (mode == G_TYPE && !type))) return fail(TIP_ERR_ARG, "%s: mode %d needs the valid / type bytes", who, mode);
    if (m > 0 && !sums && !n_sel && !values) return fail(TIP_ERR_ARG, "%s: no output", who);
    if ((values || value_labels) && (!values || !value_offsets || values_cap < 0))
        return fail(TIP_ERR_ARG, "%s: per-edge values need value_offsets and a capacity", who);
    return TIP_OK;
}

static int check_state_args(const char *who, const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *member,
                            const double *state, int64_t m, const double *nb_sum, const int64_t *nb_cnt)
{
    if (int rc = check_graph(who, offsets, adj, n, n_adj, m)) return rc;
    if ((n > 0 && (!member || !state)) || (m > 0 && (!nb_sum || !nb_cnt))) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    return TIP_OK;
}

// a host CSR whose rows are searched: sound and ascending
static int check_sorted_host_graph(const char *who, const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const int32_t *query,
                                   int64_t m)
{
    if (int rc = check_host_graph(who, offsets, adj, n, n_adj, query, m)) return rc;
    return check_rows_ascend(who, offsets, adj, n);
}

// the capacity offsets of a two-call entry's second call (member_offsets, value_offsets), checked on the host
static int check_host_offsets(const char *who, const char *name, const int64_t *off, int64_t m, int64_t cap)
{
    for (int64_t q = 0; q < m; ++q)
        if (off[q] < 0 || off[q] > cap) return fail(TIP_ERR_ARG, "%s: %s[%ld] = %ld, capacity %ld", who, name, (long)q, (long)off[q], (long)cap);
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_neighbor_csr_i32_dev(const int32_t *pairs, int64_t n_pairs, int64_t n, const uint8_t *working, int32_t *offsets, int32_t *adj,
                             int64_t cap, int64_t *n_adj_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_csr_args("tip_neighbor_csr_i32_dev", pairs, n_pairs, n, offsets, adj, cap)) return rc;
    return neighbor_csr_dev("tip_neighbor_csr_i32_dev", pairs, n_pairs, n, working, offsets, adj, cap, n_adj_host);
}

int tip_neighbor_csr_i32(const int32_t *pairs, int64_t n_pairs, int64_t n, const uint8_t *working, int32_t *offsets, int32_t *adj, int64_t cap,
                         int64_t *n_adj)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_csr_args("tip_neighbor_csr_i32", pairs, n_pairs, n, offsets, adj, cap)) return rc;
    if (!n_adj) return fail(TIP_ERR_ARG, "tip_neighbor_csr_i32: n_adj is NULL");
    Staging st;
    int32_t *doff = st.out(offsets, (size_t)n + 1), *dadj = st.out(adj, (size_t)cap);
    const int32_t *dp = st.in(pairs, (size_t)2 * n_pairs);
    const uint8_t *dw = st.in(working, (size_t)n);
    if (st.rc) return st.rc;
    if (int rc = neighbor_csr_dev("tip_neighbor_csr_i32", dp, n_pairs, n, dw, doff, dadj, cap, n_adj)) return rc;
    st.set_count(dadj, (size_t)*n_adj);
    return st.finish();
}

int tip_graph_counts_i32_dev(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *empty,
                             const uint8_t *type, const int32_t *query, int64_t m, int mode, int sel_bit, int sel_positive, int64_t *out)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_counts_args("tip_graph_counts_i32_dev", offsets, adj, n, n_adj, valid, type, m, mode, sel_bit, sel_positive, out, sel))
        return rc;
    return graph_counts_launch(offsets, adj, n, n_adj, valid, empty, type, query, m, mode, sel, out);
}

int tip_graph_counts_i32(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *empty,
                         const uint8_t *type, const int32_t *query, int64_t m, int mode, int sel_bit, int sel_positive, int64_t *out)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_counts_args("tip_graph_counts_i32", offsets, adj, n, n_adj, valid, type, m, mode, sel_bit, sel_positive, out, sel)) return rc;
    if (int rc = check_sorted_host_graph("tip_graph_counts_i32", offsets, adj, n, n_adj, query, m)) return rc;
    if (m == 0) return TIP_OK;
    Staging st;
    const int32_t *doff = st.in(offsets, (size_t)n + 1), *dadj = st.in(adj, (size_t)n_adj), *dq = st.in(query, (size_t)m);
    const uint8_t *dvalid = st.in(valid, (size_t)n), *dempty = st.in(empty, (size_t)n), *dtype = st.in(type, (size_t)n);
    int64_t *dout = st.out(out, (size_t)m);
    if (st.rc) return st.rc;
    if (int rc = graph_counts_launch(doff, dadj, n, n_adj, dvalid, dempty, dtype, dq, m, mode, sel, dout)) return rc;
    return st.finish();
}

int tip_graph_second_i32_dev(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *type,
                             const int32_t *query, int64_t m, int sel_bit, int sel_positive, int64_t *sizes, const int64_t *member_offsets,
                             int32_t *members, int64_t members_cap)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_second_args("tip_graph_second_i32_dev", offsets, adj, n, n_adj, valid, type, m, sel_bit, sel_positive, sizes, member_offsets,
                                   members, members_cap, sel))
        return rc;
    return graph_second_launch(offsets, adj, n, n_adj, valid, type, query, m, sel, sizes, member_offsets, members, members_cap);
}

int tip_graph_second_i32(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *type,
                         const int32_t *query, int64_t m, int sel_bit, int sel_positive, int64_t *sizes, const int64_t *member_offsets,
                         int32_t *members, int64_t members_cap)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_second_args("tip_graph_second_i32", offsets, adj, n, n_adj, valid, type, m, sel_bit, sel_positive, sizes, member_offsets,
                                   members, members_cap, sel))
        return rc;
    if (int rc = check_sorted_host_graph("tip_graph_second_i32", offsets, adj, n, n_adj, query, m)) return rc;
    if (m == 0) return TIP_OK;
    if (members)
        if (int rc = check_host_offsets("tip_graph_second_i32", "member_offsets", member_offsets, m, members_cap)) return rc;
    Staging st;
    const int32_t *doff = st.in(offsets, (size_t)n + 1), *dadj = st.in(adj, (size_t)n_adj), *dq = st.in(query, (size_t)m);
    const uint8_t *dvalid = st.in(valid, (size_t)n), *dtype = st.in(type, (size_t)n);
    const int64_t *dmoff = st.in(member_offsets, (size_t)m);
    int64_t *dsizes = st.out(sizes, (size_t)m);
    int32_t *dmem = st.out(members, (size_t)members_cap, true);
    if (st.rc) return st.rc;
    if (int rc = graph_second_launch(doff, dadj, n, n_adj, dvalid, dtype, dq, m, sel, dsizes, dmoff, dmem, members_cap)) return rc;
    return st.finish();
}

int tip_contact_sums_i32_dev(const int32_t *pairs, const int64_t *counts, int64_t n_triples, const int32_t *offsets, const int32_t *adj, int64_t n,
                             int64_t n_adj, const uint8_t *valid, const uint8_t *type, const int32_t *query, int64_t m, int mode, int sel_bit,
                             int sel_positive, int64_t *sums, int64_t *n_sel, const int64_t *value_offsets, int64_t *values,
                             int32_t *value_labels, int64_t values_cap)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_contact_args("tip_contact_sums_i32_dev", pairs, counts, n_triples, offsets, adj, n, n_adj, valid, type, m, mode, sel_bit,
                                    sel_positive, sums, n_sel, value_offsets, values, value_labels, values_cap, sel))
        return rc;
    return contact_sums_launch(pairs, counts, n_triples, offsets, adj, n, n_adj, valid, type, query, m, mode, sel, sums, n_sel, value_offsets, values,
                               value_labels, values_cap);
}

int tip_contact_sums_i32(const int32_t *pairs, const int64_t *counts, int64_t n_triples, const int32_t *offsets, const int32_t *adj, int64_t n,
                         int64_t n_adj, const uint8_t *valid, const uint8_t *type, const int32_t *query, int64_t m, int mode, int sel_bit,
                         int sel_positive, int64_t *sums, int64_t *n_sel, const int64_t *value_offsets, int64_t *values, int32_t *value_labels,
                         int64_t values_cap)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    Selector sel;
    if (int rc = check_contact_args("tip_contact_sums_i32", pairs, counts, n_triples, offsets, adj, n, n_adj, valid, type, m, mode, sel_bit, sel_positive,
                                    sums, n_sel, value_offsets, values, value_labels, values_cap, sel))
        return rc;
    if (int rc = check_sorted_host_graph("tip_contact_sums_i32", offsets, adj, n, n_adj, query, m)) return rc;
    if (m == 0) return TIP_OK;
    if (values)
        if (int rc = check_host_offsets("tip_contact_sums_i32", "value_offsets", value_offsets, m, values_cap)) return rc;
    Staging st;
    const int32_t *doff = st.in(offsets, (size_t)n + 1), *dadj = st.in(adj, (size_t)n_adj), *dq = st.in(query, (size_t)m);
    const uint8_t *dvalid = st.in(valid, (size_t)n), *dtype = st.in(type, (size_t)n);
    const int32_t *dp = st.in(pairs, (size_t)2 * n_triples);
    const int64_t *dc = st.in(counts, (size_t)n_triples), *dvoff = st.in(value_offsets, (size_t)m);
    int64_t *dsum = st.out(sums, (size_t)m), *dnsel = st.out(n_sel, (size_t)m), *dval = st.out(values, (size_t)values_cap, true);
    int32_t *dlab = st.out(value_labels, (size_t)values_cap, true);
    if (st.rc) return st.rc;
    if (int rc = contact_sums_launch(dp, dc, n_triples, doff, dadj, n, n_adj, dvalid, dtype, dq, m, mode, sel, dsum, dnsel, dvoff, dval, dlab,
                                     values_cap))
        return rc;
    return st.finish();
}

int tip_graph_neighbor_state_f64_dev(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *member,
                                     const double *state, const int32_t *query, int64_t m, double *nb_sum, int64_t *nb_cnt)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_state_args("tip_graph_neighbor_state_f64_dev", offsets, adj, n, n_adj, member, state, m, nb_sum, nb_cnt)) return rc;
    return neighbor_state_launch(offsets, adj, n, n_adj, member, state, query, m, nb_sum, nb_cnt);
}

int tip_graph_neighbor_state_f64(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *member, const double *state,
                                 const int32_t *query, int64_t m, double *nb_sum, int64_t *nb_cnt)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_state_args("tip_graph_neighbor_state_f64", offsets, adj, n, n_adj, member, state, m, nb_sum, nb_cnt)) return rc;
    if (int rc = check_host_graph("tip_graph_neighbor_state_f64", offsets, adj, n, n_adj, query, m)) return rc;   // (rows in any order)
    if (m == 0) return TIP_OK;
    Staging st;
    const int32_t *doff = st.in(offsets, (size_t)n + 1), *dadj = st.in(adj, (size_t)n_adj), *dq = st.in(query, (size_t)m);
    const uint8_t *dmember = st.in(member, (size_t)n);
    const double *dstate = st.in(state, (size_t)n);
    double *dsum = st.out(nb_sum, (size_t)m);
    int64_t *dcnt = st.out(nb_cnt, (size_t)m);
    if (st.rc) return st.rc;
    if (int rc = neighbor_state_launch(doff, dadj, n, n_adj, dmember, dstate, dq, m, dsum, dcnt)) return rc;
    return st.finish();
}

}  // extern "C"
