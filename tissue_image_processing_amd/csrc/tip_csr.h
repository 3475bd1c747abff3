// tip_csr.h -- the CSR pieces shared by the neighbour-graph features (tip_graph.hip) and the Delaunay rows (tip_order.hip):
// offsets int32[n + 1], adj int32[n_adj] of 1-based labels.  Device side: the label test, the clamped row read, the search in an
// ascending row, the rank of an entry among its row (row_rank: also how the track linker, tip_link.hip, orders a subnet's members in
// LDS) and the per-row rank sort.  Host side: the dimension check of both forms and the validation of a HOST CSR before it is
// uploaded.
#pragma once
#include "tip_internal.h"

namespace tip {

constexpr int CSR_WAVE = 64, CSR_BLOCK = 256, CSR_WPB = CSR_BLOCK / CSR_WAVE;

__device__ __forceinline__ bool label_ok(int l, int n) { return (unsigned)(l - 1) < (unsigned)n; }

// row r of the CSR, clamped to [0, n_adj]
__device__ __forceinline__ void row_of(const int32_t *__restrict__ offsets, int r, long n_adj, int &b, int &e)
{
    b = offsets[r];
    e = offsets[r + 1];
    if (b < 0) b = 0;
    if (e > n_adj) e = (int)n_adj;
    if (e < b) e = b;
}

// position of label k in the ascending row [b, e) of adj, or -1
__device__ __forceinline__ int row_find(const int32_t *__restrict__ adj, int b, int e, int k)
{
    while (b < e) {
        const int mid = b + ((e - b) >> 1), v = adj[mid];
        if (v == k) return mid;
        if (v < k) b = mid + 1;
        else e = mid;
    }
    return -1;
}

// the slot, counted from b, of entry a (of value v) of the row raw[b .. e) in ascending order: the number of entries below it,
// ties by position
template <typename Idx>
__device__ __forceinline__ Idx row_rank(const int32_t *raw, Idx b, Idx e, int v, Idx a)
{
    Idx rank = 0;
    for (Idx c = b; c < e; ++c) {
        const int w = raw[c];
        rank += (w < v || (w == v && c < a)) ? 1 : 0;
    }
    return rank;
}

// one wavefront per row: entry a of raw goes to the slot row_rank gives it, plus `add`.
// Lanes stride over the row in chunks of 64, so a hub row longer than a wavefront takes several chunks.  The row starts at
// offsets[row] and ends at offsets[row + 1], or row_len[row] entries later when row_len is given; a row that does not fit out
// (cap) or raw (raw_cap) is left out (the entry point reports the overflow).
template <typename OffT>
__global__ __launch_bounds__(CSR_BLOCK) void k_rank_sort(const OffT *__restrict__ offsets, const int32_t *__restrict__ row_len,
                                                         const int32_t *__restrict__ raw, long raw_cap, int32_t *__restrict__ out, int n,
                                                         long cap, int add)
{
    const int row = blockIdx.x * CSR_WPB + (threadIdx.x >> 6), lane = threadIdx.x & (CSR_WAVE - 1);
    if (row >= n) return;
    const long b = (long)offsets[row], e = row_len ? b + row_len[row] : (long)offsets[row + 1];
    if (b < 0 || e < b || e > cap || e > raw_cap) return;
    for (long a = b + lane; a < e; a += CSR_WAVE) {
        const int v = raw[a];
        out[b + row_rank(raw, b, e, v, a)] = v + add;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the dimensions and pointers of a CSR with m query rows, for the host and the device forms
inline int check_graph(const char *who, const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, int64_t m)
{
    if (n < 0 || n > 0x7ffffffe || m < 0) return fail(TIP_ERR_ARG, "%s: n = %ld rows, m = %ld queries", who, (long)n, (long)m);
    if (n_adj < 0 || n_adj > 0x7fffffff) return fail(TIP_ERR_ARG, "%s: n_adj = %ld", who, (long)n_adj);
    if (!offsets || (n_adj > 0 && !adj)) return fail(TIP_ERR_ARG, "%s: the CSR arrays (offsets, adj)", who);
    return TIP_OK;
}

// a HOST CSR and query list, before they are uploaded: monotone offsets that end at n_adj, labels in 1..n, queries below n
// (NULL: query q is row q, so m <= n)
inline int check_host_graph(const char *who, const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const int32_t *query,
                            int64_t m)
{
    if (offsets[0] != 0 || offsets[n] != n_adj) return fail(TIP_ERR_ARG, "%s: offsets run from %d to %d, adj has %ld entries", who, offsets[0], offsets[n], (long)n_adj);
    for (int64_t r = 0; r < n; ++r) {
        if (offsets[r + 1] < offsets[r]) return fail(TIP_ERR_ARG, "%s: offsets decrease at row %ld", who, (long)r);
        for (int a = offsets[r]; a < offsets[r + 1]; ++a)
            if (adj[a] < 1 || adj[a] > n) return fail(TIP_ERR_ARG, "%s: row %ld holds label %d (1..%ld)", who, (long)r, adj[a], (long)n);
    }
    if (!query && m > n) return fail(TIP_ERR_ARG, "%s: %ld queries of %ld rows", who, (long)m, (long)n);
    for (int64_t q = 0; query && q < m; ++q)
        if (query[q] < 0 || query[q] >= n) return fail(TIP_ERR_ARG, "%s: query %ld is row %d of %ld", who, (long)q, query[q], (long)n);
    return TIP_OK;
}

// ... and the rows ascending, for the entries that search a row (after check_host_graph: the offsets are sound)
inline int check_rows_ascend(const char *who, const int32_t *offsets, const int32_t *adj, int64_t n)
{
    for (int64_t r = 0; r < n; ++r)
        for (int a = offsets[r] + 1; a < offsets[r + 1]; ++a)
            if (adj[a] <= adj[a - 1]) return fail(TIP_ERR_ARG, "%s: row %ld is not ascending", who, (long)r);
    return TIP_OK;
}

}  // namespace tip
