// tip_ws_binary.hip -- mode B of the watershed (tip_watershed.hip picks it): the exact flood of a two-valued image.
#include "tip_ws.h"
#include "tip_uf.h"
#include <algorithm>

namespace tip {

// ---- mode B: two-valued image (pl.py:194 floods a {0, 255} boundary image) --------------------------------------------
// Every low-valued pixel is a marker with the same heap key, and every other pixel has the same value, so the serial
// flood is (a) the markers popping in the order the array heap's mechanics give equal keys -- tip_heaporder.hip -- and
// (b) a FIFO: entries of the single remaining level pop in push order.  Push order = (pop rank of the pusher, neighbour
// slot up / left / right / down), so the flood is a breadth-first search in generations whose pixels carry a dense RANK:
// generation g+1's ranks come from sorting (rank of the gen-g pusher) * 4 + slot, done with a flag scatter + scan over
// the 4 n_g possible keys.  When a pixel pops it becomes a line iff the neighbours labelled before it (earlier
// generations, or the same generation with a smaller rank) carry two different labels, else it takes its pusher's label.
//   st[p]   low 32: label / 0 undecided / LINE;  high 32: rank + 1 of a marker or of a candidate (0: not reached yet)
//   cand[p] min over pushes of (key << 32 | pusher's label); ~0: never pushed
constexpr unsigned long long MB_NONE = ~0ULL;

__global__ void __launch_bounds__(256) k_mb_marker_flags(const unsigned long long *__restrict__ st, int *__restrict__ isroot, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) isroot[i] = st_lab(st[i]) > 0 ? 1 : 0;
}

// c[raster rank of the marker pixel] = number of its 4-neighbours inside the image that are not markers
__global__ void __launch_bounds__(256) k_mb_push_counts(const unsigned long long *__restrict__ st, const int *__restrict__ mrank,
                                                        unsigned char *__restrict__ c, int Y, int X)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= X) return;
    const int i = y * X + x;
    if (st_lab(st[i]) <= 0) return;
    int k = 0;
    if (y > 0 && st_lab(st[i - X]) == 0) ++k;
    if (x > 0 && st_lab(st[i - 1]) == 0) ++k;
    if (x < X - 1 && st_lab(st[i + 1]) == 0) ++k;
    if (y < Y - 1 && st_lab(st[i + X]) == 0) ++k;
    c[mrank[i]] = (unsigned char)k;
}

// E[order[t]] = t: pop rank of every marker from the pop sequence
__global__ void __launch_bounds__(256) k_mb_invert(const unsigned *__restrict__ order, unsigned *__restrict__ E, long M)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < M) E[order[t]] = (unsigned)t;
}

__global__ void __launch_bounds__(256) k_mb_init(unsigned long long *__restrict__ st, const int *__restrict__ mrank,
                                                 const unsigned *__restrict__ E, unsigned long long *__restrict__ cand, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int l = st_lab(st[i]);
    st[i] = l > 0 ? pack_st(l, (int)(E[mrank[i]] + 1u)) : 0ULL;
    cand[i] = MB_NONE;
}

// Block-aggregated append: the items of a 256-thread block are collected in LDS and the block reserves its slice of
// the global list with ONE atomic (hundreds of thousands of same-address atomics on the list counter serialise in L2:
// one per lane cost 1.9 ms per frame, one per block costs nothing measurable).
struct BlockList {
    int *items;     // LDS, capacity 4 * 256
    int *count;     // LDS
    int *base;      // LDS
};
__device__ __forceinline__ void bl_init(const BlockList &b)
{
    if (threadIdx.x == 0) *b.count = 0;
    __syncthreads();
}
__device__ __forceinline__ void bl_push(const BlockList &b, int value) { b.items[atomicAdd(b.count, 1)] = value; }
__device__ __forceinline__ void bl_flush(const BlockList &b, int *__restrict__ list, int *__restrict__ counter)
{
    __syncthreads();
    const int n = *b.count;
    if (n == 0) return;
    if (threadIdx.x == 0) *b.base = atomicAdd(counter, n);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) list[*b.base + i] = b.items[i];
}

// a labelled pixel p of rank r pushes its undecided neighbours: key = r * 4 + slot, slot = position of the neighbour in
// skimage's push order (up, left, right, down).  The first push of a pixel appends it to the next generation's list.
__device__ __forceinline__ void mb_push_from(unsigned long long *__restrict__ st, unsigned long long *__restrict__ cand,
                                             const BlockList &bl, int p, int Y, int X)
{
    const unsigned long long s = st[p];
    const int l = st_lab(s);
    if (l <= 0) return;
    const unsigned long long r4 = (unsigned long long)(unsigned)(st_tref(s) - 1) * 4ULL;
    const int y = p / X, x = p - y * X;
    const int nb[4] = {y > 0 ? p - X : -1, x > 0 ? p - 1 : -1, x < X - 1 ? p + 1 : -1, y < Y - 1 ? p + X : -1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int u = nb[k];
        if (u < 0 || st[u] != 0ULL) continue;
        const unsigned long long val = ((r4 + (unsigned long long)k) << 32) | (unsigned)l;
        if (atomicMin(&cand[u], val) == MB_NONE) bl_push(bl, u);
    }
}

__global__ void __launch_bounds__(256) k_mb_push_markers(unsigned long long *__restrict__ st, unsigned long long *__restrict__ cand,
                                                         int *__restrict__ next, int *__restrict__ counter, int Y, int X)
{
    __shared__ int s_items[4 * 256], s_count, s_base;
    const BlockList bl{s_items, &s_count, &s_base};
    bl_init(bl);
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x < X) mb_push_from(st, cand, bl, y * X + x, Y, X);
    bl_flush(bl, next, counter);
}

// fate of one pixel of the generation (rank r): true when decided.  When the pixel pops, the neighbours labelled before it
// are those of earlier generations plus the same-generation neighbours of smaller rank that took a label.  A pending
// same-generation neighbour q of smaller rank will end as a line (ignored) or with its pusher's label, which is already
// known (cand[q]): if that label equals the one label this pixel sees, q cannot change the outcome and is not waited for --
// a pixel only waits for smaller-ranked neighbours that would bring a DIFFERENT label, i.e. across a collision front, where
// the chains are two pixels long instead of running along the whole front.
// COH: every load / store goes to the L2 (agent scope), for the one-workgroup kernel that runs whole generations back to back: a cache
// line it read in an earlier generation may be stale in the CU's vector cache once atomics have changed it in the L2.
__device__ __forceinline__ unsigned long long mb_ld(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int mb_ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mb_st(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mb_st(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool COH = false>
__device__ __forceinline__ bool mb_try_resolve(unsigned long long *st, const unsigned long long *cand, int p, int myr, int Y, int X)
{
    volatile unsigned long long *vst = st;
    const int y = p / X, x = p - y * X;
    const int nb[4] = {y > 0 ? p - X : -1, x > 0 ? p - 1 : -1, x < X - 1 ? p + 1 : -1, y < Y - 1 ? p + X : -1};
    int l0 = 0;
    bool diff = false;
    unsigned wait_mask = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (nb[k] < 0) continue;
        const unsigned long long s = COH ? mb_ld(st + nb[k]) : vst[nb[k]];
        const int l = st_lab(s);
        if (l > 0) {
            if (l0 == 0) l0 = l;
            else if (l != l0) diff = true;
        } else if (l == 0) {
            const int r = st_tref(s);
            if (r != 0 && r < myr) wait_mask |= 1u << k;
        }
    }
    if (!diff && wait_mask) {       // (two labels already: a line whatever the pending neighbours become)
        bool pending = false;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((wait_mask >> k) & 1u) pending |= (int)(unsigned)((COH ? mb_ld(cand + nb[k]) : cand[nb[k]]) & 0xffffffffULL) != l0;
        if (pending) return false;
    }
    const unsigned long long out = pack_st(diff ? LINE_LAB : (int)(unsigned)((COH ? mb_ld(cand + p) : cand[p]) & 0xffffffffULL), myr);
    if (COH) mb_st(st + p, out); else vst[p] = out;
    return true;
}

// ---- the generation loop without a host round trip per generation ------------------------------------------------------------------
// The sizes of a generation live on the device (MbState); every kernel reads them there and walks its list with a grid-stride loop,
// so the host queues several generations' launches back to back and looks at the state once per batch (13 generations on a U-Net
// tail frame: two looks instead of thirteen synchronisations).  A generation after the last one is a handful of empty launches.
struct MbState {
    int ncur;        // pixels of the generation that pushes (its ranked list); generation 0: the markers push
    int nnext;       // pixels pushed so far by this generation (append counter of the unordered list)
    int keyspace;    // rank keys of the generation being ranked: 4 x ncur (generation 0: 4 x markers)
    int gen;         // generations completed
    int pcount[4];   // waiting-list counters of the resolve passes
    int flip;        // which of the two ranked-list buffers holds the generation that pushes (0: listA)
    int small_gens;  // generations finished by the one-workgroup kernel (diagnostic)
    int gsize[30];   // pixels of generation 1, 2, ... (diagnostic, TIP_WS_DEBUG)
};

__global__ void k_mb_state_init(MbState *S, int keyspace0)
{
    S->ncur = 0; S->nnext = 0; S->keyspace = keyspace0; S->gen = 0; S->flip = 0; S->small_gens = 0;
    for (int q = 0; q < 4; ++q) S->pcount[q] = 0;
    for (int q = 0; q < 30; ++q) S->gsize[q] = 0;
}

__global__ void __launch_bounds__(256) k_mb_push_list_dn(unsigned long long *__restrict__ st, unsigned long long *__restrict__ cand,
                                                         const int *__restrict__ listA, const int *__restrict__ listB, MbState *S,
                                                         int *__restrict__ next, int Y, int X)
{
    __shared__ int s_items[4 * 256], s_count, s_base;
    const BlockList bl{s_items, &s_count, &s_base};
    const int nlist = S->ncur;
    const int *__restrict__ list = S->flip ? listB : listA;
    for (int j0 = blockIdx.x * blockDim.x; j0 < nlist; j0 += gridDim.x * blockDim.x) {      // (block-uniform trip count: barriers inside)
        bl_init(bl);
        const int i = j0 + threadIdx.x;
        if (i < nlist) mb_push_from(st, cand, bl, list[i], Y, X);
        bl_flush(bl, next, &S->nnext);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_mb_flag_keys_dn(const unsigned long long *__restrict__ cand, const int *__restrict__ next,
                                                         const MbState *S, int *__restrict__ flag)
{
    const int nnext = S->nnext;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nnext; i += gridDim.x * blockDim.x) flag[(unsigned)(cand[next[i]] >> 32)] = 1;
}

// exclusive scan of the key flags, length on the device: a fixed grid walks the 2048-element chunks; a block first needs the sum of all
// chunks in front of its own, which it accumulates as it goes (its chunks are gridDim.x apart)
constexpr int MBS_ITEMS = SCAN_ITEMS, MBS_CHUNK = SCAN_BLOCK;      // (the tile of scan_tile_i32, tip_wave.h)
__global__ void __launch_bounds__(SCAN_THREADS) k_mb_scan_chunks(const int *__restrict__ in, int *__restrict__ out, const MbState *S, int *__restrict__ csum)
{
    __shared__ int wsum[SCAN_THREADS / 64];
    const int n = S->nnext > 0 ? S->keyspace : 0;
    for (int c0 = blockIdx.x; (long)c0 * MBS_CHUNK < n; c0 += gridDim.x) {
        const int total = scan_tile_i32(in, out, (long)c0 * MBS_CHUNK + (long)threadIdx.x * MBS_ITEMS, n, wsum);
        if (threadIdx.x == 0) csum[c0] = total;
        __syncthreads();                            // (the next chunk writes wsum)
    }
}
__global__ void __launch_bounds__(256) k_mb_scan_add(int *__restrict__ out, const MbState *S, const int *__restrict__ csum)
{
    __shared__ int wsum[4];
    const int n = S->nnext > 0 ? S->keyspace : 0;
    int off = 0, done_to = 0;                    // sum of csum[0 .. done_to)
    for (int c0 = blockIdx.x; (long)c0 * MBS_CHUNK < n; c0 += gridDim.x) {
        int part = 0;
        for (int j = done_to + threadIdx.x; j < c0; j += 256) part += csum[j];
        off += block_sum<4>(part, wsum);
        done_to = c0;
        const long base = (long)c0 * MBS_CHUNK + (long)threadIdx.x * MBS_ITEMS;
#pragma unroll
        for (int i = 0; i < MBS_ITEMS; ++i)
            if (base + i < n) out[base + i] += off;
        __syncthreads();
    }
}

// ranks of the generation; the key flags of the NEXT generation's key space (4 x this generation's pixels) are cleared on the way
__global__ void __launch_bounds__(256) k_mb_assign_ranks_dn(unsigned long long *__restrict__ st, const unsigned long long *__restrict__ cand,
                                                            const int *__restrict__ next, const MbState *S, const int *__restrict__ drank,
                                                            int *__restrict__ listA, int *__restrict__ listB, int *__restrict__ kflag_next)
{
    const int nnext = S->nnext;
    int *__restrict__ list = S->flip ? listA : listB;        // the generation being ranked goes to the OTHER buffer
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nnext; i += gridDim.x * blockDim.x) {
        const int u = next[i];
        const int r = drank[(unsigned)(cand[u] >> 32)];
        st[u] = pack_st(0, r + 1);
        list[r] = u;
    }
    const long nk = 4L * nnext;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += (long)gridDim.x * blockDim.x) kflag_next[i] = 0;
}

// resolve pass p (0: the whole generation; else the waiting list of pass p - 1), device counts, grid-stride
__global__ void __launch_bounds__(256) k_mb_resolve_dn(unsigned long long *__restrict__ st, const unsigned long long *__restrict__ cand,
                                                       const int *__restrict__ listA, const int *__restrict__ listB, MbState *S, int pass,
                                                       const int *__restrict__ src, int Y, int X, int *__restrict__ pend)
{
    __shared__ int s_items[4 * 256], s_count, s_base;
    const BlockList bl{s_items, &s_count, &s_base};
    const int n = pass == 0 ? S->nnext : S->pcount[pass - 1];
    const int *__restrict__ list = S->flip ? listA : listB;
    for (int j0 = blockIdx.x * blockDim.x; j0 < n; j0 += gridDim.x * blockDim.x) {
        bl_init(bl);
        const int j = j0 + threadIdx.x;
        if (j < n) {
            const int i = pass == 0 ? j : src[j];
            const int p = list[i];
            bool waiting = true;
            for (int attempt = 0; attempt < 2 && waiting; ++attempt) waiting = !mb_try_resolve(st, cand, p, i + 1, Y, X);
            if (waiting) bl_push(bl, i);
        }
        bl_flush(bl, pend, &S->pcount[pass]);
        __syncthreads();
    }
}

// the one-block tail of a generation, then the state moves on to the next generation
constexpr int MBT_THREADS = 256;
__global__ void __launch_bounds__(MBT_THREADS) k_mb_resolve_tail_dn(unsigned long long *__restrict__ st, const unsigned long long *__restrict__ cand,
                                                             const int *__restrict__ listA, const int *__restrict__ listB,
                                                             const int *__restrict__ pend, MbState *S, int last_pass, int Y, int X, WsInfo *info)
{
    const int n = S->pcount[last_pass];
    const int *__restrict__ list = S->flip ? listA : listB;
    volatile unsigned long long *vst = st;
    int left = n;
    for (int sweep = 0; sweep <= n && left > 0; ++sweep) {
        int mine = 0;
        for (int j = threadIdx.x; j < n; j += MBT_THREADS) {
            const int i = pend[j], p = list[i];
            if (st_lab(vst[p]) != 0) continue;
            if (!mb_try_resolve(st, cand, p, i + 1, Y, X)) mine = 1;
        }
        __threadfence_block();
        left = __syncthreads_count(mine);
    }
    if (threadIdx.x == 0) {
        if (left) info->unfinished = 1;       // only if the generation is inconsistent (never seen)
        const int nn = S->nnext;
        S->ncur = nn;
        S->keyspace = 4 * nn;
        S->nnext = 0;
        if (nn > 0 && S->gen < 30) S->gsize[S->gen] = nn;
        S->gen += nn > 0 ? 1 : 0;
        S->flip ^= 1;
        for (int q = 0; q < 4; ++q) S->pcount[q] = 0;
    }
}

// Small generations, as many as follow each other, in ONE workgroup: the late generations of a frame are a few hundred to a few thousand
// pixels (the flood's fronts meeting inside the boundary bands), and a generation of the grid-wide path is nine launches whatever its size.
// Here a generation is: push (append counter in LDS), the key flags as BITS in LDS (4 x ncur of them), ranks from a scan of the words'
// population counts, the ranked list, and resolve sweeps until nothing waits -- barriers instead of launches.  The kernel leaves as soon
// as a generation is larger than `small` again (state and key flags as the grid-wide kernels expect them), or when the flood is over.
constexpr int MB_SMALL_DEFAULT = 8192, MB_BATCH_DEFAULT = 4;
// 256 threads and 8 KB of LDS, like every kernel of this flood: a workgroup of that size (<= 64 registers a lane) finds room on a CU
// BESIDE the two waves per SIMD of another frame's convolution kernel (220 registers each of 512); the 1024-thread workgroups these
// two kernels had first waited for a convolution workgroup to retire -- 0.2 ms per launch, 5 ms of latency per frame in the kernel
// trace of the headline.  (Latency only: an A/B on one box shows the same frames/s either way, the frame's worker thread has that slack.)
constexpr int MBG_THREADS = 256, MBG_WORDS = 1024;            // key bits: 4 x ncur <= 32 x MBG_WORDS
constexpr int MB_SMALL_MAX = MBG_WORDS * 32 / 4;
__global__ void __launch_bounds__(MBG_THREADS) k_mb_small_gens(unsigned long long *st, unsigned long long *cand, int *listA, int *listB,
                                                               int *unordered, MbState *S, int small, int *kflag, int Y, int X, WsInfo *info)
{
    __shared__ unsigned bits[MBG_WORDS];
    __shared__ int pre[MBG_WORDS];
    __shared__ int wsum[MBG_THREADS / 64];
    __shared__ int s_nnext;
    int ncur = S->ncur, flip = S->flip, gen = S->gen;
    if (ncur <= 0 || ncur > small) return;                    // (uniform)
    const int t = threadIdx.x;
    int unfinished = 0, done = 0;
    for (;;) {
        int *cur = flip ? listB : listA, *nxt = flip ? listA : listB;
        const int nwords = (4 * ncur + 31) >> 5;
        for (int w = t; w < nwords; w += MBG_THREADS) bits[w] = 0u;
        if (t == 0) s_nnext = 0;
        __syncthreads();
        // push: key = rank of the pusher * 4 + slot (up, left, right, down); the first push of a pixel appends it
        for (int i = t; i < ncur; i += MBG_THREADS) {
            const int p = mb_ld(cur + i);
            const unsigned long long sp = mb_ld(st + p);
            const int l = st_lab(sp);
            if (l <= 0) continue;
            const unsigned long long r4 = (unsigned long long)(unsigned)(st_tref(sp) - 1) * 4ULL;
            const int y = p / X, x = p - y * X;
            const int nb[4] = {y > 0 ? p - X : -1, x > 0 ? p - 1 : -1, x < X - 1 ? p + 1 : -1, y < Y - 1 ? p + X : -1};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int u = nb[k];
                if (u < 0 || mb_ld(st + u) != 0ULL) continue;
                const unsigned long long val = ((r4 + (unsigned long long)k) << 32) | (unsigned)l;
                if (atomicMin(&cand[u], val) == MB_NONE) mb_st(unordered + atomicAdd(&s_nnext, 1), u);
            }
        }
        __threadfence();
        __syncthreads();
        const int nnext = s_nnext;
        if (nnext > 0) {
            for (int i = t; i < nnext; i += MBG_THREADS) {
                const unsigned key = (unsigned)(mb_ld(cand + mb_ld(unordered + i)) >> 32);
                atomicOr(&bits[key >> 5], 1u << (key & 31u));
            }
            __syncthreads();
            int carry = 0;
            for (int base = 0; base < nwords; base += MBG_THREADS) {
                const int w = base + t;
                const int c = w < nwords ? __popc(bits[w]) : 0;
                int total;
                const int before = block_exclusive_scan<MBG_THREADS / 64>(c, wsum, total);
                if (w < nwords) pre[w] = carry + before;
                carry += total;
                __syncthreads();
            }
            for (int i = t; i < nnext; i += MBG_THREADS) {
                const int u = mb_ld(unordered + i);
                const unsigned key = (unsigned)(mb_ld(cand + u) >> 32);
                const int r = pre[key >> 5] + __popc(bits[key >> 5] & ((1u << (key & 31u)) - 1u));
                mb_st(st + u, pack_st(0, r + 1));
                mb_st(nxt + r, u);
            }
            __threadfence();
            __syncthreads();
            int left = nnext;
            for (int sweep = 0; sweep <= nnext && left > 0; ++sweep) {
                int mine = 0;
                for (int i = t; i < nnext; i += MBG_THREADS) {
                    const int p = mb_ld(nxt + i);
                    if (st_lab(mb_ld(st + p)) != 0) continue;
                    if (!mb_try_resolve<true>(st, cand, p, i + 1, Y, X)) mine = 1;
                }
                __threadfence();
                left = __syncthreads_count(mine);
            }
            if (left) unfinished = 1;
            if (t == 0 && gen < 30) S->gsize[gen] = nnext;
            ++gen;
            ++done;
        }
        flip ^= 1;
        ncur = nnext;
        if (ncur == 0 || ncur > small) break;
    }
    for (int i = t; i < 4 * ncur; i += MBG_THREADS) kflag[i] = 0;       // the grid-wide path ranks the next generation: its key flags start clean
    if (t == 0) {
        if (unfinished) info->unfinished = 1;
        S->ncur = ncur; S->keyspace = 4 * ncur; S->nnext = 0; S->gen = gen; S->flip = flip; S->small_gens += done;
        for (int q = 0; q < 4; ++q) S->pcount[q] = 0;
    }
}

// The markers of the marker stage (st: label, or 0) flooded in generations; labels in st
int flood_two_valued(WsScratch &w, int Y, int X)
{
    hipStream_t s = ctx().stream;
    const Tuning &tune = tuning();
    const long n = (long)Y * X;
    WsInfo *info = w.info;
    unsigned long long *st = w.st;
    int rc;
    // (a) pop order of the equal-keyed markers: per-marker push counts -> host recurrence (tip_heaporder.hip) -> ranks
    int *mrank = w.rank, *total_d = &info->n_markers;    // (n_markers was copied out by the marker stage; reused as the scan's total)
    TIP_LAUNCH("mb_marker_flags", k_mb_marker_flags, dim3(cdiv(n, 256)), dim3(256), 0, (const unsigned long long *)st, w.isroot, n);
    if ((rc = exclusive_scan_i32(w.isroot, mrank, n, total_d))) return rc;
    int M = 0;
    TIP_HIP(hipMemcpyAsync(&M, total_d, sizeof(int), hipMemcpyDeviceToHost, s));
    TIP_HIP(hipStreamSynchronize(s));
    unsigned char *c_d = w.ws.get<unsigned char>((size_t)M);
    unsigned *E_d = w.ws.get<unsigned>((size_t)M), *order_d = w.ws.get<unsigned>((size_t)M);
    unsigned long long *cand = w.ws.get<unsigned long long>(n);
    int *lists = w.ws.get<int>((size_t)2 * n);
    int *pendA = w.isroot, *pendB = w.flag;   // waiting lists of the resolve passes (isroot / flag are free here)
    // rank keys of a generation live in [0, 4 * size of the previous one): the markers first, later at most every
    // other pixel
    const size_t keycap = (size_t)4 * (size_t)std::max<long>(M, n - M) + 4;
    int *kflag = w.ws.get<int>(keycap), *drank = w.ws.get<int>(keycap);
    if (!c_d || !E_d || !order_d || !cand || !lists || !kflag || !drank) return TIP_ERR_NOMEM;
    TIP_LAUNCH("mb_push_counts", k_mb_push_counts, dim3(cdiv(X, 256), Y), dim3(256), 0, (const unsigned long long *)st,
               (const int *)mrank, c_d, Y, X);
    {
        // counts down, pop sequence up, through this thread's pinned staging buffer (asynchronous copies, no per-frame allocation)
        const size_t order_off = ((size_t)M + 63) & ~(size_t)63;
        unsigned char *pin = (unsigned char *)pinned_scratch(order_off + (size_t)M * 4);
        if (!pin) return TIP_ERR_NOMEM;
        uint32_t *horder = reinterpret_cast<uint32_t *>(pin + order_off);
        TIP_HIP(hipMemcpyAsync(pin, c_d, (size_t)M, hipMemcpyDeviceToHost, s));
        TIP_HIP(hipStreamSynchronize(s));
        if ((rc = marker_pop_order(pin, M, horder))) return rc;
        TIP_HIP(hipMemcpyAsync(order_d, horder, (size_t)M * 4, hipMemcpyHostToDevice, s));      // (the buffer is next touched after this frame's later synchronisations)
    }
    TIP_LAUNCH("mb_invert", k_mb_invert, dim3(cdiv(M, 256)), dim3(256), 0, (const unsigned *)order_d, E_d, (long)M);
    TIP_LAUNCH("mb_init", k_mb_init, dim3(cdiv(n, 256)), dim3(256), 0, st, (const int *)mrank, (const unsigned *)E_d, cand, n);
    // (b) generations: sizes on the device (MbState), launches queued MB_BATCH generations at a time, one look at the state per batch
    int *unordered = w.parent;                          // append buffer of a generation before it is ranked (parent is free here)
    MbState *S = w.ws.get<MbState>(1);
    const long nm = n - M;                              // non-marker pixels: the most a generation (and all of them together) can hold
    const long keycap_later = 4L * nm + 4;
    int *csum = w.ws.get<int>((size_t)(std::max<long>(4L * M, keycap_later) / MBS_CHUNK + 2));
    if (!S || !csum) return TIP_ERR_NOMEM;
    TIP_LAUNCH("mb_state_init", k_mb_state_init, dim3(1), dim3(1), 0, S, (int)std::min<long>(4L * M, 0x7fffffffL));
    TIP_HIP(hipMemsetAsync(kflag, 0, (size_t)(4L * M) * sizeof(int), s));
    constexpr int MB_PASSES = 2;                        // (pixels wait only across collision fronts: the second pass is already nearly empty, the tail takes what it leaves)
    const int mb_small = tune.mb_small < 0 ? MB_SMALL_DEFAULT : std::min(tune.mb_small, MB_SMALL_MAX);
    const int mb_batch = tune.mb_batch > 0 ? std::min(tune.mb_batch, 64) : MB_BATCH_DEFAULT;
    const int lgrid = (int)std::max<long>(1, std::min<long>(cdiv(nm, 256), 1024));      // fixed grids, grid-stride loops over device counts
    int *listA = lists, *listB = lists + n;             // ranked lists of the pushing / the pushed generation; MbState::flip says which is which
    MbState hS;
    WsInfo h;
    for (int gen = 0;;) {
        for (int b = 0; b < mb_batch; ++b, ++gen) {
            if (gen == 0)
                TIP_LAUNCH("mb_push_markers", k_mb_push_markers, dim3(cdiv(X, 256), Y), dim3(256), 0, st, cand, unordered, &S->nnext, Y, X);
            else
                TIP_LAUNCH("mb_push_list", k_mb_push_list_dn, dim3(lgrid), dim3(256), 0, st, cand, (const int *)listA, (const int *)listB, S,
                           unordered, Y, X);
            TIP_LAUNCH("mb_flag_keys", k_mb_flag_keys_dn, dim3(lgrid), dim3(256), 0, (const unsigned long long *)cand, (const int *)unordered,
                       (const MbState *)S, kflag);
            const long keys = gen == 0 ? 4L * M : keycap_later;
            const int sgrid = (int)std::max<long>(1, std::min<long>(cdiv(keys, MBS_CHUNK), 1024));
            TIP_LAUNCH("mb_scan_chunks", k_mb_scan_chunks, dim3(sgrid), dim3(256), 0, (const int *)kflag, drank, (const MbState *)S, csum);
            TIP_LAUNCH("mb_scan_add", k_mb_scan_add, dim3(sgrid), dim3(256), 0, drank, (const MbState *)S, (const int *)csum);
            TIP_LAUNCH("mb_assign_ranks", k_mb_assign_ranks_dn, dim3(lgrid), dim3(256), 0, st, (const unsigned long long *)cand,
                       (const int *)unordered, (const MbState *)S, (const int *)drank, listA, listB, kflag);
            // fate of the generation: parallel passes that ping-pong the list of waiting pixels, then the one-block tail, which
            // also moves the state on to the next generation
            for (int pass = 0; pass < MB_PASSES; ++pass) {
                int *dst = pass & 1 ? pendB : pendA;
                const int *src = pass == 0 ? nullptr : (pass & 1 ? pendA : pendB);
                TIP_LAUNCH("mb_resolve", k_mb_resolve_dn, dim3(pass == 0 ? lgrid : std::max(1, lgrid >> (2 * pass))), dim3(256), 0, st,
                           (const unsigned long long *)cand, (const int *)listA, (const int *)listB, S, pass, src, Y, X, dst);
            }
            TIP_LAUNCH("mb_resolve_tail", k_mb_resolve_tail_dn, dim3(1), dim3(MBT_THREADS), 0, st, (const unsigned long long *)cand,
                       (const int *)listA, (const int *)listB, (const int *)((MB_PASSES - 1) & 1 ? pendB : pendA), S, MB_PASSES - 1, Y, X, info);
            // whatever small generations follow (usually all that are left) run in one workgroup
            if (mb_small > 0)
                TIP_LAUNCH("mb_small_gens", k_mb_small_gens, dim3(1), dim3(MBG_THREADS), 0, st, cand, listA, listB, unordered, S, mb_small, kflag, Y, X, info);
        }
        TIP_HIP(hipMemcpyAsync(&hS, S, sizeof hS, hipMemcpyDeviceToHost, s));
        TIP_HIP(hipMemcpyAsync(&h, info, sizeof h, hipMemcpyDeviceToHost, s));      // (the same look: did every generation resolve?)
        TIP_HIP(hipStreamSynchronize(s));
        if (hS.ncur == 0) break;                        // the last generation pushed nothing: the flood is complete
        if (gen > 4 * (Y + X) + 64) return fail(TIP_ERR_HIP, "watershed: the two-valued flood does not terminate");
    }
    if (tune.ws_debug) {
        fprintf(stderr, "[tip] two-valued flood: %d generations (%d in the one-workgroup kernel), sizes", hS.gen, hS.small_gens);
        for (int q = 0; q < 30 && q < hS.gen; ++q) fprintf(stderr, " %d", hS.gsize[q]);
        fprintf(stderr, "\n");
    }
    if (h.unfinished != 0) return fail(TIP_ERR_HIP, "watershed: a generation of the two-valued flood did not resolve");
    return TIP_OK;
}

}  // namespace tip
