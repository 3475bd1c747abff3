// tip_ws_tiles.hip -- mode A of the watershed (tip_watershed.hip picks it): certified tile rounds, the per-component
// endgame, the wide pass and the serial finish.
#include "tip_ws.h"
#include "tip_uf.h"
#include <algorithm>
#include <vector>

namespace tip {

// ---- mode A: tile-local rounds ------------------------------------------------------------------------------------------
// The rounds are latency bound: what counts is how many tiles a CU keeps in flight (LDS per tile).  Two launch flavours:
// the everyday one (16x16 interior, one wave, 3-pixel halo, pockets of up to 6 cells, 2-cell evaluated margin, event-driven
// work list; 10 KB of LDS: 16 tiles per CU) and, when a whole launch makes no progress, the wide one (12-pixel halo,
// 48-cell pockets: stuck pockets are thin staircases up to ~10 px long on smooth landscapes), tried before the serial
// finish (tip_ws_serial.hip).  Other flavours measured slower.
constexpr int WT_FAST = 16, WTH_FAST = 64, WH_FAST = 3, WK_FAST = 6, WM_FAST = 2, EV_FAST = 1;
constexpr int WT_WIDE = 32, WTH_WIDE = 256, WH_WIDE = 12, WK_WIDE = 48;
constexpr int WS_OPEN_A = 8, WS_OPEN_B = 6;   // the opening: tile launches before / after the early endgame
constexpr int WS_MAX_ROUNDS = 4096;     // rounds of one tile per launch
constexpr int WST_STUCK = 0x40000000;   // tile_wst: the tile's last run decided nothing (low bits: undecided cells left in its window)
// tile-local marker "undecided and already on the work list": label 0 with a non-zero reference field (never leaves LDS)
constexpr unsigned long long ST_LISTED = 1ULL << 32;

struct T2 { double v; int i; };
__device__ __forceinline__ bool t_lt(const T2 &a, const T2 &b) { return a.v < b.v || (a.v == b.v && a.i < b.i); }

// one window cell: value slot and packed state side by side, so the flood rule fetches a neighbour with ONE 16-byte LDS read
struct __attribute__((aligned(16))) WCell { double v; unsigned long long st; };

struct TileView {
    const WCell *cell;                 // LDS window.  .st: packed state (label | pop-time reference pixel << 32);
                                       // .v: undecided cell: its image value (= key value); labelled cell: its pop-time
                                       // VALUE (its own value, or the puller's pop-time value for a pulled pixel)
    unsigned short *vis;               // LDS: this thread's pocket list
    int budget;                        // pocket flood budget (cells)
    int WL;                            // window edge (tile + 2 * halo)
    int g00, X;                        // global linear index of window cell 0 (may be negative), image row length
};

// Is undecided cell q (key < t) certain not to be labelled before time t?  Flood the pocket of undecided cells with
// key < t around q (breadth first, the per-thread list in LDS is queue and visited set at once); the pocket is closed
// iff nothing labelled before t touches it.  Running out of budget or window is "cannot certify" (the pixel waits).
// Out of line to keep the everyday rule small -- so everything it needs travels BY VALUE in registers, with the LDS
// arrays as address-space-3 pointers: a TileView reference would live on the (global-memory) stack and every field
// access in the flood would be a scratch load (measured: a certificate round cost 400k cycles that way).
typedef __attribute__((address_space(3))) const WCell *lds_ccell;
typedef __attribute__((address_space(3))) unsigned short *lds_u16;

__device__ __forceinline__ bool ws_cert(lds_ccell cell, lds_u16 vis, int budget, int WL, int g00, int X, int q, int asker,
                                     double tvv, int tii)
{
    const T2 t{tvv, tii};
    int nv = 1, head = 0;
    vis[0] = (unsigned short)q;
    while (head < nv) {
        const int c = vis[head++];
        const int cy = c / WL, cx = c - cy * WL;
        if (cy == 0 || cy == WL - 1 || cx == 0 || cx == WL - 1) return false;  // neighbours outside the window
        const int gc = g00 + cy * X + cx;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const int m = k == 0 ? c - WL : (k == 1 ? c - 1 : (k == 2 ? c + 1 : c + WL));
            if (m == asker) continue;
            const int gm = k == 0 ? gc - X : (k == 1 ? gc - 1 : (k == 2 ? gc + 1 : gc + X));
            const double cmv = cell[m].v;
            const unsigned long long sm = cell[m].st;
            const int l = st_lab(sm);
            if (l == LINE_LAB) continue;
            if (l > 0) {
                if (t_lt(T2{cmv, st_tref(sm)}, t)) return false;
            } else if (t_lt(T2{cmv, gm}, t)) {
                bool seen = false;
                for (int j = 0; j < nv; ++j) seen |= vis[j] == (unsigned short)m;
                if (!seen) {
                    if (nv >= budget) return false;
                    vis[nv++] = (unsigned short)m;
                }
            }
        }
    }
    return true;
}

__device__ __forceinline__ bool ws_cert(const TileView &tv, int q, int asker, double tvv, int tii)
{
    return ws_cert((lds_ccell)tv.cell, (lds_u16)tv.vis, tv.budget, tv.WL, tv.g00, tv.X, q, asker, tvv, tii);
}

struct Decision { int lab; int ti; double tv; };  // lab == 0: no decision; (tv, ti) = pop time: value and reference pixel

// The flood rule for one undecided cell, written for few instructions: all LDS loads first, then predicated
// arithmetic; the pocket certificates (rare) are the only calls.  certs == false: any undecided neighbour that could
// pop earlier makes the pixel wait (the common case: that neighbour is simply not processed yet).
__device__ __forceinline__ Decision ws_decide(const TileView &tv, int c, int gc, bool certs)
{
    Decision d{0, 0, 0.0};
    const int WL = tv.WL;
    const int q0 = c - WL, q1 = c - 1, q2 = c + 1, q3 = c + WL;
    const WCell n0 = tv.cell[q0], n1 = tv.cell[q1], n2 = tv.cell[q2], n3 = tv.cell[q3];
    const unsigned long long s0 = n0.st, s1 = n1.st, s2 = n2.st, s3 = n3.st;
    const int l0 = st_lab(s0), l1 = st_lab(s1), l2 = st_lab(s2), l3 = st_lab(s3);
    // (no early-out for "no labelled neighbour": cells on the work list always have one, and the rule below yields
    // "no decision" anyway if they did not)
    const double v0 = n0.v, v1 = n1.v, v2 = n2.v, v3 = n3.v, vc = tv.cell[c].v;
    const int g0 = gc - tv.X, g1 = gc - 1, g2 = gc + 1, g3 = gc + tv.X;
    int s_lab = 0, pull_lab = 0, pull_ti = 0;
    bool conflict = false, has_pull = false;
    double pull_tv = 0.0;
    unsigned early_u = 0, und = 0;   // bit k: undecided neighbour k (that could pop before this cell)
    // straight-line, select-based evaluation of the four neighbours: this code runs with few active lanes and every
    // divergent branch costs scalar exec-mask bookkeeping -- the kernel is bound by scalar/branch issue, not by math
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long sq = k == 0 ? s0 : (k == 1 ? s1 : (k == 2 ? s2 : s3));
        const int l = k == 0 ? l0 : (k == 1 ? l1 : (k == 2 ? l2 : l3));
        const int gq = k == 0 ? g0 : (k == 1 ? g1 : (k == 2 ? g2 : g3));
        const double tq = k == 0 ? v0 : (k == 1 ? v1 : (k == 2 ? v2 : v3));   // a labelled cell's slot holds its pop-time value
        const bool lab = l > 0, undq = l == 0;
        const int ti = lab ? st_tref(sq) : gq;
        const bool before = tq < vc || (tq == vc && ti < gc);
        const bool first = lab & before;                       // labelled before this cell pops
        conflict |= first & (s_lab != 0) & (s_lab != l);
        s_lab = (first & (s_lab == 0)) ? l : s_lab;
        const bool later = lab & !before;                      // a possible puller
        const bool better = later & (!has_pull | (tq < pull_tv) | ((tq == pull_tv) & (ti < pull_ti)));
        has_pull |= later;
        pull_tv = better ? tq : pull_tv;
        pull_ti = better ? ti : pull_ti;
        pull_lab = better ? l : pull_lab;
        und |= undq ? (1u << k) : 0u;
        early_u |= (undq & before) ? (1u << k) : 0u;
    }
    if (!certs) {
        // the everyday round, branch-free: nothing is decided while an undecided neighbour could pop earlier
        unsigned blk = 0;   // undecided neighbours that could still be labelled before the pull
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double vq = k == 0 ? v0 : (k == 1 ? v1 : (k == 2 ? v2 : v3));
            const int gq = k == 0 ? g0 : (k == 1 ? g1 : (k == 2 ? g2 : g3));
            const bool after_pull = (pull_tv < vq) | ((pull_tv == vq) & (pull_ti < gq));
            blk |= ((((und >> k) & 1u) != 0u) & !after_pull) ? 1u : 0u;
        }
        const bool quiet = early_u == 0;
        const bool ok_normal = (s_lab != 0) & quiet;
        const bool ok_pull = (s_lab == 0) & has_pull & quiet & (blk == 0);
        d.lab = ok_normal ? (conflict ? LINE_LAB : s_lab) : (ok_pull ? pull_lab : 0);
        d.ti = ok_normal ? gc : pull_ti;
        d.tv = ok_normal ? vc : pull_tv;
        return d;
    }
    if (early_u) {
#pragma unroll 1
        for (int k = 0; k < 4; ++k)
            if ((early_u >> k) & 1u) {
                const int q = k == 0 ? q0 : (k == 1 ? q1 : (k == 2 ? q2 : q3));
                if (!ws_cert(tv, q, c, vc, gc)) return d;
            }
    }
    if (s_lab != 0) {
        d.lab = conflict ? LINE_LAB : s_lab;
        d.ti = gc; d.tv = vc;
        return d;
    }
    if (!has_pull) return d;
    // stuck pixel: it is pulled by its earliest-labelled neighbour unless another neighbour can still get there first
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        if (!((und >> k) & 1u)) continue;
        const int q = k == 0 ? q0 : (k == 1 ? q1 : (k == 2 ? q2 : q3));
        const double vq = k == 0 ? v0 : (k == 1 ? v1 : (k == 2 ? v2 : v3));
        const int gq = k == 0 ? g0 : (k == 1 ? g1 : (k == 2 ? g2 : g3));
        if (pull_tv < vq || (pull_tv == vq && pull_ti < gq)) continue;   // q cannot pop before the pull
        if (!certs) return d;
        if (!ws_cert(tv, q, c, pull_tv, pull_ti)) return d;
    }
    d.lab = pull_lab; d.ti = pull_ti; d.tv = pull_tv;
    return d;
}

// One block = one 32x32 tile (+ halo) iterated to its local fixed point.  Work list: only undecided cells that touch a
// labelled cell (the frontier) are evaluated each round; a cell that gets labelled wakes its undecided interior
// neighbours.  Cheap rule while the tile progresses, pocket certificates for one round when it stalls.
// WM > 0: the tile also evaluates a margin of WM cells around its interior (redundantly with its neighbours -- a certified
// decision is the same whoever takes it) and stores every decision straight to global memory: dependency chains that
// zig-zag across a tile border no longer cost one launch per crossing.
// EV = 1: event-driven work list.  A cell that has to wait LEAVES the list and comes back when one of its neighbours is
// decided (label or line) -- instead of being re-evaluated every round until its lower neighbours are through.
// first = 1 (a frame's first launch, the wide pass): every tile runs, whatever its neighbours' activity words say.
template <int WT, int WS_THREADS, int WH, int WK, int WM = 0, int EV = 0>
__global__ void __launch_bounds__(WS_THREADS) k_ws_tiles(const double *__restrict__ v, unsigned long long *__restrict__ st, int Y, int X,
                                                  int tilesX, int tilesY, const unsigned char *__restrict__ changed_prev,
                                                  unsigned char *__restrict__ changed_cur, int *__restrict__ tile_und,
                                                  int *__restrict__ tile_front, int *__restrict__ tile_wst, int first, int dbg, WsInfo *info)
{
    constexpr int WL = WT + 2 * WH;
    constexpr int WE = WT + 2 * WM, E0 = WH - WM, E1 = WL - E0;    // evaluated region: window rows / columns [E0, E1)
    static_assert(WM >= 0 && WM < WH, "the outermost window ring is read-only");
    __shared__ WCell cells[WL * WL];
    __shared__ unsigned short svis[WS_THREADS * WK];
    __shared__ unsigned short slist[2][WE * WE];
    __shared__ int s_n[2], s_any, s_und, s_chg, s_front;
    const int tile = blockIdx.x, ty = tile / tilesX, tx = tile % tilesX;
    // (every block writes its changed_cur word, also when it has nothing to do: no memset between launches)
    if (!first) {
        bool act = tile_und[tile] != 0;
        if (act) {
            act = false;
            for (int j = -1; j <= 1; ++j)
                for (int i = -1; i <= 1; ++i) {
                    const int yy = ty + j, xx = tx + i;
                    if (yy >= 0 && yy < tilesY && xx >= 0 && xx < tilesX) act |= changed_prev[yy * tilesX + xx] != 0;
                }
        }
        if (!act) { if (threadIdx.x == 0) changed_cur[tile] = 0; return; }
    }
    const int gy0 = ty * WT - WH, gx0 = tx * WT - WH;
    int wcount = 0;          // undecided cells in the window at load time
    {   // window load: all state loads of the thread in flight together, then all value loads (the value a labelled
        // cell needs is its pop-time value v[tref]); one wave per tile and few tiles per CU: nothing else hides latency
        constexpr int NLOAD = (WL * WL + WS_THREADS - 1) / WS_THREADS;
        unsigned long long ls[NLOAD];
        double lv[NLOAD];
        int lg[NLOAD];
#pragma unroll
        for (int u = 0; u < NLOAD; ++u) {
            const int c = threadIdx.x + u * WS_THREADS;
            const int ly = c / WL, lx = c - ly * WL;
            const int gy = gy0 + ly, gx = gx0 + lx;
            const bool in = c < WL * WL && gy >= 0 && gy < Y && gx >= 0 && gx < X;
            lg[u] = in ? gy * X + gx : -1;
            ls[u] = st[in ? lg[u] : 0];
            if (!in) ls[u] = pack_st(LINE_LAB, 0);
        }
        // A tile that decided nothing last time -- not even with pocket certificates, which cost ~40 plain rounds -- and is
        // woken by a neighbour's news can only get further if its OWN window has changed.  Decisions are final, so the
        // number of undecided cells in the window is an exact change detector: same count, same window, leave at once.
        if (WS_THREADS == 64 && tile_wst != nullptr) {
#pragma unroll
            for (int u = 0; u < NLOAD; ++u) wcount += st_lab(ls[u]) == 0 ? 1 : 0;
            for (int d = 32; d >= 1; d >>= 1) wcount += __shfl_xor(wcount, d, 64);   // (by hand: wave_sum changes this kernel's code)
            if (!first && tile_wst[tile] == (wcount | WST_STUCK)) {
                if (threadIdx.x == 0) changed_cur[tile] = 0;
                return;
            }
        }
#pragma unroll
        for (int u = 0; u < NLOAD; ++u) {
            const int src = lg[u] < 0 ? 0 : (st_lab(ls[u]) > 0 ? st_tref(ls[u]) : lg[u]);
            lv[u] = v[src];
        }
#pragma unroll
        for (int u = 0; u < NLOAD; ++u) {
            const int c = threadIdx.x + u * WS_THREADS;
            if (c < WL * WL) { cells[c].v = lv[u]; cells[c].st = ls[u]; }
        }
    }
    if (threadIdx.x == 0) { s_n[0] = 0; s_n[1] = 0; s_any = 0; s_und = 0; s_chg = 0; s_front = 0; }
    __syncthreads();
    const int g00 = gy0 * X + gx0;
    TileView tv{cells, svis + threadIdx.x * WK, WK, WL, g00, X};
    // initial frontier: undecided cells of the evaluated region next to a labelled cell
    unsigned was_und = 0;   // (WM == 0) bit k: own interior cell k was undecided when the window was loaded
    if (WM == 0) {
#pragma unroll
        for (int k = 0; k < WT * WT / WS_THREADS; ++k) {
            const int p = threadIdx.x + k * WS_THREADS;
            const int c = (p / WT + WH) * WL + (p % WT + WH);
            if (st_lab(cells[c].st) == 0) {
                was_und |= 1u << k;
                if (st_lab(cells[c - WL].st) > 0 || st_lab(cells[c - 1].st) > 0 || st_lab(cells[c + 1].st) > 0 || st_lab(cells[c + WL].st) > 0) {
                    cells[c].st = ST_LISTED;
                    slist[0][atomicAdd(&s_n[0], 1)] = (unsigned short)c;
                }
            }
        }
    } else {
        for (int p = threadIdx.x; p < WE * WE; p += WS_THREADS) {
            const int c = (p / WE + E0) * WL + (p % WE + E0);
            if (st_lab(cells[c].st) == 0 &&
                (st_lab(cells[c - WL].st) > 0 || st_lab(cells[c - 1].st) > 0 || st_lab(cells[c + 1].st) > 0 || st_lab(cells[c + WL].st) > 0)) {
                cells[c].st = ST_LISTED;      // (still label 0 for the threads that scan its neighbours)
                slist[0][atomicAdd(&s_n[0], 1)] = (unsigned short)c;
            }
        }
    }
    __syncthreads();
    int cur = 0, my_evals = 0, my_rounds = 0;
    bool certs = false;
    if (EV) {
        bool certs_done = false;
        for (int round = 0; round < WS_MAX_ROUNDS; ++round) {
            int n = s_n[cur];
            if (n == 0) {
                // the list ran dry.  A tile that got nowhere at all tries one round with pocket certificates on its frontier
                // (they cost ~40 plain rounds; a tile that moved is re-run next launch anyway, with its neighbours' news)
                if (certs_done || s_chg > 0) break;
                __syncthreads();
                for (int p = threadIdx.x; p < WE * WE; p += WS_THREADS) {
                    const int c = (p / WE + E0) * WL + (p % WE + E0);
                    if (cells[c].st == 0ULL &&
                        (st_lab(cells[c - WL].st) > 0 || st_lab(cells[c - 1].st) > 0 || st_lab(cells[c + 1].st) > 0 || st_lab(cells[c + WL].st) > 0)) {
                        cells[c].st = ST_LISTED;
                        slist[cur][atomicAdd(&s_n[cur], 1)] = (unsigned short)c;
                    }
                }
                __syncthreads();
                certs = true; certs_done = true;
                if (dbg && threadIdx.x == 0) atomicAdd(&info->dbg_certs, 1ULL);
                n = s_n[cur];
                if (n == 0) break;
            }
            my_rounds++;
            if (threadIdx.x == 0) s_n[cur ^ 1] = 0;
            __syncthreads();
#pragma unroll 1
            for (int base = 0; base < n; base += WS_THREADS) {
                const int i = base + threadIdx.x;
                int c = -1;
                Decision dec{0, 0, 0.0};
                if (i < n) {
                    c = slist[cur][i];         // (listed cells are undecided: a cell enters the list once per stay)
                    my_evals++;
                    dec = ws_decide(tv, c, g00 + (c / WL) * X + c % WL, certs);
                }
                __syncthreads();  // every read of this chunk is done
                if (c >= 0 && dec.lab == 0) cells[c].st = 0ULL;   // waits: off the list until a neighbour is decided
                __syncthreads();  // (the drops first: a neighbour decided in this very chunk must be able to wake the cell)
                if (c >= 0 && dec.lab != 0) {
                    cells[c].st = pack_st(dec.lab, dec.ti); cells[c].v = dec.tv;
                    if (WM > 0) st[g00 + (c / WL) * X + c % WL] = pack_st(dec.lab, dec.ti);   // (an undecided cell lies inside the image)
                    atomicAdd(&s_chg, 1);
                    const int cy = c / WL, cx = c - cy * WL;   // c is evaluated: a neighbour is too unless c is on that edge of the region
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int q = k == 0 ? c - WL : (k == 1 ? c - 1 : (k == 2 ? c + 1 : c + WL));
                        const bool inside = k == 0 ? cy > E0 : (k == 1 ? cx > E0 : (k == 2 ? cx < E1 - 1 : cy < E1 - 1));
                        if (inside && atomicCAS(&cells[q].st, 0ULL, ST_LISTED) == 0ULL)
                            slist[cur ^ 1][atomicAdd(&s_n[cur ^ 1], 1)] = (unsigned short)q;
                    }
                }
                __syncthreads();
            }
            cur ^= 1;
            certs = false;
        }
    } else {
        for (int round = 0; round < WS_MAX_ROUNDS; ++round) {
            const int n = s_n[cur];
            if (n == 0) break;
            my_rounds++;
            if (threadIdx.x == 0) { s_n[cur ^ 1] = 0; s_any = 0; }
            __syncthreads();
            // The list is worked off in chunks of one entry per thread, each chunk committed before the next is evaluated
            // (decisions are certified on the states they read, so committing earlier is just a finer round).  One inlined
            // copy of the flood rule instead of four keeps the kernel small -- it is branchy scalar-heavy code and used to
            // overflow the instruction cache -- and almost every round has a single chunk anyway.
    #pragma unroll 1
            for (int base = 0; base < n; base += WS_THREADS) {
                const int i = base + threadIdx.x;
                int c = -1;
                Decision dec{0, 0, 0.0};
                if (i < n) {
                    const int c0 = slist[cur][i];
                    if (st_lab(cells[c0].st) == 0) { my_evals++; c = c0; dec = ws_decide(tv, c, g00 + (c / WL) * X + c % WL, certs); }
                    // else: decided meanwhile (pushed by a neighbour in the round it was decided itself)
                }
                __syncthreads();  // every read of this chunk is done
                if (c >= 0) {
                    if (dec.lab == 0) {  // still waiting: stays on the frontier
                        slist[cur ^ 1][atomicAdd(&s_n[cur ^ 1], 1)] = (unsigned short)c;
                    } else {
                        cells[c].st = pack_st(dec.lab, dec.ti); cells[c].v = dec.tv;
                        s_any = 1;
                        atomicAdd(&s_chg, 1);
                        if (dec.lab > 0) {
                            const int cy = c / WL, cx = c - cy * WL;   // c is evaluated: a neighbour is too unless c is on that edge of the region
    #pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int q = k == 0 ? c - WL : (k == 1 ? c - 1 : (k == 2 ? c + 1 : c + WL));
                                const bool inside = k == 0 ? cy > E0 : (k == 1 ? cx > E0 : (k == 2 ? cx < E1 - 1 : cy < E1 - 1));
                                if (inside && atomicCAS(&cells[q].st, 0ULL, ST_LISTED) == 0ULL)
                                    slist[cur ^ 1][atomicAdd(&s_n[cur ^ 1], 1)] = (unsigned short)q;
                            }
                        }
                    }
                }
                __syncthreads();
            }
            cur ^= 1;
            // every wave reads the round's flags before thread 0 may reset them at the top of the next round (blocks of
            // more than one wave: without the barrier the waves could take different branches here)
            const int any = s_any, chg = s_chg;
            if (WS_THREADS > 64) __syncthreads();
            if (any) { certs = false; continue; }
            if (certs) break;   // nothing moved even with pocket certificates: wait for the neighbours
            // local stall.  Pocket certificates cost ~40 plain rounds, and a tile that has just moved is re-run next launch
            // anyway (with its neighbours' news): only a tile that got nowhere at all tries them.
            if (chg > 0) break;
            certs = true;
        }
    }
    __syncthreads();
    // und: undecided cells left; front: those of them that touch a labelled cell.  When no tile changed any more and
    // the frontier is empty everywhere, the serial flood's heap would be empty too: the rest stays 0.
    int und = 0, front = 0;
#pragma unroll
    for (int k = 0; k < WT * WT / WS_THREADS; ++k) {
        if (WM == 0 && !((was_und >> k) & 1u)) continue;   // decided before this launch (cells outside the image are LINE)
        const int p = threadIdx.x + k * WS_THREADS;
        const int c = (p / WT + WH) * WL + (p % WT + WH);
        const unsigned long long sc = cells[c].st;
        if (st_lab(sc) == 0) {
            und++;
            front += st_lab(cells[c - WL].st) > 0 || st_lab(cells[c - 1].st) > 0 || st_lab(cells[c + 1].st) > 0 || st_lab(cells[c + WL].st) > 0;
        } else if (WM == 0) {
            st[(ty * WT + p / WT) * X + tx * WT + p % WT] = sc;   // only this tile writes its interior
        }
    }
    if (und) { atomicAdd(&s_und, und); atomicAdd(&s_front, front); }
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_und[tile] = s_und;
        tile_front[tile] = s_front;
        if (tile_wst != nullptr) tile_wst[tile] = (wcount - s_chg) | (s_chg == 0 ? WST_STUCK : 0);   // (stuck = certificates tried)
        changed_cur[tile] = s_chg > 0;
        if (s_chg > 0) atomicAdd(&info->changed_part[tile & 63], s_chg);
        if (dbg) {
            atomicAdd(&info->dbg_rounds, (unsigned long long)my_rounds);
            atomicAdd(&info->dbg_tiles, 1ULL);
            if (s_chg == 0) atomicAdd(&info->dbg_idle, 1ULL);
        }
    }
    if (dbg && my_evals) atomicAdd(&info->dbg_evals, (unsigned long long)my_evals);
}

// ---- mode A endgame: what is still undecided when the tile launches stall are stuck pockets and the pixels that
// wait for them.  Connected components of undecided pixels evolve independently (everything around them is final), so
// each one is finished by ONE wave running the serial rule -- commit the component's smallest pop time, repeat -- on an
// LDS copy of the component.  Components larger than END_CAP are left to the wide tile pass / the serial finish.
constexpr int END_CAP = 512;
constexpr int END_GRID = 4096;     // blocks of the endgame launch: they stride over the device-side component count
constexpr int WS_END_STEPS = 32;    // serial commits per component and endgame: clears the stuck seeds, the rest is tile work

struct SameU {
    const unsigned long long *st;
    __device__ __forceinline__ bool valid(int i) const { return st_lab(st[i]) == 0; }
    __device__ __forceinline__ bool same(int, int) const { return true; }
};

__global__ void __launch_bounds__(256) k_end_count(const unsigned long long *__restrict__ st, const int *__restrict__ parent,
                                                   int *__restrict__ cnt, int *__restrict__ isroot, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool u = st_lab(st[i]) == 0;
    isroot[i] = (u && parent[i] == (int)i) ? 1 : 0;
    if (u) atomicAdd(&cnt[parent[i]], 1);
}

// every component root reserves its slice of the cell buffer and its slot in the root list with two atomics (a few
// hundred to a few thousand roots per frame: cheaper than two 4 M-element scans; the order of components is irrelevant)
__global__ void __launch_bounds__(256) k_end_offsets(const int *__restrict__ cnt, const int *__restrict__ isroot,
                                                     int *__restrict__ off, int *__restrict__ roots, int *__restrict__ counters, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !isroot[i]) return;
    off[i] = atomicAdd(&counters[1], cnt[i]);
    roots[atomicAdd(&counters[0], 1)] = (int)i;
}

__global__ void __launch_bounds__(256) k_end_scatter(const unsigned long long *__restrict__ st, const int *__restrict__ parent,
                                                     const int *__restrict__ off, int *__restrict__ cursor,
                                                     int *__restrict__ cells, int *__restrict__ slot,
                                                     long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (st_lab(st[i]) != 0) return;
    const int r = parent[i];
    const int k = atomicAdd(&cursor[r], 1);
    cells[off[r] + k] = (int)i;
    slot[i] = k;
}

// One wave replays the serial flood on one component.  Every cell caches its candidate pop time
//     cand = max(own key, earliest pop time among its labelled neighbours)          (none while it has no labelled one)
// as a sortable 128-bit key (encoded value | reference pixel, own pixel) in the REGISTERS of its owner lane (cell k ->
// lane k % 64, slot k / 64).  Pop times only grow, so a commit can only GIVE a candidate to neighbours that had none: a
// step is a register scan + wave-wide minimum, the flood rule for the winner (all lanes redundantly: the LDS reads
// are broadcasts) and at most four candidate updates.
__global__ void __launch_bounds__(64) k_end_resolve(const double *__restrict__ v, unsigned long long *__restrict__ st, int Y, int X,
                                                    const int *__restrict__ roots, const int *__restrict__ cnt,
                                                    const int *__restrict__ off, const int *__restrict__ cells,
                                                    const int *__restrict__ slot, const int *__restrict__ ncomp_d, int max_steps,
                                                    WsInfo *info)
{
    constexpr int EPL = END_CAP / 64;       // cells per lane
    constexpr unsigned long long NONE = ~0ULL;
    __shared__ double cv[END_CAP];          // value of the cell
    __shared__ int cgi[END_CAP];            // global index
    __shared__ int clab[END_CAP], ctr[END_CAP];   // state: label / 0 / LINE and pop-time reference
    // neighbour tables, [direction][cell] so that lanes walking consecutive cells hit consecutive banks
    __shared__ int cnb[4][END_CAP];         // >= 0 local slot, -1 nothing (outside / line), -2 external labelled cell
    __shared__ double ev[4][END_CAP];       // external labelled neighbour: pop-time value
    __shared__ int etr[4][END_CAP], elab[4][END_CAP];
    // (the grid is launched without knowing the number of components on the host: blocks stride over the device-side count)
    const int ncomp = *ncomp_d;
    for (int comp = blockIdx.x; comp < ncomp; comp += gridDim.x) {
    const int r = roots[comp];
    const int m = cnt[r];
    if (m > END_CAP) { if (threadIdx.x == 0) atomicAdd(&info->end_oversize, m); continue; }
    const int base = off[r];
    const int lane = threadIdx.x;
    // candidate keys: hi = encoded pop-time value (NONE: not a candidate), lo = reference pixel << 32 | own pixel
    // (hi == NONE: lo == 0 "no labelled neighbour yet", lo == 1 "committed")
    unsigned long long ch[EPL], cl[EPL];
#pragma unroll
    for (int u = 0; u < EPL; ++u) {
        ch[u] = NONE; cl[u] = 1;
        const int k = lane + 64 * u;
        if (k >= m) continue;
        const int gi = cells[base + k];
        const int y = gi / X, x = gi - y * X;
        const double kv = v[gi];
        cv[k] = kv; cgi[k] = gi; clab[k] = 0; ctr[k] = 0;
        const int nb[4] = {y > 0 ? gi - X : -1, x > 0 ? gi - 1 : -1, x < X - 1 ? gi + 1 : -1, y < Y - 1 ? gi + X : -1};
        bool has = false; double tv = 0.0; int ti = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int code = -1;
            if (nb[j] >= 0) {
                const unsigned long long sq = st[nb[j]];
                const int l = st_lab(sq);
                if (l == 0) code = slot[nb[j]];
                else if (l > 0) {
                    const int tr = st_tref(sq);
                    const double qv = v[tr];
                    code = -2; elab[j][k] = l; etr[j][k] = tr; ev[j][k] = qv;
                    if (!has || qv < tv || (qv == tv && tr < ti)) { tv = qv; ti = tr; has = true; }
                }
            }
            cnb[j][k] = code;
        }
        // pop time = max(own key, earliest labelled neighbour)
        double pv = kv; int pi = gi;
        if (has && (tv > pv || (tv == pv && ti > pi))) { pv = tv; pi = ti; }
        cl[u] = 0;
        if (has) { ch[u] = enc_f64(pv + 0.0); cl[u] = ((unsigned long long)(unsigned)pi << 32) | (unsigned)gi; }
    }
    __syncthreads();
    int committed = 0;
    for (int step = 0; step < max_steps; ++step) {
        // lane-local best, then wave minimum
        unsigned long long bh = ch[0], bl = cl[0];
        int bu = 0;
#pragma unroll
        for (int u = 1; u < EPL; ++u)
            if (ch[u] < bh || (ch[u] == bh && cl[u] < bl)) { bh = ch[u]; bl = cl[u]; bu = u; }
        const unsigned long long mh = bh, ml = bl;
        for (int d = 32; d >= 1; d >>= 1) {     // (by hand: wave_reduce over the pair changes this kernel's code)
            const unsigned long long oh = __shfl_xor(bh, d, 64), ol = __shfl_xor(bl, d, 64);
            if (oh < bh || (oh == bh && ol < bl)) { bh = oh; bl = ol; }
        }
        if (bh == NONE) break;  // nothing reachable is left (wave-uniform)
        const int wl = __ffsll((unsigned long long)__ballot(mh == bh && ml == bl)) - 1;   // unique: lo holds the own pixel
        const int k = wl + 64 * __shfl(bu, wl, 64);
        const int bi = (int)(unsigned)(bl >> 32);    // the winner pops at (value bh, reference pixel bi)
        // the flood rule for the winner (same on every lane)
        const double kv = cv[k]; const int ki = cgi[k];
        int s_lab = 0, pull_lab = 0, pull_tr = 0; bool conflict = false, has_pull = false; double pt = 0.0; int pti = 0;
        int codes[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int code = cnb[j][k];
            codes[j] = code;
            double qv; int qi, ql;
            if (code == -2) { qv = ev[j][k]; qi = etr[j][k]; ql = elab[j][k]; }
            else if (code >= 0 && clab[code] > 0) { const int tr = ctr[code]; qi = tr; qv = tr == cgi[code] ? cv[code] : v[tr]; ql = clab[code]; }
            else continue;
            if (qv < kv || (qv == kv && qi < ki)) {
                if (s_lab == 0) s_lab = ql; else if (s_lab != ql) conflict = true;
            } else if (!has_pull || qv < pt || (qv == pt && qi < pti)) { has_pull = true; pt = qv; pti = qi; pull_lab = ql; pull_tr = qi; }
        }
        const int new_lab = s_lab != 0 ? (conflict ? LINE_LAB : s_lab) : pull_lab;
        const int new_tr = s_lab != 0 ? ki : pull_tr;
        // a label (not a line) gives its still candidate-less neighbours a pop time: max(their key, (bh, bi))
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int code = codes[j];
            if (code < 0 || new_lab <= 0) continue;        // wave-uniform
            const unsigned long long qh = enc_f64(cv[code] + 0.0);
            const int qg = cgi[code];
            const bool later = bh > qh || (bh == qh && bi > qg);
            const unsigned long long nh = later ? bh : qh;
            const unsigned long long nl = ((unsigned long long)(unsigned)(later ? bi : qg) << 32) | (unsigned)qg;
            const int ol = code & 63, ou = code >> 6;
#pragma unroll
            for (int u = 0; u < EPL; ++u)
                if (lane == ol && u == ou && ch[u] == NONE && cl[u] == 0) { ch[u] = nh; cl[u] = nl; }
        }
#pragma unroll
        for (int u = 0; u < EPL; ++u)
            if (lane == wl && u == bu) { ch[u] = NONE; cl[u] = 1; }
        if (lane == 0) { clab[k] = new_lab; ctr[k] = new_tr; }
        committed++;
        __syncthreads();
    }
    for (int k = lane; k < m; k += 64)
        if (clab[k] != 0) st[cgi[k]] = pack_st(clab[k], ctr[k]);
    if (lane == 0 && committed) atomicAdd(&info->end_part[comp & 63], committed);
    if (lane == 0 && committed == max_steps) atomicAdd(&info->end_unfinished, 1);   // (may have been finished exactly: harmless)
    __syncthreads();   // the LDS copy is reused by the block's next component
    }
}

__global__ void k_ws_changed_reset(WsInfo *info)
{
    info->changed = 0;
    for (int q = 0; q < 64; ++q) info->changed_part[q] = 0;
}
__global__ void k_ws_end_reset(WsInfo *info)
{
    info->end_oversize = 0; info->end_unfinished = 0; info->ncomp = 0; info->ncells = 0;
    for (int q = 0; q < 64; ++q) info->end_part[q] = 0;
}
// totals over the tiles' bookkeeping (a tile that sat a launch out keeps its last count, which is still true: only the
// tile itself decides its interior -- after an endgame every tile is woken and recounts)
__global__ void __launch_bounds__(256) k_ws_tile_totals(const int *__restrict__ tile_und, const int *__restrict__ tile_front, int ntiles,
                                                        WsInfo *info)
{
    __shared__ int su, sf;
    if (threadIdx.x == 0) { su = 0; sf = 0; }
    __syncthreads();
    int u = 0, f = 0;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ntiles; t += gridDim.x * blockDim.x) {
        const int a = tile_und[t];
        u += a;
        if (a) f += tile_front[t];
    }
    struct UF { int u, f; };
    const UF s = wave_reduce(UF{u, f}, [](UF a, UF b) { return UF{a.u + b.u, a.f + b.f}; });
    u = s.u; f = s.f;
    if ((threadIdx.x & 63) == 0 && (u | f)) { atomicAdd(&su, u); atomicAdd(&sf, f); }
    __syncthreads();
    if (threadIdx.x == 0 && (su | sf)) { atomicAdd(&info->und_total, su); atomicAdd(&info->front_total, sf); }
}
__global__ void k_ws_iter_reset(WsInfo *info)
{
    info->und_total = 0; info->front_total = 0;
    info->changed = 0; info->undecided = 0; info->unfinished = 0;
    for (int q = 0; q < 64; ++q) info->changed_part[q] = 0;
    info->dbg_rounds = 0; info->dbg_tiles = 0; info->dbg_evals = 0; info->dbg_idle = 0; info->dbg_certs = 0;
}

// ---- the schedule ------------------------------------------------------------------------------------------------------
// What the tiles leave is a serial dependency chain (plateaus larger than any certificate).  One download, the host stage
// finishes the flood with the same pop-time rule, one upload -- instead of one committed pixel per host round trip
// (which took minutes on a noisy integer image).
static int serial_finish(const double *img, unsigned long long *st, int Y, int X, int dbg, long *finished)
{
    hipStream_t s = ctx().stream;
    const long n = (long)Y * X;
    std::vector<double> himg((size_t)n);
    std::vector<uint64_t> hst((size_t)n);
    TIP_HIP(hipMemcpyAsync(himg.data(), img, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    TIP_HIP(hipMemcpyAsync(hst.data(), st, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    TIP_HIP(hipStreamSynchronize(s));
    *finished = flood_keyed_finish(himg.data(), hst.data(), Y, X);
    TIP_HIP(hipMemcpyAsync(st, hst.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    TIP_HIP(hipStreamSynchronize(s));
    if (dbg) fprintf(stderr, "ws serial finish: %ld pixels\n", *finished);
    return TIP_OK;
}

// Every phase ends in a host look at the device counters (a look idles the GPU for ~50 us):
//   1. the opening, ONE submission: open_a tile launches (the bulk), the early endgame -- what is left then are a few
//      thousand pixels in long dependency chains that would cost one latency-bound launch per tile border crossed,
//      replayed serially per component instead -- and the open_b launches its dependents need (measured on 2048^2
//      frames: endgame after 10 launches with 32 serial steps per component 2.9 ms per frame; after 6 launches 4.0 ms,
//      after 12 3.05 ms, 512 steps 3.7 ms, no early endgame 3.6 ms).  TIP_WS_DEBUG also looks after each part;
//      TIP_WS_NO_ENDGAME opens with 10 plain launches.
//   2. bursts of 2 launches while the tiles move;
//   3. on a stall: the endgame (again, for as long as it commits), then one wide pass, then the serial finish.
int flood_tiles(const double *img, WsScratch &w, int Y, int X, long *finished_serially)
{
    hipStream_t s = ctx().stream;
    const Tuning &tune = tuning();
    const long n = (long)Y * X;
    WsInfo *info = w.info;
    unsigned long long *st = w.st;
    const int open_a = tune.ws_open_a >= 0 ? tune.ws_open_a : WS_OPEN_A, open_b = tune.ws_open_b >= 0 ? tune.ws_open_b : WS_OPEN_B;
    if (open_a < 1 || open_b < 1 || open_a > 64 || open_b > 64) return fail(TIP_ERR_ARG, "watershed: bad TIP_WS_OPEN");
    const int tilesX = cdiv(X, WT_FAST), tilesY = cdiv(Y, WT_FAST), ntiles = tilesX * tilesY;
    const int wtilesX = cdiv(X, WT_WIDE), wtilesY = cdiv(Y, WT_WIDE), wntiles = wtilesX * wtilesY;
    unsigned char *wchg = w.ws.get<unsigned char>((size_t)2 * wntiles);
    int *wtile_und = w.ws.get<int>((size_t)2 * wntiles);
    unsigned char *chg = w.ws.get<unsigned char>((size_t)2 * ntiles);
    int *tile_und = w.ws.get<int>((size_t)2 * ntiles);  // [0, ntiles) undecided cells per tile, [ntiles, 2 ntiles) its frontier
    int *tile_wst = w.ws.get<int>((size_t)ntiles);
    if (!wchg || !wtile_und || !chg || !tile_und || !tile_wst) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemsetAsync(chg, 0, (size_t)2 * ntiles, s));
    TIP_HIP(hipMemsetAsync(tile_wst, 0, (size_t)ntiles * sizeof(int), s));
    // test hooks (tip_set_tuning): TIP_WS_NO_SKIP re-runs stuck tiles on every wake-up, TIP_WS_DEBUG prints the counters at
    // every look, TIP_WS_NO_ENDGAME / TIP_WS_NO_WIDE exercise the stall machinery
    int *wst_arg = tune.ws_no_skip ? nullptr : tile_wst;
    const int dbg = tune.ws_debug;
    const bool no_endgame = tune.ws_no_endgame != 0, no_wide = tune.ws_no_wide != 0;
    int *cursor = nullptr, *cellsbuf = nullptr, *slot = nullptr, *roots = nullptr;   // endgame workspaces
    int iter = 0;   // launch index: the activity words ping-pong by its parity (every block writes its word)
    WsInfo h;
    int rc, end_changed = 0;
    auto tiles = [&](int count) -> int {
        for (int k = 0; k < count; ++k, ++iter) {
            unsigned char *prev = chg + (size_t)(iter & 1) * ntiles, *cur = chg + (size_t)((iter + 1) & 1) * ntiles;
            TIP_LAUNCH("ws_tiles", (k_ws_tiles<WT_FAST, WTH_FAST, WH_FAST, WK_FAST, WM_FAST, EV_FAST>), dim3(ntiles), dim3(WTH_FAST), 0,
                       img, st, Y, X, tilesX, tilesY, (const unsigned char *)prev, cur, tile_und, tile_und + ntiles, wst_arg,
                       iter == 0 ? 1 : 0, dbg, info);
        }
        return TIP_OK;
    };
    auto look = [&](bool wide) -> int {
        TIP_LAUNCH("ws_tile_totals", k_ws_tile_totals, dim3(16), dim3(256), 0, (const int *)tile_und, (const int *)(tile_und + ntiles),
                   ntiles, info);
        TIP_HIP(hipMemcpyAsync(&h, info, sizeof h, hipMemcpyDeviceToHost, s));
        TIP_HIP(hipStreamSynchronize(s));
        for (int q = 0; q < 64; ++q) h.changed += h.changed_part[q];
        if (dbg)
            fprintf(stderr, "ws iter %d %s: tiles %llu (idle %llu, certificate rounds %llu) rounds %llu evals %llu changed %d undecided %d\n",
                    iter - 1, wide ? "wide" : "fast", h.dbg_tiles, h.dbg_idle, h.dbg_certs, h.dbg_rounds, h.dbg_evals, h.changed, h.und_total);
        return TIP_OK;
    };
    // two everyday launches, or the wide pass over every 32x32 tile (own bookkeeping arrays; every everyday tile runs in the
    // next launch and recounts), and a look
    auto burst = [&](bool wide) -> int {
        TIP_LAUNCH("ws_iter_reset", k_ws_iter_reset, dim3(1), dim3(1), 0, info);
        if (!wide) {
            if (int rc2 = tiles(2)) return rc2;
        } else {
            TIP_LAUNCH("ws_tiles_wide", (k_ws_tiles<WT_WIDE, WTH_WIDE, WH_WIDE, WK_WIDE>), dim3(wntiles), dim3(WTH_WIDE), 0, img, st, Y, X,
                       wtilesX, wtilesY, (const unsigned char *)wchg, wchg + wntiles, wtile_und, wtile_und + wntiles, (int *)nullptr, 1, dbg, info);
            TIP_HIP(hipMemsetAsync(chg + (size_t)((iter + 1) & 1) * ntiles, 1, ntiles, s));
            ++iter;
        }
        return look(wide);
    };
    // the endgame, submitted without a host round trip: components of undecided pixels, their cell lists, and one wave
    // per component replaying the serial rule (the grid strides over the device-side component count); results in
    // info->end_*; every tile is woken afterwards.  with_look: then a look at the results (end_changed: commits)
    auto endgame = [&](bool with_look) -> int {
        SameU su{st};
        if (int rc2 = uf_components(su, w.parent, Y, X)) return rc2;
        TIP_HIP(hipMemsetAsync(w.flag, 0, n * sizeof(int), s));      // cnt
        TIP_LAUNCH("ws_end_count", k_end_count, dim3(cdiv(n, 256)), dim3(256), 0, (const unsigned long long *)st,
                   (const int *)w.parent, w.flag, w.isroot, n);
        if (!cursor) {   // taken from the pool once per call
            cursor = w.ws.get<int>(n); cellsbuf = w.ws.get<int>(n); slot = w.ws.get<int>(n); roots = w.ws.get<int>(n);
        }
        if (!cursor || !cellsbuf || !slot || !roots) return TIP_ERR_NOMEM;
        TIP_LAUNCH("ws_end_reset", k_ws_end_reset, dim3(1), dim3(1), 0, info);
        TIP_LAUNCH("ws_end_offsets", k_end_offsets, dim3(cdiv(n, 256)), dim3(256), 0, (const int *)w.flag, (const int *)w.isroot,
                   w.rank /* start of every component's cells in cellsbuf */, roots, &info->ncomp, n);
        TIP_HIP(hipMemsetAsync(cursor, 0, n * sizeof(int), s));
        TIP_LAUNCH("ws_end_scatter", k_end_scatter, dim3(cdiv(n, 256)), dim3(256), 0, (const unsigned long long *)st,
                   (const int *)w.parent, (const int *)w.rank, cursor, cellsbuf, slot, n);
        TIP_LAUNCH("ws_end_resolve", k_end_resolve, dim3(END_GRID), dim3(64), 0, img, st, Y, X, (const int *)roots,
                   (const int *)w.flag, (const int *)w.rank, (const int *)cellsbuf, (const int *)slot, (const int *)&info->ncomp,
                   WS_END_STEPS, info);
        TIP_HIP(hipMemsetAsync(chg, 1, (size_t)2 * ntiles, s));
        if (!with_look) return TIP_OK;
        TIP_HIP(hipMemcpyAsync(&h, info, sizeof h, hipMemcpyDeviceToHost, s));
        TIP_HIP(hipStreamSynchronize(s));
        end_changed = 0;
        for (int q = 0; q < 64; ++q) end_changed += h.end_part[q];
        if (dbg)
            fprintf(stderr, "ws endgame: %d components, committed %d, oversize cells %d, unfinished %d\n", h.ncomp, end_changed,
                    h.end_oversize, h.end_unfinished);
        return TIP_OK;
    };
    // every component was replayed to its end: the rest is unreachable
    auto endgame_complete = [&]() { return h.end_oversize == 0 && h.end_unfinished == 0; };

    // 1. the opening
    TIP_LAUNCH("ws_iter_reset", k_ws_iter_reset, dim3(1), dim3(1), 0, info);
    if (no_endgame) {
        if ((rc = tiles(10)) || (rc = look(false))) return rc;
    } else {
        if ((rc = tiles(open_a)) || (dbg && (rc = look(false))) || (rc = endgame(dbg))) return rc;
        if (dbg) TIP_LAUNCH("ws_iter_reset", k_ws_iter_reset, dim3(1), dim3(1), 0, info);   // (the counters of the second part)
        else TIP_LAUNCH("ws_changed_reset", k_ws_changed_reset, dim3(1), dim3(1), 0, info);
        if ((rc = tiles(open_b)) || (rc = look(false))) return rc;
        if (h.und_total == 0 || endgame_complete()) return TIP_OK;
        // the endgame's dependents still moving: bursts (the opening's look does not count towards the crawl)
        if (h.changed > 0 && (rc = burst(false))) return rc;
    }
    // 2. bursts while the tiles move, 3. the stall handling
    int crawl = 0;
    bool wide = false;                  // the last look followed the wide pass
    bool endgame_due = !no_endgame;     // a stall runs the endgame until one commits nothing
    for (;;) {
        // crawl detector: a plateau of equal values floods in raster order under mode A's static keys -- one serial chain
        // that the tiles follow at ~16 pixels per launch.  When several bursts in a row decide less than 1/64 of what is
        // left, the rest goes to the serial finish instead of thousands of launches.
        crawl = (h.changed > 0 && h.und_total > 2048 && (long)h.changed * 64 < (long)h.und_total) ? crawl + 1 : 0;
        if (h.changed > 0 && crawl < 6) {
            wide = false;
        } else {
            if (h.und_total == 0) return TIP_OK;
            if (crawl >= 6) return serial_finish(img, st, Y, X, dbg, finished_serially);
            // no progress and no undecided pixel touches a labelled one: what is left is enclosed by lines and stays 0
            // (after a wide pass the fine tiles' counts are stale -- too large, never too small -- so not then)
            if (h.front_total == 0 && !wide) return TIP_OK;
            if (endgame_due) {
                // serial rule on every connected component of undecided pixels that fits one wave's LDS copy
                if ((rc = endgame(true))) return rc;
                if (endgame_complete()) return TIP_OK;
                // oversize components remain: back to the tile rounds for them, or, if the endgame committed nothing,
                // the wide pass
                endgame_due = end_changed > 0;
                wide = !endgame_due;
            } else if (!wide && !no_wide) {
                wide = true;
            } else {
                return serial_finish(img, st, Y, X, dbg, finished_serially);
            }
        }
        if ((rc = burst(wide))) return rc;
    }
}

}  // namespace tip
