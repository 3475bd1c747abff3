// tip_ws.h -- shared by the watershed's units (not part of the C-ABI): tip_watershed.hip (markers, choice of mode,
// exported entries), tip_ws_tiles.hip (mode A) and tip_ws_binary.hip (mode B).
#pragma once
#include "tip_internal.h"

namespace tip {

__device__ __forceinline__ unsigned long long enc_f64(double d)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

__device__ __forceinline__ unsigned long long pack_st(int lab, int tref)
{
    return ((unsigned long long)(unsigned)tref << 32) | (unsigned)lab;
}
__device__ __forceinline__ int st_lab(unsigned long long s) { return (int)(unsigned)(s & 0xffffffffULL); }
__device__ __forceinline__ int st_tref(unsigned long long s) { return (int)(unsigned)(s >> 32); }

constexpr int LINE_LAB = -1;

struct WsInfo {           // device-resident scalars
    unsigned long long emin, emax;   // encoded min / max of the image
    unsigned long long n_other;      // pixels that are neither min nor max
    int ties;                        // equal-valued non-marker neighbours exist
    int n_markers;
    int changed, undecided;          // per-iteration counters (mode A) / frontier, pending (mode B)
    int unfinished, pad_;            // endgame: components whose replay hit the step limit
    int changed_part[64];            // tile / component kernels spread their `changed` adds over 64 words: thousands of
                                     // same-address atomics per launch serialise in L2 (host adds them up)
    unsigned long long dbg_rounds, dbg_tiles, dbg_evals;  // diagnostics (TIP_WS_DEBUG=1)
    unsigned long long dbg_idle, dbg_certs;               // tile instances that decided nothing / that ran a certificate round
    // endgame results (own words: the tile launches that follow the endgame in the same submission must not clobber them)
    int end_part[64];                // serial commits, spread like changed_part
    int end_oversize, end_unfinished;   // cells of components larger than END_CAP / components whose replay hit the step limit
    int ncomp, ncells;               // endgame: components of undecided pixels and their cells (k_end_offsets)
    int und_total, front_total;      // k_ws_tile_totals: undecided pixels / those of them that touch a labelled pixel
};

// The n-sized device buffers of one watershed call.  The marker stage fills them (st: packed state, label | pop-time
// reference << 32); the flood modes reuse the others as their own scratch and take further workspaces from `ws`.
struct WsScratch {
    WsGuard ws;
    WsInfo *info;
    int *parent, *flag, *isroot, *rank;
    unsigned long long *st;
};

int marker_pop_order(const uint8_t *c, long M, uint32_t *order);   // tip_heaporder.hip
int flood_exact(const double *img, const int32_t *markers, int32_t *labels, int Y, int X);   // tip_ws_serial.hip
long flood_keyed_finish(const double *img, uint64_t *st, int Y, int X);
// mode A (tip_ws_tiles.hip); *finished_serially: pixels the host's serial finish decided, -1 if it did not run
int flood_tiles(const double *img, WsScratch &w, int Y, int X, long *finished_serially);
// mode B (tip_ws_binary.hip)
int flood_two_valued(WsScratch &w, int Y, int X);

}  // namespace tip
