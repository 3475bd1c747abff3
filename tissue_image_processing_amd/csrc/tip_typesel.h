// tip_typesel.h -- the cell-type selector shared by the window statistics (tip_spatial.hip) and the neighbour-graph features
// (tip_graph.hip).
#pragma once
#include "tip_internal.h"

namespace tip {

// is_positive_for_type (ti.py:146-176) on one type byte: the bit is set and the byte is not the invalid marker 255; sel_kind
// 0 = no selector, 1 = positive, 2 = not positive (the negation takes invalid bytes, as upstream's ~ does)
__device__ __forceinline__ bool sp_selected(uint8_t t, int sel_kind, int bit)
{
    if (sel_kind == 0) return true;
    const bool pos = ((t >> bit) & 1) && t != 255;
    return sel_kind == 1 ? pos : !pos;
}

struct Selector { int kind = 0, bit = 0; };   // what the kernels take; the default selects every row

// the C-ABI's (sel_bit, sel_positive) as a Selector; allow_none: sel_bit -1 is "no selector"
inline int parse_selector(const char *who, int sel_bit, int sel_positive, bool allow_none, Selector &sel)
{
    if (sel_bit > 7 || sel_bit < (allow_none ? -1 : 0))
        return fail(TIP_ERR_ARG, allow_none ? "%s: type bit %d (0..7, or -1 for no selector)" : "%s: type bit %d (0..7)", who, sel_bit);
    sel.kind = sel_bit < 0 ? 0 : (sel_positive ? 1 : 2);
    sel.bit = sel_bit < 0 ? 0 : sel_bit;
    return TIP_OK;
}

}  // namespace tip
