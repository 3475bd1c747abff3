// tip_typesel.h -- the cell-type selector shared by the window statistics (tip_spatial.hip) and the neighbour-graph features
// (tip_graph.hip).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace tip {

// is_positive_for_type (ti.py:146-176) on one type byte: the bit is set and the byte is not the invalid marker 255; sel_kind
// 0 = no selector, 1 = positive, 2 = not positive (the negation takes invalid bytes, as upstream's ~ does)
__device__ __forceinline__ bool sp_selected(uint8_t t, int sel_kind, int bit)
{
    if (sel_kind == 0) return true;
    const bool pos = ((t >> bit) & 1) && t != 255;
    return sel_kind == 1 ? pos : !pos;
}

}  // namespace tip
