// Double-quantised (nested) absmax, bitsandbytes' compress_statistics: the per-block scale is stored as a uint8 code into a
// 256-entry f32 table, one f32 scale per group of `nested_blocksize` blocks and one f32 offset per weight.
//     absmax[i] = fl32( fl32( code256[q[i]] * nested_absmax[i / g] ) + offset )
// Two f32 roundings, as bitsandbytes' dequantize_blockwise followed by `absmax += offset` gives them: never one fused multiply-add.
// Shared by the expander / compressor (nested_absmax.hip) and the NESTED instantiations of the NF4 GEMV (gemv_nf4.hip), so the GEMV
// forms bit for bit the scale the expander writes.
#pragma once

#include "fp4_common.h"

namespace fp4 {

constexpr int kNestedGemvShift = 8;  // the GEMV reads groups of 256 blocks only (what every bitsandbytes file holds)

__device__ __forceinline__ float unnest_scale(float code, float group_scale, float offset) {
#pragma clang fp contract(off)
    const float t = code * group_scale;
    return t + offset;
}

}  // namespace fp4
