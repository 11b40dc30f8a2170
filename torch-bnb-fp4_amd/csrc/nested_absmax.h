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

// The statistics' part of the argument check of the entry points that read them compressed (gemv_nf4.hip, gemm_wide_nf4.hip), ahead
// of the un-nested twin's own check: FP4_OK, or the status to return with the message set.  `kind` is what reads the groups ("GEMV",
// "GEMM"), `plain_op` the entry point to run on the expanded statistics instead.
inline int nested_check_args(const char *name, const char *kind, const char *plain_op, int epilogue, int nested_blocksize, int64_t M,
                             int64_t K, const float *nested_absmax, const float *code256) {
    if (epilogue != FP4_EPILOGUE_NONE && epilogue != FP4_EPILOGUE_SILU_MUL_PAIRS) {
        set_error("%s: unknown epilogue %d", name, epilogue);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (nested_blocksize <= 0) {
        set_error("%s: nested_blocksize=%d (need a positive group size)", name, nested_blocksize);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (M > 0 && K > 0 && (!nested_absmax || !code256)) {  // absmax_u8 is checked with the other operands
        set_error("%s: null pointer", name);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (nested_blocksize != (1 << kNestedGemvShift)) {
        set_error("%s: nested_blocksize %d is not covered (the %s reads groups of 256 blocks); expand the statistics with "
                  "fp4_hip_absmax_unnest and run %s", name, nested_blocksize, kind, plain_op);
        return FP4_ERR_UNSUPPORTED;
    }
    return FP4_OK;
}

}  // namespace fp4
