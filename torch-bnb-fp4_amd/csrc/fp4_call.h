// The host side that the FP4 decode entry points share (gemv_fp4.hip: one row; gemm_small_fp4.hip, gemm_wide_fp4.hip,
// gemm_splitk_fp4.hip: 1..128 rows), and the two conversions the NF4 half (nf4_call.h) shares with them.
//
// An extern "C" entry point fills an Fp4Call by member name and hands it on; every host function below it takes the descriptor, none
// a row of operands.  Each kernel family has ONE launch function, launch_<family>(kernel, grid, block, lds, call [, what only that
// family takes]), which is the only place the family's kernel argument list is spelt: launch_gemm16() below for the 16-bit matrix
// kernels of three files, launch_gemv16() / launch_gemv32() in gemv_fp4.hip, launch_xstat() / launch_reduce() in gemm_splitk_fp4.hip.
// A dispatcher picks the template integers and the grid and calls it.  with_dtype() turns the runtime dtype into the template
// argument, epilogue_mode() the ABI's `epilogue` into the kernels' `mode`, for_row_chunks() splits more rows than one launch takes.
//
// How to add a kernel to a family: instantiate it in the family's dispatcher and pass it to the family's launch function; no
// operand is named there.  A kernel with another argument list is a new family: one launch function beside it.
#pragma once

#include <type_traits>

#include "gemv_common.h"

namespace fp4 {

struct Fp4Call {
    const void *x = nullptr;  // [B][K] of dtype
    const uint8_t *W = nullptr;
    const float *absmax = nullptr;  // one per block
    const void *bias = nullptr, *residual = nullptr;
    void *out = nullptr;
    int64_t B = 1, M = 0, K = 0;  // B activation rows (the GEMV: 1)
    int blocksize = 0, dtype = 0;
    int mode = 0;  // the flags of gemv_common.h: kModeSiluMulPairs, kModeOutF32
    hipStream_t stream = nullptr;
    void *workspace = nullptr;  // fp4_hip_gemm_small_ws only
    int64_t workspace_bytes = 0;

    int bs_shift() const { return ilog2_exact(blocksize); }  // -1: not a power of two
    bool gated() const { return mode & kModeSiluMulPairs; }
    int64_t M_out() const { return gated() ? M / 2 : M; }
    // the operands as the 16-bit kernels take them
    const uint16_t *x16() const { return static_cast<const uint16_t *>(x); }
    const uint16_t *bias16() const { return static_cast<const uint16_t *>(bias); }
    const uint16_t *residual16() const { return static_cast<const uint16_t *>(residual); }
    uint16_t *out16() const { return static_cast<uint16_t *>(out); }
};

// runtime dtype (validated: fp16 or bf16, with WITH_F32 also f32) -> template argument: f(std::integral_constant<int, FP4_DTYPE_*>{}),
// whose result is returned
template <bool WITH_F32 = false, typename F>
inline auto with_dtype(int dtype, F &&f) {
    if (dtype == FP4_DTYPE_F16) return f(std::integral_constant<int, FP4_DTYPE_F16>{});
    if constexpr (WITH_F32) {
        if (dtype == FP4_DTYPE_F32) return f(std::integral_constant<int, FP4_DTYPE_F32>{});
    }
    return f(std::integral_constant<int, FP4_DTYPE_BF16>{});
}

// `epilogue` of the C ABI -> the kernels' `mode`, or -1 with the message set (the caller returns FP4_ERR_INVALID_ARGUMENT)
inline int epilogue_mode(const char *name, int epilogue) {
    if (epilogue != FP4_EPILOGUE_NONE && epilogue != FP4_EPILOGUE_SILU_MUL_PAIRS) {
        set_error("%s: unknown epilogue %d", name, epilogue);
        return -1;
    }
    return epilogue == FP4_EPILOGUE_SILU_MUL_PAIRS ? kModeSiluMulPairs : 0;
}

// The one launch of the 16-bit matrix kernels (gemm16_small, gemm16_mfma and its persistent form, gemm16_wide_*): their argument list
// (x, W, absmax, bias, residual, out, B, M, K, [what the family adds: bs_shift; ntiles,] mode), spelt here only.  FP4_OK.
template <typename Kern, typename... Extra>
inline int launch_gemm16(Kern kern, dim3 grid, dim3 block, size_t lds, const Fp4Call &c, Extra... extra) {
    hipLaunchKernelGGL(kern, grid, block, lds, c.stream, c.x16(), c.W, c.absmax, c.bias16(), c.residual16(), c.out16(), (int)c.B, (int)c.M,
                       (int)c.K, extra..., c.mode);
    return FP4_OK;
}

// f(chunk) over the rows of a 16-bit call in even chunks of at most `unit` rows, one after the other: x, residual and out advanced
// (a null residual stays null; whether a null out may is the caller's rule, which checks it first or not at all), until one returns
// another status than FP4_OK, which is returned
template <typename F>
inline int for_row_chunks(const Fp4Call &c, int64_t unit, F &&f) {
    const int64_t chunks = (c.B + unit - 1) / unit, per = (c.B + chunks - 1) / chunks;
    for (int64_t b0 = 0; b0 < c.B; b0 += per) {
        Fp4Call part = c;
        part.B = c.B - b0 < per ? c.B - b0 : per;
        part.x = static_cast<const uint8_t *>(c.x) + size_t(b0) * size_t(c.K) * 2;
        if (c.residual) part.residual = static_cast<const uint8_t *>(c.residual) + size_t(b0) * size_t(c.M_out()) * 2;
        if (c.out) part.out = static_cast<uint8_t *>(c.out) + size_t(b0) * size_t(c.M_out()) * 2;
        if (const int rc = f(part)) return rc;
    }
    return FP4_OK;
}

}  // namespace fp4
