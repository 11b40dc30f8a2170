// Device helpers shared by the five translation units that drive v_mfma_f32_16x16x32_{bf16,f16}: gemm_small_fp4.hip,
// gemm_wide_fp4.hip, gemm_splitk_fp4.hip, gemm_small_nf4.hip and gemm_wide_nf4.hip.  (The NF4 hi / lo decode has a header of its
// own, nf4_mfma.h, so that an edit there leaves the FP4 kernels' sources as they were.)
#pragma once

#include "gemv_common.h"

namespace fp4 {
namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// c + a * b on one 16x16 tile, K = 32: fragments of eight 16-bit T per lane, as packed dwords
template <int DT>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (DT == FP4_DTYPE_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// 8 FP4 weights of one packed dword as 12*code in natural order: (e0,e1) (e2,e3) (e4,e5) (e6,e7)
template <int DT>
__device__ __forceinline__ u32x4 decode8_natural(uint32_t q) {
    uint32_t P[4];
    decode8<DT>(q, P);
    u32x4 n;
    n.x = perm(P[2], P[0], 0x05040100u);
    n.y = perm(P[2], P[0], 0x07060302u);
    n.z = perm(P[3], P[1], 0x05040100u);
    n.w = perm(P[3], P[1], 0x07060302u);
    return n;
}

// LDS-DMA (global_load_lds_dwordx4, no VGPR staging): lane l's 16 bytes at `src` land at lds_wave_base + 16 l
__device__ __forceinline__ void lds_dma16(const uint8_t *src, uint8_t *lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// counted wait: at most N of this wave's vector-memory operations stay in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

}  // namespace
}  // namespace fp4
