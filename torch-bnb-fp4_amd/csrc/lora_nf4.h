// Device helpers of the LoRA adapter term of the NF4 decode kernels (gemv_nf4.hip, gemm_small_nf4.hip, gemm_wide_nf4.hip) and of
// the down projection (lora_nf4.hip):
//     y = W_nf4 x + B (s * A x)        A : T[R, K],  B : T[M, R],  t = s * A x : float[rows][R] (never rounded to T)
// Only LORA instantiations use them: the plain and the fused kernels compile to what they were.
#pragma once

#include "fp4_common.h"

namespace fp4 {
namespace {

// 8 elements of T as loaded (one u32x4 of a 16-bit T, two of f32) -> f32
template <int DT>
__device__ __forceinline__ void lora_widen8(const u32x4 *v, f32x4 &a, f32x4 &b) {
    if constexpr (DT == FP4_DTYPE_F32) {
        a = __builtin_bit_cast(f32x4, v[0]);
        b = __builtin_bit_cast(f32x4, v[1]);
    } else {
        a = f32x4{to_f32<DT>(uint16_t(v[0].x & 0xFFFFu)), to_f32<DT>(uint16_t(v[0].x >> 16)), to_f32<DT>(uint16_t(v[0].y & 0xFFFFu)),
                  to_f32<DT>(uint16_t(v[0].y >> 16))};
        b = f32x4{to_f32<DT>(uint16_t(v[0].z & 0xFFFFu)), to_f32<DT>(uint16_t(v[0].z >> 16)), to_f32<DT>(uint16_t(v[0].w & 0xFFFFu)),
                  to_f32<DT>(uint16_t(v[0].w >> 16))};
    }
}

// 8 consecutive elements of a T array (unit i8 = elements [8 i8, 8 i8 + 8): one 16-byte load of 16-bit T, two of f32) as f32
template <int DT>
__device__ __forceinline__ void lora_load8(const void *p, int64_t i8, f32x4 &a, f32x4 &b) {
    constexpr int kRegs = DT == FP4_DTYPE_F32 ? 2 : 1;
    u32x4 v[kRegs];
#pragma unroll
    for (int q = 0; q < kRegs; ++q) v[q] = reinterpret_cast<const u32x4 *>(p)[i8 * kRegs + q];
    lora_widen8<DT>(v, a, b);
}

// sum_i a[i] * b[i] over 8 elements on top of `acc`, in element order
__device__ __forceinline__ float lora_dot8(f32x4 a0, f32x4 a1, f32x4 b0, f32x4 b1, float acc) {
    acc = __builtin_fmaf(a0.x, b0.x, acc);
    acc = __builtin_fmaf(a0.y, b0.y, acc);
    acc = __builtin_fmaf(a0.z, b0.z, acc);
    acc = __builtin_fmaf(a0.w, b0.w, acc);
    acc = __builtin_fmaf(a1.x, b1.x, acc);
    acc = __builtin_fmaf(a1.y, b1.y, acc);
    acc = __builtin_fmaf(a1.z, b1.z, acc);
    acc = __builtin_fmaf(a1.w, b1.w, acc);
    return acc;
}

// delta = sum_j f32(B_row[j]) * t_row[j], j = 0 .. R - 1 in order (R % 8 == 0, both rows 16-byte aligned): what one thread of the
// matrix-core kernels' store loop adds to its finished f32 sum before anything is rounded
template <int DT>
__device__ __forceinline__ float lora_delta(const void *B_row, const float *t_row, int R) {
    float d = 0.0f;
    for (int j8 = 0; j8 < (R >> 3); ++j8) {
        f32x4 b0, b1;
        lora_load8<DT>(B_row, j8, b0, b1);
        const f32x4 t0 = reinterpret_cast<const f32x4 *>(t_row)[2 * j8], t1 = reinterpret_cast<const f32x4 *>(t_row)[2 * j8 + 1];
        d = lora_dot8(b0, b1, t0, t1, d);
    }
    return d;
}

// Several adapters in one batch (the MULTI instantiations): B_stack holds n_adapters arrays T[M][R] one after another and ids[n]
// names the adapter of activation row n.  -> the slice of row n's adapter, or nullptr where ids[n] is outside 0 .. n_adapters - 1
// ("no adapter for this row": no address is formed from such an id).  The slice offset id * M * R is 64-bit.
template <typename T>
__device__ __forceinline__ const T *lora_stack_slice(const T *B_stack, const int *ids, int n_adapters, int n, int M, int R) {
    const int id = ids[n];
    if (uint32_t(id) >= uint32_t(n_adapters)) return nullptr;
    return B_stack + int64_t(id) * M * R;
}

}  // namespace

// the adapter checks shared by fp4_hip_gemv_lora_nf4 / fp4_hip_gemm_lora_nf4 (lora_nf4.hip): FP4_OK, or the status to return with
// the message set - a null pointer or R <= 0 is an invalid argument, a rank or an alignment the kernels do not cover is unsupported
int lora_check_adapter(const char *name, const void *lora_B, const float *t, int64_t R);

// the same for the *_lora_multi_* entry points: n_adapters < 1 or a null ids is an invalid argument, then lora_check_adapter on the
// stack's base (R % 8 == 0 keeps every slice of an aligned stack aligned)
int lora_check_stack(const char *name, const void *B_stack, const int32_t *ids, int64_t n_adapters, const float *t, int64_t R);

}  // namespace fp4
