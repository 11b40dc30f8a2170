// LoRA adapters beside an NF4 weight for gfx950 (MI355X): the down projection of
//     y = W_nf4 x + B (s * A x)                    A : T[R, K],  B : T[M, R],  s = lora_alpha / r (one factor per adapter row)
// Not in the reference.  An adapter cannot be merged into 4-bit weights without re-quantising them, so a QLoRA model is always
// served in this form.  Two steps, both with f32 accumulation in a fixed order (deterministic, no atomics, no allocation, no sync):
//   1. this file:  t[b][j] = scale[j] * sum_k A[j][k] x[b][k], written as f32 to float t[rows][R] and never rounded to T;
//   2. the LORA instantiations of the NF4 decode kernels (gemv_nf4.hip, gemm_small_nf4.hip, gemm_wide_nf4.hip) add
//      delta[b][r] = sum_j f32(B[r][j]) t[b][j] to their f32 row sum before anything is rounded (helpers in lora_nf4.h).
//
// lora_down_kernel: one 256-thread workgroup per adapter row j and 8 activation rows.  The four waves split K in 8-element units
// (16-byte loads of a 16-bit T, two for f32), unit u of a pass belongs to thread u % 256; a pass covers 256 * kDownUnits units =
// 8192 elements, so for K <= 8192 the row of A is read once and stays in registers (as f32) while the workgroup goes over its
// activation rows, four at a time so that their x loads are in flight together.  Per activation row the lanes' partial sums meet
// through the dpp chain of the GEMV (wave_sum), lane 0 of every wave keeps the wave's running sum over the passes in its own LDS
// slot, and after the last pass thread b adds the four slots of row b in wave order.  A unit past the end of the row is clamped
// and its A fragment zeroed, a row past the batch is clamped and not stored (branch-free loads).
#include "gemv_common.h"
#include "lora_nf4.h"

namespace fp4 {

namespace {

constexpr int kDownMaxRows = 64;
constexpr int kDownUnits = 4;     // 8-element units per thread and pass
constexpr int kDownRowsPerWg = 8;  // activation rows per workgroup (blockIdx.y), so that wide batches do not serialise on one CU
constexpr int kDownGroup = 4;      // activation rows whose loads are in flight together

template <int DT>
__global__ __launch_bounds__(256) void lora_down_kernel(const void *__restrict__ x, const void *__restrict__ A,
                                                        const float *__restrict__ scale, float *__restrict__ t, int Bt, int R, int K) {
    __shared__ float s_red[kDownRowsPerWg][4];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x;
    const int b_base = blockIdx.y * kDownRowsPerWg;
    const int U = K >> 3;  // units per row
    for (int u0 = 0; u0 < U; u0 += 256 * kDownUnits) {
        int uidx[kDownUnits];
        f32x4 a[kDownUnits][2];
#pragma unroll
        for (int i = 0; i < kDownUnits; ++i) {
            const int u = u0 + i * 256 + tid;
            const bool live = u < U;
            uidx[i] = live ? u : U - 1;
            lora_load8<DT>(A, int64_t(j) * U + uidx[i], a[i][0], a[i][1]);
            if (!live) a[i][0] = a[i][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int g = 0; g < kDownRowsPerWg; g += kDownGroup) {
            if (b_base + g >= Bt) break;  // uniform
            float p[kDownGroup];
#pragma unroll
            for (int r = 0; r < kDownGroup; ++r) {
                const int b = b_base + g + r < Bt ? b_base + g + r : Bt - 1;  // a row past the batch is computed, never stored
                p[r] = 0.0f;
#pragma unroll
                for (int i = 0; i < kDownUnits; ++i) {
                    f32x4 x0, x1;
                    lora_load8<DT>(x, int64_t(b) * U + uidx[i], x0, x1);
                    p[r] = lora_dot8(a[i][0], a[i][1], x0, x1, p[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < kDownGroup; ++r) {
                const float v = wave_sum(p[r]);
                if (lane == 0) s_red[g + r][wave] = u0 == 0 ? v : s_red[g + r][wave] + v;  // a slot is only ever touched by this lane
            }
        }
    }
    __syncthreads();
    const int b = b_base + tid;
    if (tid < kDownRowsPerWg && b < Bt)
        t[int64_t(b) * R + j] = scale[j] * (((s_red[tid][0] + s_red[tid][1]) + s_red[tid][2]) + s_red[tid][3]);
}

// lora_down_kernel with the adapter chosen per activation row: A_stack : T[n_adapters][R][K], scale_stack : float[n_adapters][R],
// ids : int32[Bt] (read here, never on the host).  Unit-to-thread mapping, pass structure, wave_sum, slot order and the final
// four-slot add are lora_down_kernel's, so row b carries the bits of lora_down_kernel on A_stack[ids[b]].  The A fragment is
// reloaded only when a row's adapter differs from the one held in registers (ids[b] is uniform over the workgroup: a uniform
// branch); four rows of one adapter keep their x loads in flight together as there, a mixed group goes row by row.  A row whose
// id names no adapter touches neither A nor x and gets t = +0.
template <int DT>
__global__ __launch_bounds__(256) void lora_down_multi_kernel(const void *__restrict__ x, const void *__restrict__ A_stack,
                                                              const float *__restrict__ scale_stack, const int *__restrict__ ids,
                                                              float *__restrict__ t, int Bt, int R, int K, int n_adapters) {
    __shared__ float s_red[kDownRowsPerWg][4];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x;
    const int b_base = blockIdx.y * kDownRowsPerWg;
    const int U = K >> 3;  // units per row
    auto adapter_of = [&](int b) {  // -1: none
        const int id = ids[b];
        return uint32_t(id) < uint32_t(n_adapters) ? id : -1;
    };
    for (int u0 = 0; u0 < U; u0 += 256 * kDownUnits) {
        int uidx[kDownUnits];
        bool live[kDownUnits];
#pragma unroll
        for (int i = 0; i < kDownUnits; ++i) {
            const int u = u0 + i * 256 + tid;
            live[i] = u < U;
            uidx[i] = live[i] ? u : U - 1;
        }
        f32x4 a[kDownUnits][2];
        int held = -1;  // the adapter whose fragment of this pass is in `a`
        auto hold = [&](int id) {
            if (id == held) return;  // uniform
#pragma unroll
            for (int i = 0; i < kDownUnits; ++i) {
                lora_load8<DT>(A_stack, (int64_t(id) * R + j) * U + uidx[i], a[i][0], a[i][1]);
                if (!live[i]) a[i][0] = a[i][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
            held = id;
        };
        auto row_dot = [&](int b) {
            float p = 0.0f;
#pragma unroll
            for (int i = 0; i < kDownUnits; ++i) {
                f32x4 x0, x1;
                lora_load8<DT>(x, int64_t(b) * U + uidx[i], x0, x1);
                p = lora_dot8(a[i][0], a[i][1], x0, x1, p);
            }
            return p;
        };
#pragma unroll
        for (int g = 0; g < kDownRowsPerWg; g += kDownGroup) {
            if (b_base + g >= Bt) break;  // uniform
            int bb[kDownGroup], id[kDownGroup];
#pragma unroll
            for (int r = 0; r < kDownGroup; ++r) {
                bb[r] = b_base + g + r < Bt ? b_base + g + r : Bt - 1;  // a row past the batch is computed, never stored
                id[r] = adapter_of(bb[r]);
            }
            float p[kDownGroup];
            if (id[0] == id[1] && id[1] == id[2] && id[2] == id[3]) {  // uniform
                if (id[0] < 0) continue;
                hold(id[0]);
#pragma unroll
                for (int r = 0; r < kDownGroup; ++r) p[r] = row_dot(bb[r]);
            } else {
#pragma unroll
                for (int r = 0; r < kDownGroup; ++r) {
                    p[r] = 0.0f;
                    if (id[r] < 0) continue;
                    hold(id[r]);
                    p[r] = row_dot(bb[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < kDownGroup; ++r) {
                if (id[r] < 0) continue;  // uniform: its slots are never read
                const float v = wave_sum(p[r]);
                if (lane == 0) s_red[g + r][wave] = u0 == 0 ? v : s_red[g + r][wave] + v;  // a slot is only ever touched by this lane
            }
        }
    }
    __syncthreads();
    const int b = b_base + tid;
    if (tid < kDownRowsPerWg && b < Bt) {
        const int id = adapter_of(b);
        t[int64_t(b) * R + j] =
            id < 0 ? 0.0f : scale_stack[int64_t(id) * R + j] * (((s_red[tid][0] + s_red[tid][1]) + s_red[tid][2]) + s_red[tid][3]);
    }
}

}  // namespace

int lora_check_stack(const char *name, const void *B_stack, const int32_t *ids, int64_t n_adapters, const float *t, int64_t R) {
    if (n_adapters < 1 || !ids) {
        set_error("%s: n_adapters=%lld ids=%p (need at least one adapter in the stack and a device array of ids)", name,
                  (long long)n_adapters, (const void *)ids);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    return lora_check_adapter(name, B_stack, t, R);
}

int lora_check_adapter(const char *name, const void *lora_B, const float *t, int64_t R) {
    if (R < 0) {
        set_error("%s: R=%lld (need R >= 0)", name, (long long)R);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    const uintptr_t align = reinterpret_cast<uintptr_t>(lora_B) | reinterpret_cast<uintptr_t>(t);
    if (R < 8 || R > 256 || (R % 8) != 0 || (align & 15u) != 0) {
        set_error("%s: the adapter term is not available for R=%lld (needs a rank that is a multiple of 8 in 8..256 - pad A and B "
                  "with zeros - and 16-byte aligned lora_B and t); run the plain fused op and add the adapter separately",
                  name, (long long)R);
        return FP4_ERR_UNSUPPORTED;
    }
    return FP4_OK;
}

}  // namespace fp4

extern "C" int fp4_hip_lora_down(const void *x, const void *A, const float *scale, float *t, int64_t Bt, int64_t R, int64_t K, int dtype,
                                 void *stream) {
    using namespace fp4;
    if (Bt < 0 || R < 0 || K < 0) {
        set_error("fp4_hip_lora_down: Bt=%lld R=%lld K=%lld (need Bt, R, K >= 0)", (long long)Bt, (long long)R, (long long)K);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (dtype != FP4_DTYPE_F16 && dtype != FP4_DTYPE_BF16 && dtype != FP4_DTYPE_F32) {
        set_error("fp4_hip_lora_down: unsupported dtype %d", dtype);
        return FP4_ERR_UNSUPPORTED;
    }
    const uintptr_t align = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(A);
    if (Bt > kDownMaxRows || R < 8 || R > 256 || (R % 8) != 0 || K == 0 || (K % 8) != 0 || K > (int64_t(1) << 24) || (align & 15u) != 0) {
        set_error("fp4_hip_lora_down: Bt=%lld R=%lld K=%lld is not covered (1..64 rows, a rank that is a multiple of 8 in 8..256, "
                  "K %% 8 == 0, 16-byte aligned x and A); run the down projection as a dense product",
                  (long long)Bt, (long long)R, (long long)K);
        return FP4_ERR_UNSUPPORTED;
    }
    if (Bt == 0) return FP4_OK;
    if (!x || !A || !scale || !t) {
        set_error("fp4_hip_lora_down: null pointer");
        return FP4_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)R, (unsigned)((Bt + kDownRowsPerWg - 1) / kDownRowsPerWg)), block(256);
    switch (dtype) {
        case FP4_DTYPE_F16:
            hipLaunchKernelGGL((lora_down_kernel<FP4_DTYPE_F16>), grid, block, 0, s, x, A, scale, t, (int)Bt, (int)R, (int)K);
            break;
        case FP4_DTYPE_BF16:
            hipLaunchKernelGGL((lora_down_kernel<FP4_DTYPE_BF16>), grid, block, 0, s, x, A, scale, t, (int)Bt, (int)R, (int)K);
            break;
        default:
            hipLaunchKernelGGL((lora_down_kernel<FP4_DTYPE_F32>), grid, block, 0, s, x, A, scale, t, (int)Bt, (int)R, (int)K);
            break;
    }
    return check_launch("fp4_hip_lora_down");
}

extern "C" int fp4_hip_lora_down_multi(const void *x, const void *A_stack, const float *scale_stack, const int32_t *ids, float *t,
                                       int64_t Bt, int64_t n_adapters, int64_t R, int64_t K, int dtype, void *stream) {
    using namespace fp4;
    if (Bt < 0 || R < 0 || K < 0) {
        set_error("fp4_hip_lora_down_multi: Bt=%lld R=%lld K=%lld (need Bt, R, K >= 0)", (long long)Bt, (long long)R, (long long)K);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (n_adapters < 1 || !ids) {
        set_error("fp4_hip_lora_down_multi: n_adapters=%lld ids=%p (need at least one adapter in the stack and a device array of ids)",
                  (long long)n_adapters, (const void *)ids);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (dtype != FP4_DTYPE_F16 && dtype != FP4_DTYPE_BF16 && dtype != FP4_DTYPE_F32) {
        set_error("fp4_hip_lora_down_multi: unsupported dtype %d", dtype);
        return FP4_ERR_UNSUPPORTED;
    }
    const uintptr_t align = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(A_stack);
    // K % 8 == 0 keeps every slice of a 16-byte aligned stack aligned; n_adapters * R rows of A stay within the int row arithmetic
    if (Bt > kDownMaxRows || R < 8 || R > 256 || (R % 8) != 0 || K == 0 || (K % 8) != 0 || K > (int64_t(1) << 24) || (align & 15u) != 0 ||
        n_adapters > (int64_t(1) << 20)) {
        set_error("fp4_hip_lora_down_multi: Bt=%lld R=%lld K=%lld n_adapters=%lld is not covered (1..64 rows, a rank that is a multiple of 8 "
                  "in 8..256, K %% 8 == 0, 16-byte aligned x and A_stack, at most 2^20 adapters); run the down projection as a dense product",
                  (long long)Bt, (long long)R, (long long)K, (long long)n_adapters);
        return FP4_ERR_UNSUPPORTED;
    }
    if (Bt == 0) return FP4_OK;
    if (!x || !A_stack || !scale_stack || !t) {
        set_error("fp4_hip_lora_down_multi: null pointer");
        return FP4_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)R, (unsigned)((Bt + kDownRowsPerWg - 1) / kDownRowsPerWg)), block(256);
    switch (dtype) {
        case FP4_DTYPE_F16:
            hipLaunchKernelGGL((lora_down_multi_kernel<FP4_DTYPE_F16>), grid, block, 0, s, x, A_stack, scale_stack, ids, t, (int)Bt, (int)R,
                               (int)K, (int)n_adapters);
            break;
        case FP4_DTYPE_BF16:
            hipLaunchKernelGGL((lora_down_multi_kernel<FP4_DTYPE_BF16>), grid, block, 0, s, x, A_stack, scale_stack, ids, t, (int)Bt, (int)R,
                               (int)K, (int)n_adapters);
            break;
        default:
            hipLaunchKernelGGL((lora_down_multi_kernel<FP4_DTYPE_F32>), grid, block, 0, s, x, A_stack, scale_stack, ids, t, (int)Bt, (int)R,
                               (int)K, (int)n_adapters);
            break;
    }
    return check_launch("fp4_hip_lora_down_multi");
}
