// Nested (double-quantised) absmax for gfx950 -- bitsandbytes' compress_statistics, restated (bitsandbytes is not on the build or
// test machines; tests/nested_ref.py restates the rules in numpy).  Not in the reference.
//
// fp4_hip_absmax_unnest: absmax[i] = fl32(fl32(code256[q[i]] * nested_absmax[i / g]) + offset), a multiply and then an add
//   (unnest_scale, nested_absmax.h).  One lane expands 4 consecutive blocks: one dword of codes in, one 16-byte store out (g >= 64, so
//   the 4 share a group); operands that are not aligned for that, and the ragged tail, go element by element.  The 256-entry table
//   is copied to LDS once per workgroup.  `offset` is a kernel argument: nothing is read from the host at run time.
//
// fp4_hip_absmax_nest: the writing side, one workgroup per group of g blocks:
//   v = fl32(a - offset), m = max|v| over the group, n = fl32(v * fl32(1 / m)), q = the index of the table entry nearest to n
//   (distances compared in f64, where the difference of two f32 is exact for every pair that can be nearest; the lowest index wins
//   a tie), out_nested_absmax = m.  A group with m == 0 takes n = 0: every q is the index of the table's 0.0 and the group expands
//   to exactly `offset`.  The search is a scan of all 256 entries (every lane reads the same LDS word: a broadcast), so the table
//   needs no order; this runs once per saved weight, not per token.
#include "fp4_common.h"
#include "nested_absmax.h"

namespace fp4 {

namespace {

constexpr int kNestThreads = 256;

template <bool VEC>
__global__ __launch_bounds__(kNestThreads) void absmax_unnest_kernel(const uint8_t *__restrict__ q, const float *__restrict__ nested,
                                                                     const float *__restrict__ code256, float offset, int g_shift,
                                                                     int64_t nb, float *__restrict__ out) {
    __shared__ float s_code[256];
    const int tid = threadIdx.x;
    s_code[tid] = code256[tid];
    __syncthreads();
    const int64_t i0 = (int64_t(blockIdx.x) * kNestThreads + tid) * 4;
    if (i0 >= nb) return;
    if (VEC && i0 + 4 <= nb) {
        const uint32_t w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(q) + (i0 >> 2));
        const float m = nested[i0 >> g_shift];  // i0 % 4 == 0 and g >= 64: one group for the four
        const f32x4 r = {unnest_scale(s_code[w & 0xFFu], m, offset), unnest_scale(s_code[(w >> 8) & 0xFFu], m, offset),
                         unnest_scale(s_code[(w >> 16) & 0xFFu], m, offset), unnest_scale(s_code[w >> 24], m, offset)};
        __builtin_nontemporal_store(r, reinterpret_cast<f32x4 *>(out) + (i0 >> 2));
        return;
    }
    const int64_t end = i0 + 4 < nb ? i0 + 4 : nb;
    for (int64_t i = i0; i < end; ++i) out[i] = unnest_scale(s_code[q[i]], nested[i >> g_shift], offset);
}

__global__ __launch_bounds__(kNestThreads) void absmax_nest_kernel(const float *__restrict__ a, int64_t nb, float offset,
                                                                   const float *__restrict__ code256, int g_shift,
                                                                   uint8_t *__restrict__ out_q, float *__restrict__ out_nested) {
    __shared__ float s_code[256];
    __shared__ uint32_t s_max[kNestThreads / 64];
    const int tid = threadIdx.x;
    s_code[tid] = code256[tid];
    const int64_t base = int64_t(blockIdx.x) << g_shift;
    const int64_t left = nb - base;  // > 0: the grid is ceil(nb / g)
    const int count = left < (int64_t(1) << g_shift) ? int(left) : (1 << g_shift);
    // group maximum on the bit patterns of |v| (same order as the values; a NaN propagates)
    uint32_t mb = 0;
    for (int e = tid; e < count; e += kNestThreads) mb = max(mb, __builtin_bit_cast(uint32_t, a[base + e] - offset) & 0x7FFFFFFFu);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mb = max(mb, uint32_t(__shfl_xor(int(mb), d)));
    if ((tid & 63) == 0) s_max[tid >> 6] = mb;
    __syncthreads();  // table and wave maxima visible
    mb = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    const float m = __builtin_bit_cast(float, mb);
    if (tid == 0) out_nested[blockIdx.x] = m;
    const float inv = 1.0f / m;
    for (int e = tid; e < count; e += kNestThreads) {
        const float v = a[base + e] - offset;
        const float n = mb == 0 ? 0.0f : v * inv;
        int best = 0;
        double best_d = __builtin_fabs(double(s_code[0]) - double(n));
        for (int j = 1; j < 256; ++j) {
            const double d = __builtin_fabs(double(s_code[j]) - double(n));
            if (d < best_d) best_d = d, best = j;
        }
        out_q[base + e] = uint8_t(best);
    }
}

// g_shift of a nested blocksize the two kernels take (a power of two in 64..4096), else -1
int nested_shift(int nested_blocksize) {
    const int s = ilog2_exact(nested_blocksize);
    return s >= 6 && s <= 12 ? s : -1;
}

}  // namespace
}  // namespace fp4

extern "C" int fp4_hip_absmax_unnest(const uint8_t *absmax_u8, const float *nested_absmax, const float *code256, float offset,
                                     int nested_blocksize, int64_t nb, float *out_f32, void *stream) {
    using namespace fp4;
    if (nb < 0) {
        set_error("fp4_hip_absmax_unnest: nb=%lld (need nb >= 0)", (long long)nb);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    const int g_shift = nested_shift(nested_blocksize);
    if (g_shift < 0) {
        set_error("fp4_hip_absmax_unnest: nested_blocksize %d (need a power of two in 64..4096)", nested_blocksize);
        return FP4_ERR_UNSUPPORTED;
    }
    if (nb > (int64_t(1) << 31)) {
        set_error("fp4_hip_absmax_unnest: nb=%lld too large", (long long)nb);
        return FP4_ERR_UNSUPPORTED;
    }
    if (nb == 0) return FP4_OK;
    if (!absmax_u8 || !nested_absmax || !code256 || !out_f32) {
        set_error("fp4_hip_absmax_unnest: null pointer");
        return FP4_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t per_block = int64_t(kNestThreads) * 4;
    const dim3 grid((unsigned)((nb + per_block - 1) / per_block)), block(kNestThreads);
    const bool vec = (reinterpret_cast<uintptr_t>(absmax_u8) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_f32) & 15u) == 0;
    if (vec)
        hipLaunchKernelGGL((absmax_unnest_kernel<true>), grid, block, 0, s, absmax_u8, nested_absmax, code256, offset, g_shift, nb, out_f32);
    else
        hipLaunchKernelGGL((absmax_unnest_kernel<false>), grid, block, 0, s, absmax_u8, nested_absmax, code256, offset, g_shift, nb, out_f32);
    return check_launch("fp4_hip_absmax_unnest");
}

extern "C" int fp4_hip_absmax_nest(const float *absmax_f32, int64_t nb, float offset, const float *code256, int nested_blocksize,
                                   uint8_t *out_u8, float *out_nested_absmax, void *stream) {
    using namespace fp4;
    if (nb < 0) {
        set_error("fp4_hip_absmax_nest: nb=%lld (need nb >= 0)", (long long)nb);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    const int g_shift = nested_shift(nested_blocksize);
    if (g_shift < 0) {
        set_error("fp4_hip_absmax_nest: nested_blocksize %d (need a power of two in 64..4096)", nested_blocksize);
        return FP4_ERR_UNSUPPORTED;
    }
    if (nb > (int64_t(1) << 31)) {
        set_error("fp4_hip_absmax_nest: nb=%lld too large", (long long)nb);
        return FP4_ERR_UNSUPPORTED;
    }
    if (nb == 0) return FP4_OK;
    if (!absmax_f32 || !code256 || !out_u8 || !out_nested_absmax) {
        set_error("fp4_hip_absmax_nest: null pointer");
        return FP4_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t g = int64_t(1) << g_shift;
    const dim3 grid((unsigned)((nb + g - 1) / g)), block(kNestThreads);
    hipLaunchKernelGGL(absmax_nest_kernel, grid, block, 0, s, absmax_f32, nb, offset, code256, g_shift, out_u8, out_nested_absmax);
    return check_launch("fp4_hip_absmax_nest");
}
