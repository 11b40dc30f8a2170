// Blockwise NF4 quantiser for gfx950 -- bitsandbytes' quantize_4bit(..., quant_type="nf4") restated (bitsandbytes is not on
// the build or test machines, so the rule below is the spec; tests/nf4_ref.py restates it in numpy):
//   absmax = max|w| over the block;  x = w * (1/absmax) in f32;  nibble = #{ i : x > T[i] } over the 15 f32 midpoints of
//   neighbouring NF4 codes (strict >);  even element -> high nibble.
// NaN fails every compare and becomes nibble 0, so an all-zero block (0 * inf) is 0x00 bytes, as bitsandbytes writes it, and
// inf / NaN / subnormal scales need no special case: the count is the rule itself for every f32 input.
//
// Ranking without 15 compares: the codes are asymmetric, so the FP4 quantiser's bucket table on |x| does not apply; instead
// x in [-1, 1] is cut into 32 buckets of width 1/16 (bucket = floor(16x + 16), clamped to 0..32; NaN -> 0), and since the
// narrowest gap between two thresholds is 0.08 > 1/16 every bucket holds at most one threshold.  A 33-entry LDS table gives,
// per bucket, {the threshold inside it (+inf if none), the number of thresholds below it}: nibble = below + (x > thr).
// The bucket index is rounded (one fma); an x that lands in a neighbouring bucket still gets the exact count as long as no
// threshold lies within that rounding error (< 2^-22) of a bucket edge - every one is >= 0.026/16 away (static_assert below).
//
// Memory structure: one-shot grid, 512-thread workgroups of 4096 contiguous elements (the largest blocksize), each lane owns 8
// consecutive elements (one 16-byte load of 16-bit input) and writes one packed dword; the block maximum is a butterfly over
// the bs/8 lanes of a block (DPP up to 16 lanes, cross-wave through LDS above 512 elements), as in quantize_fp4.hip.
#include "fp4_common.h"

namespace fp4 {

namespace {

constexpr int kNThreads = 512;
constexpr int64_t kNTile = int64_t(kNThreads) * 8;

// f32 midpoints of neighbouring NF4 codes (bitsandbytes' dQuantizeNF4 literals rounded to f32)
constexpr uint32_t kNf4ThrBits[15] = {0xBF591CD8u, 0xBF1C5270u, 0xBEEB8480u, 0xBEADEA76u, 0xBE703CECu, 0xBE0D38BCu, 0xBD3A7871u, 0x3D22FAFFu,
                                      0x3DF64862u, 0x3E5067E0u, 0x3E9582D4u, 0x3EC753F9u, 0x3F006D04u, 0x3F248DAFu, 0x3F5C89DAu};
constexpr bool thresholds_are_midpoints() {
    for (int i = 0; i < 15; ++i) {
        const double mid = (double(__builtin_bit_cast(float, kNf4Bits[i])) + double(__builtin_bit_cast(float, kNf4Bits[i + 1]))) / 2;
        if (__builtin_bit_cast(uint32_t, float(mid)) != kNf4ThrBits[i]) return false;
    }
    return true;
}
static_assert(thresholds_are_midpoints(), "T[i] must be the f32 rounding of the midpoint of code[i] and code[i+1]");

constexpr int kBuckets = 33;  // floor(16x + 16) for x in [-1, 1]
struct BucketTable {
    uint32_t thr[kBuckets];    // bits of the threshold inside the bucket, +inf if none
    uint32_t below[kBuckets];  // thresholds below the bucket's lower edge
};
constexpr BucketTable make_bucket_table() {
    BucketTable t{};
    for (int b = 0; b < kBuckets; ++b) {
        const double lo = -1.0 + b / 16.0, hi = lo + 1.0 / 16.0;
        t.thr[b] = 0x7F800000u;
        t.below[b] = 0;
        for (int i = 0; i < 15; ++i) {
            const double v = __builtin_bit_cast(float, kNf4ThrBits[i]);
            if (v < lo) ++t.below[b];
            else if (v < hi) t.thr[b] = kNf4ThrBits[i];
        }
    }
    return t;
}
constexpr bool one_threshold_per_bucket_far_from_edges() {
    for (int i = 0; i < 15; ++i) {
        const double f = (double(__builtin_bit_cast(float, kNf4ThrBits[i])) + 1.0) * 16.0;
        const double d = f - double(int64_t(f));
        if (d < 1e-3 || d > 1.0 - 1e-3) return false;
        if (i > 0 && int64_t(f) == int64_t((double(__builtin_bit_cast(float, kNf4ThrBits[i - 1])) + 1.0) * 16.0)) return false;
    }
    return true;
}
static_assert(one_threshold_per_bucket_far_from_edges(), "the bucket ranking needs at most one threshold per bucket, away from its edges");
__device__ const BucketTable kBucketTable = make_bucket_table();

template <int DT>
__device__ __forceinline__ void load8(const void *w, int64_t e0, int64_t n, bool full, float (&v)[8]) {
    if (full) {
        if constexpr (DT == FP4_DTYPE_F32) {
            const f32x4 lo = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(w) + e0 / 4);
            const f32x4 hi = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(w) + e0 / 4 + 1);
            v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
        } else {
            const u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(w) + e0 / 8);
            const uint32_t d[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = to_f32<DT>(uint16_t(d[i] & 0xFFFFu));
                v[2 * i + 1] = to_f32<DT>(uint16_t(d[i] >> 16));
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // the ragged last tile: element by element, zeros past n
        float t = 0.0f;
        if (e0 + i < n) {
            if constexpr (DT == FP4_DTYPE_F32)
                t = reinterpret_cast<const float *>(w)[e0 + i];
            else
                t = to_f32<DT>(reinterpret_cast<const uint16_t *>(w)[e0 + i]);
        }
        v[i] = t;
    }
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_umax_nf4(uint32_t v) {
    const uint32_t moved = uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, 0xF, 0xF, false));
    return v > moved ? v : moved;
}

template <int DT>
__global__ __launch_bounds__(kNThreads) void quantize_nf4_kernel(const void *__restrict__ w, uint8_t *__restrict__ packed,
                                                                 float *__restrict__ absmax, int64_t n, int bs_shift) {
    __shared__ uint32_t s_wave_max[kNThreads / 64];
    __shared__ u32x2 s_tab[kBuckets];
    const int tid = threadIdx.x;
    // table entry first: vector-memory results return in issue order, so its latency hides under the weight load's
    const int ti = tid < kBuckets ? tid : 0;
    const u32x2 entry = {kBucketTable.thr[ti], kBucketTable.below[ti]};
    const int64_t e0 = int64_t(blockIdx.x) * kNTile + tid * 8;
    const bool full_tile = int64_t(blockIdx.x + 1) * kNTile <= n;  // uniform across the workgroup
    float v[8];
    load8<DT>(w, e0, n, full_tile, v);
    if (tid < kBuckets) s_tab[tid] = entry;

    // block maximum on the bit patterns of |w| (same order as the values; a NaN weight propagates into absmax)
    uint32_t mb = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) mb = max(mb, __builtin_bit_cast(uint32_t, v[i]) & 0x7FFFFFFFu);
    const int lanes_per_block = 1 << (bs_shift - 3);
    mb = dpp_umax_nf4<0xB1>(mb);                                      // quad_perm [1,0,3,2]
    mb = dpp_umax_nf4<0x4E>(mb);                                      // quad_perm [2,3,0,1]
    if (lanes_per_block >= 8) mb = dpp_umax_nf4<0x141>(mb);           // row_half_mirror
    if (lanes_per_block >= 16) mb = dpp_umax_nf4<0x140>(mb);          // row_mirror
    if (lanes_per_block >= 32) mb = max(mb, uint32_t(__shfl_xor(int(mb), 16)));
    if (lanes_per_block >= 64) mb = max(mb, uint32_t(__shfl_xor(int(mb), 32)));
    if (lanes_per_block > 64) {
        if ((tid & 63) == 0) s_wave_max[tid >> 6] = mb;
    }
    __syncthreads();  // table (and the wave maxima) visible
    if (lanes_per_block > 64) {
        const int waves_per_block = lanes_per_block >> 6;
        const int first = ((tid >> 6) / waves_per_block) * waves_per_block;
        for (int i = 0; i < waves_per_block; ++i) mb = max(mb, s_wave_max[first + i]);
    }
    if (e0 >= n) return;
    const float m = __builtin_bit_cast(float, mb);
    if ((tid & (lanes_per_block - 1)) == 0) __builtin_nontemporal_store(m, absmax + (e0 >> bs_shift));

    const float inv = 1.0f / m;
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = v[i] * inv;  // -ffp-contract=off (build.py): rounded before the bucket fma
        const float f = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(x, 16.0f, 16.0f), 0.0f), 32.0f);  // NaN -> 0
        const u32x2 t = s_tab[int(f)];
        const uint32_t nib = t.y + (x > __builtin_bit_cast(float, t.x) ? 1u : 0u);
        word |= nib << (8 * (i >> 1) + ((i & 1) ? 0 : 4));
    }
    if (e0 + 8 <= n) {
        __builtin_nontemporal_store(word, reinterpret_cast<uint32_t *>(packed) + e0 / 8);
    } else {
        const int nbytes = int((n - e0 + 1) / 2);
        for (int b = 0; b < nbytes; ++b) packed[e0 / 2 + b] = uint8_t(word >> (8 * b));
    }
}

}  // namespace
}  // namespace fp4

extern "C" int fp4_hip_quantize_blockwise_nf4(const void *w, int w_dtype, uint8_t *packed, float *absmax, int64_t n, int blocksize,
                                              void *stream) {
    using namespace fp4;
    const int bs_shift = ilog2_exact(blocksize);
    if (n < 0) {
        set_error("fp4_hip_quantize_blockwise_nf4: n=%lld", (long long)n);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (bs_shift < 5 || bs_shift > 12) {
        set_error("fp4_hip_quantize_blockwise_nf4: blocksize %d (need a power of two in 32..4096)", blocksize);
        return FP4_ERR_UNSUPPORTED;
    }
    if (w_dtype != FP4_DTYPE_F16 && w_dtype != FP4_DTYPE_BF16 && w_dtype != FP4_DTYPE_F32) {
        set_error("fp4_hip_quantize_blockwise_nf4: unsupported dtype %d", w_dtype);
        return FP4_ERR_UNSUPPORTED;
    }
    if (n == 0) return FP4_OK;
    if (!w || !packed || !absmax) {
        set_error("fp4_hip_quantize_blockwise_nf4: null pointer");
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if ((reinterpret_cast<uintptr_t>(w) & 15u) || (reinterpret_cast<uintptr_t>(packed) & 3u)) {
        set_error("fp4_hip_quantize_blockwise_nf4: w must be 16-byte and packed 4-byte aligned");
        return FP4_ERR_UNSUPPORTED;
    }
    if ((n + kNTile - 1) / kNTile >= (int64_t(1) << 23)) {  // grid * 512 threads must stay below 2^32
        set_error("fp4_hip_quantize_blockwise_nf4: n=%lld too large", (long long)n);
        return FP4_ERR_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + kNTile - 1) / kNTile)), block(kNThreads);
    switch (w_dtype) {
        case FP4_DTYPE_F16:
            hipLaunchKernelGGL((quantize_nf4_kernel<FP4_DTYPE_F16>), grid, block, 0, s, w, packed, absmax, n, bs_shift);
            break;
        case FP4_DTYPE_BF16:
            hipLaunchKernelGGL((quantize_nf4_kernel<FP4_DTYPE_BF16>), grid, block, 0, s, w, packed, absmax, n, bs_shift);
            break;
        default:
            hipLaunchKernelGGL((quantize_nf4_kernel<FP4_DTYPE_F32>), grid, block, 0, s, w, packed, absmax, n, bs_shift);
            break;
    }
    return check_launch("fp4_hip_quantize_blockwise_nf4");
}
