// What the two NF4 matrix-core kernels (gemm_small_nf4.hip: 1..16 activation rows, gemm_wide_nf4.hip: up to 128) share on the device:
// the hi / lo decode and the gate|up store of the fused epilogues.  Their host side - the call descriptor, the form and dtype fan-out
// and the argument check - is nf4_call.h, shared with the GEMV, which needs none of what follows.
//
// The FP4 kernels build 12*|code| in 8 bits with v_perm; the 16 NF4 codes are arbitrary f32 values, exact in neither bf16 nor fp16,
// and T(code) alone misses the project's error bar (|err| <= 1e-5 * sum|x*w| beside the final rounding) by up to 31.6x in bf16 and
// 4.7x in fp16.  So every weight goes to the matrix cores TWICE:
//     hi = T(code),  lo = T(code - hi)        |hi + lo - code| <= 5.45e-6 |code| (bf16), 1.05e-7 |code| (fp16)
// as two instructions against the same activation fragment.  Both halves come from one 256-entry LDS table indexed by the packed
// BYTE: entry = { hi(high nibble) | hi(low nibble) << 16 , lo(high nibble) | lo(low nibble) << 16 }, so one ds_read_b64 per byte
// yields one fragment dword for each of the two instructions, in natural k order, and the other operand uses x as loaded.  The
// table is computed by the workgroup from the f32 codes with the kernel's own RNE conversions.
//
// fp16: most lo values are below fp16's smallest normal (6.1e-5).  Whether v_mfma_f32_16x16x32_f16 flushes subnormal inputs is not
// documented, so the kernels do not depend on it: the fp16 table holds lo * 2^24 (every non-zero entry normal, none above 4096),
// the lo instructions run into a tile of their own, and hi_tile + 2^-24 * lo_tile (exact scaling, one FMA per element) is formed
// before the block's absmax is applied.  bf16 has f32's exponent range: both instructions share one accumulator.
#pragma once

#include "mfma_common.h"
#include "nf4_call.h"

namespace fp4 {
namespace {

// lo is stored times 2^kLoShift: 24 for fp16 (see above), 0 for bf16
template <int DT>
constexpr int kLoShift = DT == FP4_DTYPE_F16 ? 24 : 0;

// (hi, lo) of one code in T: hi = RNE_T(code), lo = RNE_T((code - hi) * 2^kLoShift); code - hi is exact in f32
template <int DT>
__device__ __forceinline__ void split_code(int nibble, uint32_t &hi, uint32_t &lo) {
    const float c = nf4_lut_entry(nibble);
    hi = from_f32<DT>(c);
    const float rest = c - to_f32<DT>(uint16_t(hi));
    lo = from_f32<DT>(rest * float(1 << kLoShift<DT>));
}

// the byte table: thread tid = 0..255 writes the entry of packed byte tid (the caller synchronises the workgroup afterwards)
template <int DT>
__device__ __forceinline__ void fill_code_table(u32x2 *s_code, int tid) {
    if (tid < 256) {
        uint32_t h0, l0, h1, l1;
        split_code<DT>(tid >> 4, h0, l0);  // element 2i: the HIGH nibble
        split_code<DT>(tid & 15, h1, l1);
        s_code[tid] = u32x2{h0 | (h1 << 16), l0 | (l1 << 16)};
    }
}

// one packed dword q = 8 weights -> their hi and their lo fragment (four dwords each, natural k order)
struct HiLoFrag {
    u32x4 hi, lo;
};
__device__ __forceinline__ HiLoFrag decode8_hi_lo(const uint8_t *code, uint32_t q) {
    // byte d of q -> table entry at 8 * byte: dword d of the hi fragment and of the lo fragment
    const u32x2 e0 = *reinterpret_cast<const u32x2 *>(code + ((q << 3) & 0x7F8u));
    const u32x2 e1 = *reinterpret_cast<const u32x2 *>(code + ((q >> 5) & 0x7F8u));
    const u32x2 e2 = *reinterpret_cast<const u32x2 *>(code + ((q >> 13) & 0x7F8u));
    const u32x2 e3 = *reinterpret_cast<const u32x2 *>(code + ((q >> 21) & 0x7F8u));
    return HiLoFrag{{e0.x, e1.x, e2.x, e3.x}, {e0.y, e1.y, e2.y, e3.y}};
}

// hi_tile + 2^-kLoShift * lo_tile: the identity for bf16 (its lo products ran into `tile`), one FMA per element for fp16
template <int DT>
__device__ __forceinline__ f32x4 fold_lo(f32x4 tile, f32x4 tile_lo) {
    if constexpr (kLoShift<DT> != 0) {
        constexpr float kUnscale = 1.0f / float(1 << kLoShift<DT>);
        tile.x = __builtin_fmaf(tile_lo.x, kUnscale, tile.x);
        tile.y = __builtin_fmaf(tile_lo.y, kUnscale, tile.y);
        tile.z = __builtin_fmaf(tile_lo.z, kUnscale, tile.z);
        tile.w = __builtin_fmaf(tile_lo.w, kUnscale, tile.w);
    }
    return tile;
}

// The gate|up store of the FUSED kernels' final pass (kModeSiluMulPairs, M even): rows (row, row + 1) = (gate, up) of activation
// row n, both in range, with the finished f32 sums (t, u) -> the product into out[B][M / 2].  The LORA instantiations first add
// delta[n][row] = sum_j f32(lora_B[row][j]) * lora_t[n][j] to the gate's sum and the up row's delta to u.  Row is the kernel's own row
// type (int or int64_t).  Which thread stores and where the up row's partial sums lie stays with each kernel: it is its own layout.
// (The single-row store - the LORA delta, then store_small - stays in the kernels as well: routed through a helper it compiles to
// the same instructions on other registers in a few instantiations, and the kernels are kept instruction for instruction.)
template <int DT, bool LORA, typename Row>
__device__ __forceinline__ void store_nf4_pair(uint16_t *out, const uint16_t *bias, const uint16_t *residual, const uint16_t *lora_B,
                                               const float *lora_t, int R, int n, Row row, int M, float t, float u) {
    if constexpr (LORA) {
        t += lora_delta<DT>(lora_B + int64_t(row) * R, lora_t + n * R, R);
        u += lora_delta<DT>(lora_B + int64_t(row + 1) * R, lora_t + n * R, R);
    }
    store_small_silu_mul<DT>(out, bias, residual, n, (int)(row >> 1), M >> 1, t, u);
}

// The same for the MULTI instantiations: activation row n's adapter is read from ids[n]; with one, store_nf4_pair<LORA = true> on
// its slice of the stack, without one store_nf4_pair<LORA = false> - the bits of the single-adapter and of the plain fused kernel.
template <int DT, typename Row>
__device__ __forceinline__ void store_nf4_pair_multi(uint16_t *out, const uint16_t *bias, const uint16_t *residual, const uint16_t *B_stack,
                                                     const int *ids, int n_adapters, const float *lora_t, int R, int n, Row row, int M,
                                                     float t, float u) {
    if (const uint16_t *slice = lora_stack_slice(B_stack, ids, n_adapters, n, M, R))
        store_nf4_pair<DT, true>(out, bias, residual, slice, lora_t, R, n, row, M, t, u);
    else
        store_nf4_pair<DT, false>(out, bias, residual, nullptr, lora_t, R, n, row, M, t, u);
}

}  // namespace
}  // namespace fp4
