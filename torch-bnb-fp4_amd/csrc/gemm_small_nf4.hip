// Small-batch NF4 product for gfx950 (MI355X): 1..16 activation rows against one NF4 weight on the matrix cores,
//     out[b][r] = T( sum_k x[b][k] * code[nib(r,k)] * absmax[(r*K+k)/64] + bias[r] )
// The tile scheme is gemm16_mfma_kernel's (gemm_small_fp4.hip): 8-wave workgroup per 16-row tile of W, the waves split K,
// row-contiguous 16-byte weight loads staged through a wave-private LDS image (wave_image.h: one definition of the weight and the x
// image for the FP4 and the NF4 kernels), scales re-read from it as broadcasts, loads one pass ahead,
// v_mfma_f32_16x16x32_{bf16,f16} with one instruction never straddling two scales, partial tiles meeting in LDS.
//
// What differs is the decode: every weight goes to the matrix cores twice, as hi = T(code) and lo = T(code - hi) from one 256-entry
// LDS table indexed by the packed byte.  nf4_mfma.h has the decode, the reason for it and fp16's 2^24 rule; here the weight is the
// A operand and the B side uses x as loaded.
//
// Fused decode epilogues (fp4_hip_gemm_fused_nf4, 1..16 rows with K % 512 == 0): the FUSED instantiations take a residual and the
// `mode` of gemm_small_fp4.hip.  The final pass over the LDS partials has one thread per (activation row, weight row); for the
// gate|up epilogue the thread of an even weight row also sums its odd neighbour's partials (tid + 1) and stores the pair, the odd
// thread stores nothing (store_nf4_pair, nf4_mfma.h).  A compile-time choice: the plain entry point keeps its instantiations
// instruction for instruction.
//
// LoRA adapter term (fp4_hip_gemm_lora_nf4, 2..16 rows with K % 512 == 0): the LORA instantiations (always FUSED) add
// delta[n][row] = sum_j f32(lora_B[row][j]) * lora_t[n][j] (lora_nf4.h) to the thread's finished f32 sum ahead of the epilogue, and
// to the up row's likewise; lora_t = s * A x is lora_down_kernel's f32 output.
//
// Several adapters per batch (fp4_hip_gemm_lora_multi_nf4): the MULTI instantiations (always LORA) take a stack of B arrays and read
// the adapter of activation row n from lora_ids[n] on the device, once per (n) a thread owns; a row without an adapter is stored as
// the FUSED instantiation stores it.
//
// Nested (double-quantised) absmax (fp4_hip_gemm_nested_nf4 / fp4_hip_gemm_lora_nested_nf4): the NESTED instantiations (FUSED, or
// FUSED + LORA) fetch the block's uint8 code and its group's f32 scale where the f32 scale was fetched, one pass ahead, and write
// unnest_scale(table[code], group, offset) (nested_absmax.h: a multiply, then an add) into the LDS image.  Everything that reads the
// image is unchanged, so the result equals the FUSED / LORA instantiation on the expanded absmax bit for bit.
//
// Host side: fp4_hip_gemm_small_nf4 (the plain form) and gemm_small_nf4_launch (any form, for the entry points of gemm_wide_nf4.hip)
// take an Nf4Call (nf4_call.h); dispatch_nf4_mfma goes from its form and dtype (with_nf4_form, with_dtype) to the geometry to the
// launch (launch_nf4_mfma, the only place that spells the kernel's flag order).
#include "launchers.h"
#include "nested_absmax.h"
#include "nf4_mfma.h"
#include "wave_image.h"

namespace fp4 {

namespace {

// Workgroup = 8 waves = one 16-row tile of W; wave w owns quant blocks (p*8 + w)*NBW.. of pass p.  Lane (r = l & 15, kb = l >> 4)
// supplies, per 64-weight block, the 8 packed bytes [8kb, 8kb + 8) of row r: k-sets {16kb + 8t + j}, t = 0, 1, each fed as hi and as
// lo - four matrix instructions per block and tile.  The B operand is x[n = l & 15][64b + 16kb + 8t + j], from a wave-private LDS
// image for <= XS rows (XS in {4, 8}), else straight from L2.  Both images are wave_image.h's, as in the FP4 kernel.
// FUSED = false: `residual` and `mode` are ignored.  FUSED = true: store_small's residual add, or with kModeSiluMulPairs (M even) the
// gate|up product into out[B][M / 2].  `residual` may alias `out` (each element is read, then written, by one thread).
// MULTI = true (with LORA): lora_B is a stack of n_adapters arrays T[M][R] and lora_ids[n] names activation row n's adapter; a row
// whose id names none takes the FUSED store as it is (the add is skipped, not done with zero).
// NESTED = true (with FUSED, without MULTI): `absmax` points at uint8 codes, one per block; the scale of block i is
// unnest_scale(nested_code[code[i]], nested_absmax[i >> 8], nested_offset).
template <int DT, int NBW, int XS, bool FUSED, bool LORA = false, bool MULTI = false, bool NESTED = false>
__global__ __launch_bounds__(512) void gemm_nf4_mfma_kernel(const uint16_t *__restrict__ x, const uint8_t *__restrict__ W,
                                                            const float *__restrict__ absmax, const uint16_t *__restrict__ bias,
                                                            uint16_t *out, int B, int M, int K, const uint16_t *residual, int mode,
                                                            const uint16_t *lora_B, const float *lora_t, int R, const int *lora_ids,
                                                            int n_adapters,  // new arguments last
                                                            const float *nested_absmax, const float *nested_code, float nested_offset) {
    static_assert(!LORA || FUSED, "the adapter term comes with the fused epilogues");
    static_assert(!MULTI || LORA, "the adapter stack comes with the adapter term");
    static_assert(!NESTED || (FUSED && !MULTI), "nested absmax comes with the fused epilogues and without the adapter stack");
    using WImg = WeightImage<NBW>;
    using XImg = XImage<NBW, XS>;
    constexpr int kWImageBytes = 8 * WImg::kBytes;
    constexpr int kImageBytes = kWImageBytes + 8 * XImg::kBytes;
    constexpr int kPartBytes = 8 * 256 * 4;
    // the cross-wave partial sums reuse the images' storage after the K loop; the code table has storage of its own
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[kImageBytes > kPartBytes ? kImageBytes : kPartBytes];
    __shared__ __attribute__((aligned(16))) u32x2 s_code[256];
    __shared__ float s_ncode[NESTED ? 256 : 1];
    uint8_t *s_w = s_raw;
    uint8_t *s_x = s_raw + kWImageBytes;
    float (*s_part)[256] = reinterpret_cast<float (*)[256]>(s_raw);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 15, kb = lane >> 4;
    const int row0 = blockIdx.x * 16;
    const int nblk = K >> 6;
    const int passes = nblk / (8 * NBW);
    const int64_t n_b = r < B ? r : B - 1;  // clamped rows / batch entries are computed, never stored
    const u32x4 *x4 = reinterpret_cast<const u32x4 *>(x);

    // 16 rows x NBW scales over 64 lanes (with NBW < 4 the upper lanes repeat rows: same address, same value)
    const int srow = (lane / NBW) & 15, sj0 = lane % NBW;
    u32x4 xstage[XImg::kUnits];
    u32x4 wstage[WImg::kInstr];
    float amstage;
    [[maybe_unused]] uint32_t aqstage;  // NESTED: the block's code; amstage holds its group's scale
    auto issue_staged = [&](int pass) {  // x first (L2), then the weight stream (HBM), then the scales; all branch-free
        const int b0 = (pass * 8 + wave) * NBW;
        if constexpr (XS > 0) {
#pragma unroll
            for (int i = 0; i < XImg::kUnits; ++i) {
                const int n = XImg::unit_row(i, lane), c16 = XImg::unit_col(i, lane);
                const int64_t nn = n < B ? n : B - 1;
                xstage[i] = x4[((nn * K + 64 * b0) >> 3) + c16];
            }
        }
#pragma unroll
        for (int i = 0; i < WImg::kInstr; ++i) wstage[i] = __builtin_nontemporal_load(WImg::fetch_unit(W, i, lane, row0, M, K, b0));
        const int64_t row = row0 + srow < M ? row0 + srow : M - 1;
        if constexpr (NESTED) {
            const int64_t blk = row * nblk + b0 + sj0;
            aqstage = reinterpret_cast<const uint8_t *>(absmax)[blk];
            amstage = nested_absmax[blk >> kNestedGemvShift];
        } else {
            amstage = absmax[row * nblk + b0 + sj0];
        }
    };
    issue_staged(0);

    // the byte table, once per workgroup, while the first pass's loads fly
    fill_code_table<DT>(s_code, tid);
    if constexpr (NESTED) {
        if (tid < 256) s_ncode[tid] = nested_code[tid];
    }
    __syncthreads();
    const uint8_t *code = reinterpret_cast<const uint8_t *>(s_code);

    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int p = 0; p < passes; ++p) {
        u32x4 xr[XS ? 1 : NBW][2];
        if constexpr (XS == 0) {
            const int b0 = (p * 8 + wave) * NBW;
#pragma unroll
            for (int j = 0; j < NBW; ++j) {
                const int64_t e = n_b * K + 64 * (b0 + j) + 16 * kb;
                xr[j][0] = x4[e >> 3];
                xr[j][1] = x4[(e >> 3) + 1];
            }
        }
        if (p > 0) __builtin_amdgcn_wave_barrier();  // the previous pass's reads are done before the image is rewritten
        uint8_t *img = WImg::at(s_w, wave);
#pragma unroll
        for (int i = 0; i < WImg::kInstr; ++i) {
            const int rr = WImg::fetch_row(i, lane);
            if (WImg::inside(rr)) *WImg::unit(img, rr, lane) = wstage[i];
        }
        if constexpr (NESTED)
            WImg::scales(img, srow)[sj0] = unnest_scale(s_ncode[aqstage], amstage, nested_offset);
        else
            WImg::scales(img, srow)[sj0] = amstage;
        if constexpr (XS > 0) {
#pragma unroll
            for (int i = 0; i < XImg::kUnits; ++i)
                *XImg::unit(XImg::at(s_x, wave), XImg::unit_row(i, lane), XImg::unit_col(i, lane)) = xstage[i];  // natural k order
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (p + 1 < passes) issue_staged(p + 1);  // uniform; flies while this pass is decoded and multiplied

        u32x2 wq[NBW];
        float am[4][NBW];
        WImg::read_frags(img, r, kb, wq);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float *src = WImg::scales(img, kb * 4 + g);
            if constexpr (NBW % 4 == 0) {
#pragma unroll
                for (int j = 0; j < NBW; j += 4) {
                    const f32x4 v = reinterpret_cast<const f32x4 *>(src)[j >> 2];
                    am[g][j] = v.x, am[g][j + 1] = v.y, am[g][j + 2] = v.z, am[g][j + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NBW; ++j) am[g][j] = src[j];
            }
        }
#pragma unroll
        for (int j = 0; j < NBW; ++j) {
            f32x4 tile = {0.0f, 0.0f, 0.0f, 0.0f}, tile_lo = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                u32x4 bfrag;
                if constexpr (XS > 0)
                    bfrag = *XImg::frag(XImg::at(s_x, wave), r, j, kb, t);
                else
                    bfrag = xr[j][t];
                const uint32_t q = t == 0 ? wq[j].x : wq[j].y;
                const HiLoFrag w = decode8_hi_lo(code, q);
                tile = mfma16<DT>(w.hi, bfrag, tile);
                if constexpr (kLoShift<DT> == 0)
                    tile = mfma16<DT>(w.lo, bfrag, tile);
                else
                    tile_lo = mfma16<DT>(w.lo, bfrag, tile_lo);
            }
            tile = fold_lo<DT>(tile, tile_lo);
            acc.x = __builtin_fmaf(tile.x, am[0][j], acc.x);
            acc.y = __builtin_fmaf(tile.y, am[1][j], acc.y);
            acc.z = __builtin_fmaf(tile.z, am[2][j], acc.z);
            acc.w = __builtin_fmaf(tile.w, am[3][j], acc.w);
        }
    }
    __syncthreads();  // every wave is done with its image before the partials overwrite the storage
    *reinterpret_cast<f32x4 *>(&s_part[wave][lane * 4]) = acc;
    __syncthreads();
    if (tid < 256) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) t += s_part[w][tid];
        const int l = tid >> 2, reg = tid & 3;  // D layout: col = l & 15 (activation row), row = (l >> 4) * 4 + reg (weight row)
        const int n = l & 15, row = row0 + (l >> 4) * 4 + reg;
        if constexpr (FUSED) {
            if (mode & kModeSiluMulPairs) {
                if (!(reg & 1)) {  // row0 is a multiple of 16: an even reg is an even weight row (gate), tid + 1 its up row
                    float u = 0.0f;
#pragma unroll
                    for (int w = 0; w < 8; ++w) u += s_part[w][tid + 1];
                    if constexpr (MULTI) {
                        if (row < M && n < B) store_nf4_pair_multi<DT>(out, bias, residual, lora_B, lora_ids, n_adapters, lora_t, R, n, row, M, t, u);
                    } else {
                        if (row < M && n < B) store_nf4_pair<DT, LORA>(out, bias, residual, lora_B, lora_t, R, n, row, M, t, u);
                    }
                }
            } else if (row < M && n < B) {
                if constexpr (MULTI) {
                    if (const uint16_t *slice = lora_stack_slice(lora_B, lora_ids, n_adapters, n, M, R))
                        t += lora_delta<DT>(slice + int64_t(row) * R, lora_t + n * R, R);
                } else if constexpr (LORA) {
                    t += lora_delta<DT>(lora_B + int64_t(row) * R, lora_t + n * R, R);
                }
                store_small<DT>(out, bias, residual, n, row, M, t);
            }
        } else {
            if (row < M && n < B) store_small<DT>(out, bias, nullptr, n, row, M, t);
        }
    }
}

// Form: the Nf4Form of the call (nf4_call.h).  The kernel's own flag order is spelt here and nowhere else on the host.
template <int DT, int NBW, int XS, typename Form>
void launch_nf4_mfma(const Nf4Call &a) {
    hipLaunchKernelGGL((gemm_nf4_mfma_kernel<DT, NBW, XS, Form::fused, Form::lora, Form::multi, Form::nested>), dim3((unsigned)((a.M + 15) / 16)),
                       dim3(512), 0, a.stream, static_cast<const uint16_t *>(a.x), a.W, static_cast<const float *>(a.scales),
                       static_cast<const uint16_t *>(a.bias), static_cast<uint16_t *>(a.out), (int)a.B, (int)a.M, (int)a.K,
                       static_cast<const uint16_t *>(a.residual), a.mode, static_cast<const uint16_t *>(a.adapter.B), a.adapter.t,
                       (int)a.adapter.R, a.adapter.ids, (int)a.adapter.n_adapters, a.nested_stats.group, a.nested_stats.table,
                       a.nested_stats.offset);
}

template <int DT, typename Form>
void dispatch_nf4_mfma_shape(const Nf4Call &a) {
    const int B = (int)a.B, M = (int)a.M, K = (int)a.K;
    const int units = K / 512;  // quant blocks per wave over the whole K
    const int blocks = (M + 15) / 16;
    // the FP4 kernel's rules: at most 4 blocks per wave and pass; x staged per wave in LDS always for <= 4 rows, for 5..8 rows only
    // while the grid is a single round anyway (the larger image leaves fewer workgroups per CU)
    if (units % 4 == 0) {
        if (B <= 4) return launch_nf4_mfma<DT, 4, 4, Form>(a);
        if (B <= 8 && blocks <= device_cu_count()) return launch_nf4_mfma<DT, 4, 8, Form>(a);
        return launch_nf4_mfma<DT, 4, 0, Form>(a);
    }
    if (units % 2 == 0) return launch_nf4_mfma<DT, 2, 0, Form>(a);
    return launch_nf4_mfma<DT, 1, 0, Form>(a);
}

// a validated call of any form -> its kernel
void dispatch_nf4_mfma(const Nf4Call &a) {
    with_nf4_form(a, [&](auto form) {
        with_dtype(a.dtype, [&](auto dt) { dispatch_nf4_mfma_shape<decltype(dt)::value, decltype(form)>(a); });
    });
}

}  // namespace

// for the entry points of gemm_wide_nf4.hip, which have validated the call - operands, adapter and statistics: 1..16 rows,
// K % 512 == 0, fp16 / bf16, M even for the gate|up epilogue.  Launches only.
void gemm_small_nf4_launch(const Nf4Call &call) { dispatch_nf4_mfma(call); }

}  // namespace fp4

extern "C" int fp4_hip_gemm_small_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, void *out,
                                      int64_t B, int64_t M, int64_t K, int blocksize, int dtype, void *stream) {
    using namespace fp4;
    const char *name = "fp4_hip_gemm_small_nf4";
    const Nf4Call c{.x = x, .W = packed, .scales = absmax, .bias = bias, .out = out, .B = B, .M = M, .K = K, .blocksize = blocksize,
                    .dtype = dtype, .stream = static_cast<hipStream_t>(stream)};
    if (const int rc = nf4_check_args(name, c, 16, 512)) return rc;
    if (M == 0 || B == 0) return FP4_OK;
    dispatch_nf4_mfma(c);
    return check_launch(name);
}
