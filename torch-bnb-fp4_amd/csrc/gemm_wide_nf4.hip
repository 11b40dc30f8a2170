// Wide-batch NF4 product for gfx950 (MI355X): up to 128 activation rows against one NF4 weight on the matrix cores, one pass over
// the packed weight per at most 64 rows,
//     out[b][r] = T( sum_k x[b][k] * code[nib(r,k)] * absmax[(r*K+k)/64] + bias[r] )
// f32 accumulation, bias added in f32, one rounding to T.
//
// Operand roles are gemm_wide_fp4.hip's: x is the A operand, the weight the B operand of v_mfma_f32_16x16x32_{bf16,f16}, so a
// lane's four accumulators of a tile belong to ONE weight row (D column = lane & 15) and four activation rows, and the block's
// absmax is one scalar per lane and 64-weight block.  No instruction straddles two scales.
//
// The decode is gemm_small_nf4.hip's, shared through nf4_mfma.h (which says why): every weight goes to the matrix cores twice,
//     hi = T(code),  lo = T(code - hi),
// both halves from one 256-entry LDS table indexed by the packed BYTE (one ds_read_b64 per byte = one fragment dword of each half,
// natural k order).  A decoded fragment pair is used for all NT column tiles of x:
// 8 table reads per lane, weight row and block feed 4 * NT matrix instructions (the 2..16-row kernel: 8 reads for 4).
// fp16 keeps the rule that no subnormal matrix input is relied on: the lo products run into a tile of their own.
//
// Work split: a workgroup of 8 waves owns RT 16-row tiles of W (RT in {1, 2}, chosen by M) and all NT <= 4 column tiles; the waves
// split K in units of NBW blocks (unit u = pass * 8 + wave; NBW = 4 where K % 256 == 0, else 1; a ragged last pass leaves the
// upper waves idle).  The weight unit and its scales are fetched one pass ahead with row-contiguous 16-byte loads and staged
// through a wave-private LDS image; x fragments come straight from L2, one block ahead, and are shared by the RT row tiles.  The
// row tiles are looped INSIDE a block so that only tile[NT] (fp16: two of them) is live beside acc[RT][NT].  The eight waves'
// partial tiles meet in LDS and are added in a fixed order: deterministic, no atomics, no workspace.
//
// Fused decode epilogues (fp4_hip_gemm_fused_nf4): the FUSED instantiations take a residual and the `mode` of gemm_wide_fp4.hip.  The
// final pass has one thread per (tile, activation row, weight row); for the gate|up epilogue the thread of an even weight row also
// sums its odd neighbour's partials (wr + 1 = src + 4, as wide_epilogue of gemm_wide_fp4.hip does) and stores the pair, odd rows
// store nothing (store_nf4_pair, nf4_mfma.h); row tiles are 16 rows and row0 is even, so a pair never straddles a tile.  A compile-time
// choice: the plain entry point keeps its instantiations instruction for instruction.
//
// LoRA adapter term (fp4_hip_gemm_lora_nf4, 1..64 rows): the LORA instantiations (always FUSED) add
// delta[n][row] = sum_j f32(lora_B[row][j]) * lora_t[n][j] (lora_nf4.h) to the thread's finished f32 sum ahead of the epilogue, and
// to the up row's likewise; lora_t = s * A x is lora_down_kernel's f32 output.
//
// Several adapters per batch (fp4_hip_gemm_lora_multi_nf4, 1..64 rows): the MULTI instantiations (always LORA) take a stack of B
// arrays and read the adapter of activation row n from lora_ids[n] on the device, once per (n) of the store loop; a row without an
// adapter is stored as the FUSED instantiation stores it.
//
// Nested (double-quantised) absmax (fp4_hip_gemm_nested_nf4 / fp4_hip_gemm_lora_nested_nf4): the NESTED instantiations (FUSED, or
// FUSED + LORA) fetch the block's uint8 code and its group's f32 scale where the f32 scale was fetched, one pass ahead, and write
// unnest_scale(table[code], group, offset) (nested_absmax.h: a multiply, then an add) into the LDS image.  Everything that reads the
// image is unchanged, so the result equals the FUSED / LORA instantiation on the expanded absmax bit for bit.
//
// Host side: the six extern "C" entry points each fill an Nf4Call (nf4_call.h) and share one path, gemm_wide_nf4_entry(name, call):
// one check, one adapter check, one hand-over to the 2..16-row kernel (gemm_small_nf4_launch), one chunk loop.  dispatch_wide_nf4 goes
// from the call's form and dtype (with_nf4_form, with_dtype) to the tile counts to the launch (launch_wide_nf4, the only place that
// spells the kernel's flag order).
#include <atomic>

#include "launchers.h"
#include "nested_absmax.h"
#include "nf4_mfma.h"
#include "wave_image.h"

namespace fp4 {

namespace {

// Lane (r = l & 15, kb = l >> 4).  Instruction t = 0, 1 of a block takes k = 32t .. 32t + 31 in natural order: the B operand is the
// packed dword [16t + 4kb, 16t + 4kb + 4) of weight row r (k = 32t + 8kb + j), the A operand x[16nt + r][64b + 32t + 8kb + j], so
// one x load instruction reads 64 contiguous bytes per activation row.  D: lane holds out[16nt + 4kb + reg][row0 + 16rt + r].
// Weight image (per wave): WeightImage<NBW, 16 * RT> of wave_image.h, the RT row tiles fetched and addressed as one image.
// FUSED = false: `residual` and `mode` are ignored.  FUSED = true: store_small's residual add, or with kModeSiluMulPairs (M even) the
// gate|up product into out[B][M / 2].  `residual` may alias `out` (each element is read, then written, by one thread).
// MULTI = true (with LORA): lora_B is a stack of n_adapters arrays T[M][R] and lora_ids[n] names activation row n's adapter; a row
// whose id names none takes the FUSED store as it is (the add is skipped, not done with zero).
// NESTED = true (with FUSED, without MULTI): `absmax` points at uint8 codes, one per block; the scale of block i is
// unnest_scale(nested_code[code[i]], nested_absmax[i >> 8], nested_offset).
template <int DT, int NT, int RT, int NBW, bool FUSED, bool LORA = false, bool MULTI = false, bool NESTED = false>
__global__ __launch_bounds__(512) void gemm_wide_nf4_kernel(const uint16_t *__restrict__ x, const uint8_t *__restrict__ W,
                                                            const float *__restrict__ absmax, const uint16_t *__restrict__ bias,
                                                            uint16_t *out, int B, int M, int K, const uint16_t *residual, int mode,
                                                            const uint16_t *lora_B, const float *lora_t, int R, const int *lora_ids,
                                                            int n_adapters,  // new arguments last
                                                            const float *nested_absmax, const float *nested_code, float nested_offset) {
    static_assert(!LORA || FUSED, "the adapter term comes with the fused epilogues");
    static_assert(!MULTI || LORA, "the adapter stack comes with the adapter term");
    static_assert(!NESTED || (FUSED && !MULTI), "nested absmax comes with the fused epilogues and without the adapter stack");
    constexpr int kRows = 16 * RT;
    using WImg = WeightImage<NBW, kRows>;
    constexpr int kImageBytes = 8 * WImg::kBytes;
    constexpr int kTiles = RT * NT;
    constexpr int kPartBytes = 4 * kTiles * 256 * 4;  // four slots: see the reduction below
    // the cross-wave partial sums reuse the images' storage after the K loop; the code table has storage of its own
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[kImageBytes > kPartBytes ? kImageBytes : kPartBytes];
    __shared__ __attribute__((aligned(16))) u32x2 s_code[256];
    __shared__ float s_ncode[NESTED ? 256 : 1];
    float (*s_part)[kTiles * 256] = reinterpret_cast<float (*)[kTiles * 256]>(s_raw);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 15, kb = lane >> 4;
    const int64_t row0 = int64_t(blockIdx.x) * kRows;
    const int nblk = K >> 6;
    const int nunits = nblk / NBW;
    const int passes = (nunits + 7) >> 3;
    const u32x4 *x4 = reinterpret_cast<const u32x4 *>(x);

    constexpr int kScaleInstr = (kRows * NBW + 63) / 64;  // with fewer than 64 scales the upper lanes repeat rows: same address, same value
    u32x4 wstage[WImg::kInstr];
    float amstage[kScaleInstr];
    [[maybe_unused]] uint32_t aqstage[NESTED ? kScaleInstr : 1];  // NESTED: the block's code; amstage holds its group's scale
    auto issue_staged = [&](int pass) {  // the weight stream (HBM), then the scales; branch-free, a unit past the end is clamped
        const int u = pass * 8 + wave;
        const int b0 = (u < nunits ? u : nunits - 1) * NBW;
#pragma unroll
        for (int i = 0; i < WImg::kInstr; ++i) wstage[i] = __builtin_nontemporal_load(WImg::fetch_unit(W, i, lane, row0, M, K, b0));
#pragma unroll
        for (int i = 0; i < kScaleInstr; ++i) {
            const int idx = i * 64 + lane, rr = (idx / NBW) % kRows;
            const int64_t row = row0 + rr < M ? row0 + rr : int64_t(M) - 1;
            if constexpr (NESTED) {
                const int64_t blk = row * nblk + b0 + idx % NBW;
                aqstage[i] = reinterpret_cast<const uint8_t *>(absmax)[blk];
                amstage[i] = nested_absmax[blk >> kNestedGemvShift];
            } else {
                amstage[i] = absmax[row * nblk + b0 + idx % NBW];
            }
        }
    };
    // the x fragments of one block: rows past B are clamped (computed, never stored)
    int64_t xrow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = 16 * nt + r;
        xrow[nt] = int64_t(n < B ? n : B - 1) * K + 8 * kb;
    }
    auto load_x = [&](u32x4 (&xr)[NT][2], int blk) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t e = (xrow[nt] + 64 * int64_t(blk)) >> 3;
            xr[nt][0] = x4[e];
            xr[nt][1] = x4[e + 4];
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
    uint8_t *img = WImg::at(s_raw, wave);

    f32x4 acc[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int p = 0; p < passes; ++p) {
        const int u = p * 8 + wave;
        const bool active = u < nunits;  // wave-uniform
        const int b0 = (active ? u : nunits - 1) * NBW;
        u32x4 xcur[NT][2];
        load_x(xcur, b0);
        if (p > 0) __builtin_amdgcn_wave_barrier();  // the previous pass's reads are done before the image is rewritten
#pragma unroll
        for (int i = 0; i < WImg::kInstr; ++i) {
            const int rr = WImg::fetch_row(i, lane);
            if (WImg::inside(rr)) *WImg::unit(img, rr, lane) = wstage[i];
        }
#pragma unroll
        for (int i = 0; i < kScaleInstr; ++i) {
            const int idx = i * 64 + lane, rr = (idx / NBW) % kRows;
            if constexpr (NESTED)
                WImg::scales(img, rr)[idx % NBW] = unnest_scale(s_ncode[aqstage[i]], amstage[i], nested_offset);
            else
                WImg::scales(img, rr)[idx % NBW] = amstage[i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (p + 1 < passes) issue_staged(p + 1);  // uniform; flies while this pass is decoded and multiplied
        if (!active) continue;

#pragma unroll 1
        for (int j = 0; j < NBW; ++j) {
            u32x4 xnext[NT][2];
            if (j + 1 < NBW) load_x(xnext, b0 + j + 1);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                uint8_t *wrow = WImg::row(img, 16 * rt + r);
                const uint32_t wq[2] = {*WImg::frag4(wrow, j, kb, 0), *WImg::frag4(wrow, j, kb, 1)};
                const float am = WImg::row_scales(wrow)[j];
                f32x4 tile[NT], tile_lo[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) tile[nt] = tile_lo[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const HiLoFrag w = decode8_hi_lo(code, wq[t]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        tile[nt] = mfma16<DT>(xcur[nt][t], w.hi, tile[nt]);
                        if constexpr (kLoShift<DT> == 0)
                            tile[nt] = mfma16<DT>(xcur[nt][t], w.lo, tile[nt]);
                        else
                            tile_lo[nt] = mfma16<DT>(xcur[nt][t], w.lo, tile_lo[nt]);
                    }
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const f32x4 v = fold_lo<DT>(tile[nt], tile_lo[nt]);
                    acc[rt][nt].x = __builtin_fmaf(v.x, am, acc[rt][nt].x);
                    acc[rt][nt].y = __builtin_fmaf(v.y, am, acc[rt][nt].y);
                    acc[rt][nt].z = __builtin_fmaf(v.z, am, acc[rt][nt].z);
                    acc[rt][nt].w = __builtin_fmaf(v.w, am, acc[rt][nt].w);
                }
            }
            if (j + 1 < NBW) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) xcur[nt][0] = xnext[nt][0], xcur[nt][1] = xnext[nt][1];
            }
        }
    }
    // waves 4..7 park their tiles, waves 0..3 add their own on top (slot w: wave w + wave w + 4), then four slots are summed in order
    __syncthreads();  // every wave is done with its image before the partials overwrite the storage
    if (wave >= 4) {
#pragma unroll
        for (int i = 0; i < kTiles; ++i) *reinterpret_cast<f32x4 *>(&s_part[wave - 4][i * 256 + lane * 4]) = acc[i / NT][i % NT];
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
        for (int i = 0; i < kTiles; ++i) {
            f32x4 *slot = reinterpret_cast<f32x4 *>(&s_part[wave][i * 256 + lane * 4]);
            const f32x4 o = *slot, a = acc[i / NT][i % NT];
            *slot = f32x4{a.x + o.x, a.y + o.y, a.z + o.z, a.w + o.w};
        }
    }
    __syncthreads();
    // thread -> (tile, activation row of the tile, weight row of the tile), consecutive threads on consecutive weight rows
    for (int idx = tid; idx < kTiles * 256; idx += 512) {
        const int tile = idx >> 8, e = idx & 255;
        const int wr = e & 15, n_l = e >> 4;
        const int src = tile * 256 + (((n_l >> 2) * 16 + wr) << 2) + (n_l & 3);  // lane (n_l >> 2) * 16 + wr, register n_l & 3
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) t += s_part[w][src];
        const int n = 16 * (tile % NT) + n_l;
        const int64_t row = row0 + 16 * (tile / NT) + wr;
        if constexpr (FUSED) {
            if (mode & kModeSiluMulPairs) {
                if (!(wr & 1)) {  // an even weight row of the tile (gate); its up row is the next lane's column: src + 4
                    float u = 0.0f;
#pragma unroll
                    for (int w = 0; w < 4; ++w) u += s_part[w][src + 4];
                    if constexpr (MULTI) {
                        if (row < M && n < B) store_nf4_pair_multi<DT>(out, bias, residual, lora_B, lora_ids, n_adapters, lora_t, R, n, row, M, t, u);
                    } else {
                        if (row < M && n < B) store_nf4_pair<DT, LORA>(out, bias, residual, lora_B, lora_t, R, n, row, M, t, u);
                    }
                }
            } else if (row < M && n < B) {
                if constexpr (MULTI) {
                    if (const uint16_t *slice = lora_stack_slice(lora_B, lora_ids, n_adapters, n, M, R))
                        t += lora_delta<DT>(slice + row * R, lora_t + n * R, R);
                } else if constexpr (LORA) {
                    t += lora_delta<DT>(lora_B + row * R, lora_t + n * R, R);
                }
                store_small<DT>(out, bias, residual, n, (int)row, M, t);
            }
        } else {
            if (row < M && n < B) store_small<DT>(out, bias, nullptr, n, (int)row, M, t);
        }
    }
}

std::atomic<int> g_wide_nf4_variant{-1};  // sweep hook: 1 / 2 = 16 / 32 weight rows per workgroup, anything else = the heuristic

// Form: the Nf4Form of the call (nf4_call.h).  The kernel's own flag order is spelt here and nowhere else on the host.
template <int DT, int NT, int RT, int NBW, typename Form>
void launch_wide_nf4(const Nf4Call &a) {
    hipLaunchKernelGGL((gemm_wide_nf4_kernel<DT, NT, RT, NBW, Form::fused, Form::lora, Form::multi, Form::nested>),
                       dim3((unsigned)((a.M + 16 * RT - 1) / (16 * RT))), dim3(512), 0, a.stream, static_cast<const uint16_t *>(a.x), a.W,
                       static_cast<const float *>(a.scales), static_cast<const uint16_t *>(a.bias), static_cast<uint16_t *>(a.out), (int)a.B,
                       (int)a.M, (int)a.K, static_cast<const uint16_t *>(a.residual), a.mode, static_cast<const uint16_t *>(a.adapter.B),
                       a.adapter.t, (int)a.adapter.R, a.adapter.ids, (int)a.adapter.n_adapters, a.nested_stats.group, a.nested_stats.table,
                       a.nested_stats.offset);
}

template <int DT, int NT, typename Form>
void dispatch_wide_nf4_nt(const Nf4Call &a) {
    const int M = (int)a.M, K = (int)a.K;
    // 32 weight rows per workgroup halve the x traffic from L2, the kernel's largest stream: taken once that still fills three
    // quarters of the chip (the FP4 wide kernels' rule; measured here on either side of it, profiles/nf4_wide_batch.json)
    const int v = g_wide_nf4_variant.load(std::memory_order_relaxed);
    const bool rt2 = v == 2 || (v != 1 && M >= 24 * device_cu_count());
    const bool nbw4 = K % 256 == 0;
    if (rt2) {
        if (nbw4) return launch_wide_nf4<DT, NT, 2, 4, Form>(a);
        return launch_wide_nf4<DT, NT, 2, 1, Form>(a);
    }
    if (nbw4) return launch_wide_nf4<DT, NT, 1, 4, Form>(a);
    return launch_wide_nf4<DT, NT, 1, 1, Form>(a);
}

// one launch of a validated call of any form: 1..64 rows, NT = ceil(B / 16) column tiles, the last one ragged
void dispatch_wide_nf4(const Nf4Call &a) {
    with_nf4_form(a, [&](auto form) {
        with_dtype(a.dtype, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            using Form = decltype(form);
            switch ((a.B + 15) / 16) {
                case 1: return dispatch_wide_nf4_nt<DT, 1, Form>(a);
                case 2: return dispatch_wide_nf4_nt<DT, 2, Form>(a);
                case 3: return dispatch_wide_nf4_nt<DT, 3, Form>(a);
                default: return dispatch_wide_nf4_nt<DT, 4, Form>(a);
            }
        });
    });
}

// The one path of the six entry points below; `name` is the entry point the messages speak for.  A call with an adapter covers at
// most 64 rows (one launch), the others 128.
int gemm_wide_nf4_entry(const char *name, const Nf4Call &c) {
    const int64_t B = c.B, M = c.M, K = c.K;
    if (const int rc = nf4_check_args(name, c, c.lora() ? 64 : 128, 64)) return rc;
    if (M == 0 || B == 0) return FP4_OK;
    if (const int rc = nf4_check_adapter(name, c)) return rc;
    // 1..16 rows on a K the 2..16-row kernel covers: that kernel, bit for bit
    if (B <= 16 && K % 512 == 0) {
        gemm_small_nf4_launch(c);
        return check_launch(name);
    }
    const int esize = 2;
    const int64_t M_out = c.gated() ? M / 2 : M;
    // 65..128 rows: two even chunks of at most 64, one pass over the weight each (with an adapter B <= 64: one chunk, so t and ids
    // need no offset)
    const int64_t first = B > 64 ? (B + 1) / 2 : B;
    for (int64_t b0 = 0; b0 < B; b0 += first) {
        Nf4Call chunk = c;
        chunk.B = B - b0 < first ? B - b0 : first;
        chunk.x = static_cast<const uint8_t *>(c.x) + b0 * K * esize;
        if (c.residual) chunk.residual = static_cast<const uint8_t *>(c.residual) + b0 * M_out * esize;
        chunk.out = static_cast<uint8_t *>(c.out) + b0 * M_out * esize;
        dispatch_wide_nf4(chunk);
    }
    return check_launch(name);
}

}  // namespace

void set_wide_nf4_variant(int v) { g_wide_nf4_variant.store(v, std::memory_order_relaxed); }

}  // namespace fp4

extern "C" int fp4_hip_gemm_wide_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, void *out,
                                     int64_t B, int64_t M, int64_t K, int blocksize, int dtype, void *stream) {
    return fp4::gemm_wide_nf4_entry("fp4_hip_gemm_wide_nf4",
                                    {.x = x, .W = packed, .scales = absmax, .bias = bias, .out = out, .B = B, .M = M, .K = K,
                                     .blocksize = blocksize, .dtype = dtype, .stream = static_cast<hipStream_t>(stream)});
}

extern "C" int fp4_hip_gemm_fused_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                      void *out, int64_t B, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemm_fused_nf4";
    const int mode = fp4::epilogue_mode(name, epilogue);
    if (mode < 0) return FP4_ERR_INVALID_ARGUMENT;
    return fp4::gemm_wide_nf4_entry(name, {.x = x, .W = packed, .scales = absmax, .bias = bias, .residual = residual, .out = out, .B = B,
                                           .M = M, .K = K, .blocksize = blocksize, .dtype = dtype, .mode = mode, .fused = true,
                                           .stream = static_cast<hipStream_t>(stream)});
}

extern "C" int fp4_hip_gemm_lora_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                     const void *lora_B, const float *t, int64_t R, void *out, int64_t B, int64_t M, int64_t K,
                                     int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemm_lora_nf4";
    const int mode = fp4::epilogue_mode(name, epilogue);
    if (mode < 0) return FP4_ERR_INVALID_ARGUMENT;
    return fp4::gemm_wide_nf4_entry(name, {.x = x, .W = packed, .scales = absmax, .bias = bias, .residual = residual, .out = out, .B = B,
                                           .M = M, .K = K, .blocksize = blocksize, .dtype = dtype, .mode = mode, .fused = true,
                                           .stream = static_cast<hipStream_t>(stream),
                                           .adapter = {.given = true, .B = lora_B, .t = t, .R = R}});
}

extern "C" int fp4_hip_gemm_lora_multi_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                           const void *B_stack, const int32_t *ids, int64_t n_adapters, const float *t, int64_t R, void *out,
                                           int64_t B, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemm_lora_multi_nf4";
    const int mode = fp4::epilogue_mode(name, epilogue);
    if (mode < 0) return FP4_ERR_INVALID_ARGUMENT;
    return fp4::gemm_wide_nf4_entry(
        name, {.x = x, .W = packed, .scales = absmax, .bias = bias, .residual = residual, .out = out, .B = B, .M = M, .K = K,
               .blocksize = blocksize, .dtype = dtype, .mode = mode, .fused = true, .stream = static_cast<hipStream_t>(stream),
               .adapter = {.given = true, .stack = true, .B = B_stack, .t = t, .R = R, .ids = ids, .n_adapters = n_adapters}});
}

extern "C" int fp4_hip_gemm_nested_nf4(const void *x, const uint8_t *packed, const uint8_t *absmax_u8, const float *nested_absmax,
                                       const float *code256, float offset, int nested_blocksize, const void *bias, const void *residual,
                                       void *out, int64_t B, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemm_nested_nf4";
    fp4::Nf4Call c{.x = x, .W = packed, .scales = absmax_u8, .bias = bias, .residual = residual, .out = out, .B = B, .M = M, .K = K,
                   .blocksize = blocksize, .dtype = dtype, .fused = true, .stream = static_cast<hipStream_t>(stream),
                   .nested_stats = {.given = true, .group = nested_absmax, .table = code256, .offset = offset}};
    if (const int rc = fp4::nested_check_args(name, "GEMM", "fp4_hip_gemm_fused_nf4", epilogue, nested_blocksize, c)) return rc;
    return fp4::gemm_wide_nf4_entry(name, c);
}

extern "C" int fp4_hip_gemm_lora_nested_nf4(const void *x, const uint8_t *packed, const uint8_t *absmax_u8, const float *nested_absmax,
                                            const float *code256, float offset, int nested_blocksize, const void *bias, const void *residual,
                                            const void *lora_B, const float *t, int64_t R, void *out, int64_t B, int64_t M, int64_t K,
                                            int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemm_lora_nested_nf4";
    fp4::Nf4Call c{.x = x, .W = packed, .scales = absmax_u8, .bias = bias, .residual = residual, .out = out, .B = B, .M = M, .K = K,
                   .blocksize = blocksize, .dtype = dtype, .fused = true, .stream = static_cast<hipStream_t>(stream),
                   .adapter = {.given = true, .B = lora_B, .t = t, .R = R},
                   .nested_stats = {.given = true, .group = nested_absmax, .table = code256, .offset = offset}};
    if (const int rc = fp4::nested_check_args(name, "GEMM", "fp4_hip_gemm_lora_nf4", epilogue, nested_blocksize, c)) return rc;
    return fp4::gemm_wide_nf4_entry(name, c);
}
