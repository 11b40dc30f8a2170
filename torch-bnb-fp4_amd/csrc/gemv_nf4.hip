// Fused batch-1 GEMV over an NF4 weight for gfx950 (MI355X):
//     out[r] = sum_k x[k] * nf4[nib(r,k)] * absmax[(r*K+k)/bs]      (+ bias[r])
//
// Not in the reference (it has FP4 only).  The FP4 GEMV's table-free decode does not carry over: it relies on 12*code being
// exact in 8 bits, and the NF4 values are not exact in fp16 or bf16 (one fp16-rounded code is ~2^-12 off per weight, outside
// the f32-accumulation parity bar at small K).  So every weight is decoded through an f32 table in LDS and multiplied into
// f32 copies of x, which keeps each code exact; x is widened to f32 once per lane and reused for all of its rows.
//
// Geometry: the register-x mapping of the FP4 f32 kernel (gemv32_regx_kernel): 256 threads, a half-wave per row, each lane
// owns 32-weight chunks (one 16-byte load) at the same K positions for every row of its workgroup, K split into 1..4 bands
// of 32 chunks, one wave per band.  x is requested before the weight stream and the load phase is branch-free (clamped
// index + zero scale), as in gemv_fp4.hip.  Rows longer than 256 chunks (K > 8192) loop over 256-chunk slices of K.
// Two table layouts (fp4_hip_set_variant("gemv_nf4", v); profiles/nf4_gemv_ablation.txt):
//   0 = 16 f32 entries, one ds_read_b32 per weight (every read a broadcast among 16 consecutive dwords: conflict-free);
//   1 = 256 f32 pairs indexed by the packed byte, one ds_read_b64 per two weights (half the LDS instructions, but the
//       addresses of a wave are spread over 2 KiB, so reads can collide in banks).
// Irregular shapes (K % 32 != 0, blocksize not a power of two >= 32 dividing K, unaligned operands) run the FP4 generic
// kernel of gemv_fp4.hip with the NF4 table as its argument.
//
// Fused decode epilogues (fp4_hip_gemv_fused_nf4): the FUSED instantiations take a residual and the `mode` of gemv_fp4.hip.  The
// two half-waves of a wave already hold rows 2j and 2j + 1, row_base and the rows per workgroup are even, so a gate row and its
// up row meet in one wave (KSPLIT == 1) or in neighbouring s_part rows (KSPLIT > 1) and the pair never straddles a workgroup.
// The epilogue is a compile-time choice: the plain entry point keeps the instantiations it had, instruction for instruction.
//
// LoRA adapter term (fp4_hip_gemv_lora_nf4): the LORA instantiations (always FUSED) add delta[r] = sum_j f32(B[r][j]) * t[j] to the
// row's f32 sum before it is rounded; t = s * A x is lora_down_kernel's f32 output (lora_nf4.hip).  The lanes of the half-wave that
// owns the row with 8 * l32 < R request 16 bytes of B[row] and their t slice before the weight stream, as x is requested; their
// partial deltas go through a second copy of the dpp chain (not through p[it]: the plain sum keeps its order and its bits) and
// sum + delta is one f32 add.  With KSPLIT > 1 only the kw == 0 wave of a row carries the term, through a column of its own in s_part.
//
// Several adapters, chosen on the device (fp4_hip_gemv_lora_multi_nf4): the MULTI instantiations (always LORA) take a stack of B arrays
// and read the row's adapter from lora_ids[0] (uniform over the grid).  With one, lora_B becomes its slice and everything is the LORA
// kernel's; without one neither B nor t is read and the delta is not added, so the bits are the FUSED kernel's.  It exists so that a
// captured one-row step follows an in-place change of the id.
//
// Nested (double-quantised) absmax (fp4_hip_gemv_nested_nf4, with the adapter term fp4_hip_gemv_lora_nested_nf4): the NESTED
// instantiations (always FUSED, with or without LORA, never MULTI) read the block
// scale as bitsandbytes' compress_statistics stores it - a uint8 code per block, an f32 scale per 256 blocks, a 256-entry f32 table
// and an offset - and form absmax = fl32(fl32(table[code] * group) + offset) themselves (unnest_scale, nested_absmax.h): 33 instead
// of 36 bytes streamed per 64 weights and a quarter of the resident statistics.  The table sits in LDS beside the NF4 table; the
// code byte and the group scale are requested where the f32 scale was.  Everything after the scale is the FUSED kernel's, so the
// result equals fp4_hip_gemv_fused_nf4 (with LORA: fp4_hip_gemv_lora_nf4) on the expanded absmax bit for bit.
//
// Host side: the six extern "C" entry points each fill an Nf4Call (nf4_call.h) and share one path, gemv_nf4_entry(name, call): the
// checks, one read of the variant hook, one dispatch.  dispatch_nf4 goes from the call's form and dtype (with_nf4_form, with_dtype)
// to the geometry (dispatch_nf4_shape) to the launch (launch_nf4, the only place that spells the kernel's flag order).
#include <atomic>

#include "launchers.h"
#include "nf4_call.h"

namespace fp4 {

namespace {

// 8 consecutive activations (one 16-byte load of 16-bit x, two of f32) as f32
template <int DT>
__device__ __forceinline__ void load_x8(const void *x, int64_t i8, f32x4 &a, f32x4 &b) {
    if constexpr (DT == FP4_DTYPE_F32) {
        a = reinterpret_cast<const f32x4 *>(x)[2 * i8];
        b = reinterpret_cast<const f32x4 *>(x)[2 * i8 + 1];
    } else {
        const u32x4 v = reinterpret_cast<const u32x4 *>(x)[i8];
        a = f32x4{to_f32<DT>(uint16_t(v.x & 0xFFFFu)), to_f32<DT>(uint16_t(v.x >> 16)), to_f32<DT>(uint16_t(v.y & 0xFFFFu)),
                  to_f32<DT>(uint16_t(v.y >> 16))};
        b = f32x4{to_f32<DT>(uint16_t(v.z & 0xFFFFu)), to_f32<DT>(uint16_t(v.z >> 16)), to_f32<DT>(uint16_t(v.w & 0xFFFFu)),
                  to_f32<DT>(uint16_t(v.w >> 16))};
    }
}

// `residual` may alias `out`: the element is read before it is written, by the same lane
template <int DT>
__device__ __forceinline__ void store_nf4_row(void *out, const void *bias, const void *residual, int row, float sum) {
    if constexpr (DT == FP4_DTYPE_F32) {
        float t = bias ? sum + reinterpret_cast<const float *>(bias)[row] : sum;
        if (residual) t += reinterpret_cast<const float *>(residual)[row];
        reinterpret_cast<float *>(out)[row] = t;
    } else {
        store_row<DT>(reinterpret_cast<uint16_t *>(out), reinterpret_cast<const uint16_t *>(bias),
                      reinterpret_cast<const uint16_t *>(residual), row, sum);
    }
}

// the plain kernels promise the compiler that nothing else points into `out`; with a residual that may alias it they cannot
template <bool FUSED>
struct OutPtr {
    typedef void *__restrict__ type;
};
template <>
struct OutPtr<true> {
    typedef void *type;
};

// FUSED = false: `residual` and `mode` are ignored (fp4_hip_gemv_nf4).  FUSED = true: the row epilogue adds the residual, and with
// kModeSiluMulPairs (16-bit DT only, M even) rows (2i, 2i + 1) are a gate / up pair and out[i] = silu(gate_i) * up_i (+ residual[i]).
// LORA = true (with FUSED): delta[row] = sum_j lora_B[row][j] * lora_t[j] (R % 8 == 0, 8 <= R <= 256) is added to the f32 row sum first.
// NESTED = true (with FUSED, without MULTI): `absmax` points at uint8 codes, one per block; the scale of block i is
// unnest_scale(nested_code[code[i]], nested_absmax[i >> 8], nested_offset).
// MULTI = true (with LORA): lora_B is a stack of n_adapters arrays T[M][R], lora_ids[0] names the adapter; outside 0 .. n_adapters - 1 = none.
template <int DT, int KSPLIT, int G, int ITERS, bool PAIR, bool FUSED, bool LORA = false, bool NESTED = false, bool MULTI = false>
__global__ __launch_bounds__(256) void gemv_nf4_kernel(const void *__restrict__ x, const uint8_t *__restrict__ W,
                                                       const float *__restrict__ absmax, const void *__restrict__ bias,
                                                       typename OutPtr<FUSED>::type out, int M, int K, int bs_shift,
                                                       const void *residual_arg, int mode,  // new arguments last: the plain kernels keep their argument layout
                                                       const void *lora_B, const float *lora_t, int R,
                                                       const float *nested_absmax, const float *nested_code, float nested_offset,
                                                       const int *lora_ids, int n_adapters) {
    static_assert(!LORA || FUSED, "the adapter term comes with the fused epilogues");
    static_assert(!MULTI || LORA, "the adapter stack comes with the adapter term");
    [[maybe_unused]] bool adapted = LORA;  // MULTI: whether lora_ids[0] names an adapter (uniform)
    if constexpr (MULTI) {
        const int id = lora_ids[0];
        adapted = uint32_t(id) < uint32_t(n_adapters);
        if (adapted) lora_B = reinterpret_cast<const uint8_t *>(lora_B) + int64_t(id) * M * R * (DT == FP4_DTYPE_F32 ? 4 : 2);
    }
    static_assert(!NESTED || (FUSED && !MULTI), "nested absmax comes with the fused epilogues and without the adapter stack");
    const void *residual = FUSED ? residual_arg : nullptr;
    [[maybe_unused]] const bool gated = FUSED && DT != FP4_DTYPE_F32 && (mode & kModeSiluMulPairs);
    constexpr int RG = 4 / KSPLIT;
    constexpr int kRowsPerBlock = 2 * RG * ITERS;
    constexpr int kBand = G * 32 * KSPLIT;  // chunks of K covered per pass
    __shared__ float s_lut[PAIR ? 1 : 16];
    __shared__ f32x2 s_pair[PAIR ? 256 : 1];
    __shared__ float s_ncode[NESTED ? 256 : 1];
    __shared__ float s_part[kRowsPerBlock][KSPLIT + (LORA && KSPLIT > 1 ? 1 : 0)];  // LORA: column KSPLIT holds the row's delta
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int kw = wave % KSPLIT, rw = wave / KSPLIT;
    const int half = lane >> 5, l32 = lane & 31;
    const int C = K >> 5;
    const int row_base = blockIdx.x * kRowsPerBlock;
    const u32x4 *Wv = reinterpret_cast<const u32x4 *>(W);
    if constexpr (PAIR) {
        s_pair[tid] = f32x2{nf4_lut_entry(tid >> 4), nf4_lut_entry(tid & 15)};  // byte -> (high nibble, low nibble)
    } else {
        if (tid < 16) s_lut[tid] = nf4_lut_entry(tid);
    }
    if constexpr (NESTED) s_ncode[tid] = nested_code[tid];  // 256 threads, 256 entries

    int rowi[ITERS], rclamp[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        rowi[it] = 2 * (it * RG + rw) + half;
        const int row = row_base + rowi[it];
        rclamp[it] = row < M ? row : M - 1;
    }
    float p[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) p[it] = 0.0f;
    // LORA: this lane's 8 columns of B for each of its rows and the matching slice of t, requested ahead of the weight stream
    // (branch-free: a lane past R re-reads unit 0 against a zero t; waves with kw != 0 carry no adapter term)
    // (B stays as loaded - 4 VGPRs per row in a 16-bit T - until the row's epilogue widens it)
    constexpr int kLbRegs = DT == FP4_DTYPE_F32 ? 2 : 1;
    [[maybe_unused]] u32x4 lb[LORA ? ITERS : 1][kLbRegs];
    [[maybe_unused]] f32x4 lt[2];
    if constexpr (LORA) {
        if (kw == 0 && (!MULTI || adapted)) {
            const bool on = 8 * l32 < R;
            const int j8 = on ? l32 : 0;
            lt[0] = reinterpret_cast<const f32x4 *>(lora_t)[2 * j8];
            lt[1] = reinterpret_cast<const f32x4 *>(lora_t)[2 * j8 + 1];
            if (!on) lt[0] = lt[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const u32x4 *src = reinterpret_cast<const u32x4 *>(lora_B) + ((int64_t(rclamp[it]) * R >> 3) + j8) * kLbRegs;
#pragma unroll
                for (int q = 0; q < kLbRegs; ++q) lb[it][q] = src[q];
            }
        }
    }

    for (int cb = 0; cb < C; cb += kBand) {
        int cidx[G];
        bool live[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c = cb + g * (32 * KSPLIT) + kw * 32 + l32;
            live[g] = c < C;
            cidx[g] = live[g] ? c : C - 1;
        }
        f32x4 xv[G][8];
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int q = 0; q < 4; ++q) load_x8<DT>(x, int64_t(cidx[g]) * 4 + q, xv[g][2 * q], xv[g][2 * q + 1]);
        }
        u32x4 wq[ITERS][G];
        float am[ITERS][G];
        [[maybe_unused]] uint32_t aq[NESTED ? ITERS : 1][NESTED ? G : 1];  // NESTED: the block's code; am holds its group's scale
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int64_t chunk = int64_t(rclamp[it]) * C + cidx[g];
                wq[it][g] = __builtin_nontemporal_load(Wv + chunk);
                if constexpr (NESTED) {
                    const int64_t blk = (chunk << 5) >> bs_shift;
                    aq[it][g] = reinterpret_cast<const uint8_t *>(absmax)[blk];
                    am[it][g] = nested_absmax[blk >> kNestedGemvShift];
                } else {
                    const float a = absmax[(chunk << 5) >> bs_shift];
                    am[it][g] = live[g] ? a : 0.0f;
                }
            }
        }
        if (cb == 0) __syncthreads();  // tables visible (uniform: every thread runs the same passes)
        if constexpr (NESTED) {
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float a = unnest_scale(s_ncode[aq[it][g]], am[it][g], nested_offset);
                    am[it][g] = live[g] ? a : 0.0f;
                }
            }
        }
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
                for (int q = 0; q < 8; ++q) {  // weights 4q..4q+3 of the chunk = bytes 2q, 2q+1
                    const uint32_t h = (wq[it][g][q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
                    if constexpr (PAIR) {
                        const f32x2 c01 = s_pair[h & 0xFFu], c23 = s_pair[h >> 8];
                        s0 = __builtin_fmaf(c01.x, xv[g][q].x, s0);
                        s1 = __builtin_fmaf(c01.y, xv[g][q].y, s1);
                        s0 = __builtin_fmaf(c23.x, xv[g][q].z, s0);
                        s1 = __builtin_fmaf(c23.y, xv[g][q].w, s1);
                    } else {
                        s0 = __builtin_fmaf(s_lut[(h >> 4) & 15u], xv[g][q].x, s0);
                        s1 = __builtin_fmaf(s_lut[h & 15u], xv[g][q].y, s1);
                        s0 = __builtin_fmaf(s_lut[(h >> 12) & 15u], xv[g][q].z, s0);
                        s1 = __builtin_fmaf(s_lut[(h >> 8) & 15u], xv[g][q].w, s1);
                    }
                }
                p[it] = __builtin_fmaf(s0 + s1, am[it][g], p[it]);
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        float v = p[it];
        v = dpp_add<0x128>(v);
        v = dpp_add<0x124>(v);
        v = dpp_add<0x122>(v);
        v = dpp_add<0x121>(v);
        v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));  // 32-lane row sum
        if constexpr (LORA) {
            if (kw == 0 && (!MULTI || adapted)) {  // wave-uniform
                f32x4 b0, b1;
                lora_widen8<DT>(lb[it], b0, b1);
                float d = lora_dot8(b0, b1, lt[0], lt[1], 0.0f);
                d = dpp_add<0x128>(d);
                d = dpp_add<0x124>(d);
                d = dpp_add<0x122>(d);
                d = dpp_add<0x121>(d);
                d += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, d), 0x401F));  // the row's delta
                if constexpr (KSPLIT == 1)
                    v += d;  // sum' = sum + delta, one f32 add
                else if (l32 == 0)
                    s_part[rowi[it]][KSPLIT] = d;
            }
        }
        if constexpr (KSPLIT == 1) {
            const int row = row_base + rowi[it];
            if constexpr (FUSED && DT != FP4_DTYPE_F32) {
                if (gated) {
                    // the two half-waves hold the gate row (even, lanes 0..31) and the up row (odd) of one pair; M is even
                    const float up = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
                    if (lane == 0 && row < M)
                        store_silu_mul<DT>(reinterpret_cast<uint16_t *>(out), reinterpret_cast<const uint16_t *>(bias),
                                           reinterpret_cast<const uint16_t *>(residual), row >> 1, v, up);
                    continue;
                }
            }
            if (l32 == 0 && row < M) store_nf4_row<DT>(out, bias, residual, row, v);
        } else {
            if (l32 == 0) s_part[rowi[it]][kw] = v;
        }
    }
    if constexpr (KSPLIT > 1) {
        __syncthreads();
        if constexpr (FUSED && DT != FP4_DTYPE_F32) {
            if (gated) {
                if (tid < kRowsPerBlock / 2) {  // rows 2 * tid (gate) and 2 * tid + 1 (up) of this workgroup; row_base and M are even
                    float g = 0.0f, u = 0.0f;
#pragma unroll
                    for (int k = 0; k < KSPLIT; ++k) g += s_part[2 * tid][k], u += s_part[2 * tid + 1][k];
                    if constexpr (MULTI) {
                        if (adapted) g += s_part[2 * tid][KSPLIT], u += s_part[2 * tid + 1][KSPLIT];
                    } else if constexpr (LORA) {
                        g += s_part[2 * tid][KSPLIT], u += s_part[2 * tid + 1][KSPLIT];
                    }
                    const int row = row_base + 2 * tid;
                    if (row < M)
                        store_silu_mul<DT>(reinterpret_cast<uint16_t *>(out), reinterpret_cast<const uint16_t *>(bias),
                                           reinterpret_cast<const uint16_t *>(residual), row >> 1, g, u);
                }
                return;
            }
        }
        if (tid < kRowsPerBlock) {
            float t = 0.0f;
#pragma unroll
            for (int k = 0; k < KSPLIT; ++k) t += s_part[tid][k];
            if constexpr (MULTI) {
                if (adapted) t += s_part[tid][KSPLIT];
            } else if constexpr (LORA) {
                t += s_part[tid][KSPLIT];
            }
            const int row = row_base + tid;
            if (row < M) store_nf4_row<DT>(out, bias, residual, row, t);
        }
    }
}

std::atomic<int> g_gemv_nf4_variant{-1};  // sweep hook: 0 = 16-entry table, 1 = pair table, -1 = default

// Form: the Nf4Form of the call (nf4_call.h).  The kernel's own flag order is spelt here and nowhere else on the host.
template <int DT, int KSPLIT, int G, int ITERS, typename Form>
void launch_nf4(bool pair, const Nf4Call &a) {
    constexpr int rows_per_block = 2 * (4 / KSPLIT) * ITERS;
    const dim3 grid((unsigned)((a.M + rows_per_block - 1) / rows_per_block)), block(256);
    auto launch = [&](auto pair_table) {
        hipLaunchKernelGGL((gemv_nf4_kernel<DT, KSPLIT, G, ITERS, decltype(pair_table)::value, Form::fused, Form::lora, Form::nested, Form::multi>),
                           grid, block, 0, a.stream, a.x, a.W, static_cast<const float *>(a.scales), a.bias, a.out, (int)a.M, (int)a.K,
                           ilog2_exact(a.blocksize), a.residual, a.mode, a.adapter.B, a.adapter.t, (int)a.adapter.R, a.nested_stats.group,
                           a.nested_stats.table, a.nested_stats.offset, a.adapter.ids, (int)a.adapter.n_adapters);
    };
    pair ? launch(std::true_type{}) : launch(std::false_type{});
}

template <int DT, typename Form>
void dispatch_nf4_shape(bool pair, const Nf4Call &a) {
    const int M = (int)a.M;
    const int C = (int)a.K >> 5;
    const int ks = C <= 32 ? 1 : (C <= 64 ? 2 : 4);
    // the x slice is re-read by every workgroup: amortise it over up to 4 row pairs per lane while >= ~256 workgroups remain
    // (the FP4 f32 kernel's rule, gemv_fp4.hip dispatch32_regx)
    int iters = 1;
    while (iters < 4 && M / (2 * (4 / ks) * iters * 2) >= 256) iters *= 2;
#define NF4_ITERS(KS, GG)                                             \
    switch (iters) {                                                  \
        case 1: return launch_nf4<DT, KS, GG, 1, Form>(pair, a);      \
        case 2: return launch_nf4<DT, KS, GG, 2, Form>(pair, a);      \
        default: return launch_nf4<DT, KS, GG, 4, Form>(pair, a);     \
    }
    if (C <= 32) { NF4_ITERS(1, 1) }
    if (C <= 64) { NF4_ITERS(2, 1) }
    if (C <= 128) { NF4_ITERS(4, 1) }
    NF4_ITERS(4, 2)
#undef NF4_ITERS
}

// the fast path: a validated call of any form and dtype -> its kernel
void dispatch_nf4(bool pair, const Nf4Call &a) {
    with_nf4_form(a, [&](auto form) {
        with_dtype<true>(a.dtype, [&](auto dt) { dispatch_nf4_shape<decltype(dt)::value, decltype(form)>(pair, a); });
    });
}

// The one path of the six GEMV entry points; `name` is the entry point the messages speak for.  The plain form runs irregular
// shapes on the generic kernel; every other form is the fast path or FP4_ERR_UNSUPPORTED with nothing launched.
int gemv_nf4_entry(const char *name, const Nf4Call &c) {
    const int64_t M = c.M, K = c.K;
    const int blocksize = c.blocksize, dtype = c.dtype;
    if (M < 0 || K < 0 || (K & 1) || blocksize < 2 || (blocksize & 1)) {
        set_error("%s: M=%lld K=%lld blocksize=%d (need M,K >= 0, even K, even blocksize >= 2)", name, (long long)M, (long long)K,
                  blocksize);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (dtype != FP4_DTYPE_F16 && dtype != FP4_DTYPE_BF16 && dtype != FP4_DTYPE_F32) {
        set_error("%s: unsupported dtype %d", name, dtype);
        return FP4_ERR_UNSUPPORTED;
    }
    if (c.gated() && (M & 1)) {
        set_error("%s: the gate|up epilogue needs an even row count, got M=%lld", name, (long long)M);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (c.lora() && c.adapter.R < 0) {
        set_error("%s: R=%lld (need R >= 0)", name, (long long)c.adapter.R);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (M == 0) return FP4_OK;
    if (!c.out || (K > 0 && (!c.x || !c.W || !c.scales)) || (c.lora() && (!c.adapter.B || !c.adapter.t))) {
        set_error("%s: null pointer", name);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (M > (int64_t(1) << 30) || K > (int64_t(1) << 30)) {
        set_error("%s: M=%lld K=%lld too large", name, (long long)M, (long long)K);
        return FP4_ERR_UNSUPPORTED;
    }
    const uintptr_t align = reinterpret_cast<uintptr_t>(c.W) | reinterpret_cast<uintptr_t>(c.x);
    const bool fast = K > 0 && (K % 32) == 0 && ilog2_exact(blocksize) >= 5 && (K % blocksize) == 0 && (align & 15u) == 0;
    if (c.fused && (!fast || (c.gated() && dtype == FP4_DTYPE_F32))) {
        set_error("%s: the fused epilogue is not available for M=%lld K=%lld blocksize=%d dtype=%d epilogue=%d (needs K %% 32 == 0, a "
                  "power-of-two blocksize >= 32 that divides K, 16-byte aligned x and packed; the gate|up epilogue a 16-bit dtype); run "
                  "the plain GEMV and apply the epilogue separately",
                  name, (long long)M, (long long)K, blocksize, dtype, c.gated() ? 1 : 0);
        return FP4_ERR_UNSUPPORTED;
    }
    if (const int rc = nf4_check_adapter(name, c)) return rc;
    if (fast)
        dispatch_nf4(g_gemv_nf4_variant.load(std::memory_order_relaxed) == 1, c);
    else  // the plain form only
        gemv_generic_table({.x = c.x, .W = c.W, .absmax = static_cast<const float *>(c.scales), .bias = c.bias, .out = c.out, .M = M, .K = K,
                            .blocksize = blocksize, .dtype = dtype, .stream = c.stream}, FP4_TABLE_NF4);
    return check_launch(name);
}

}  // namespace

void set_gemv_nf4_variant(int v) { g_gemv_nf4_variant.store(v, std::memory_order_relaxed); }

}  // namespace fp4

extern "C" int fp4_hip_gemv_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, void *out, int64_t M,
                                int64_t K, int blocksize, int dtype, void *stream) {
    return fp4::gemv_nf4_entry("fp4_hip_gemv_nf4", {.x = x, .W = packed, .scales = absmax, .bias = bias, .out = out, .M = M, .K = K,
                                                    .blocksize = blocksize, .dtype = dtype, .stream = static_cast<hipStream_t>(stream)});
}

extern "C" int fp4_hip_gemv_fused_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                      void *out, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemv_fused_nf4";
    const int mode = fp4::epilogue_mode(name, epilogue);
    if (mode < 0) return FP4_ERR_INVALID_ARGUMENT;
    return fp4::gemv_nf4_entry(name, {.x = x, .W = packed, .scales = absmax, .bias = bias, .residual = residual, .out = out, .M = M, .K = K,
                                      .blocksize = blocksize, .dtype = dtype, .mode = mode, .fused = true,
                                      .stream = static_cast<hipStream_t>(stream)});
}

extern "C" int fp4_hip_gemv_lora_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                     const void *lora_B, const float *t, int64_t R, void *out, int64_t M, int64_t K, int blocksize,
                                     int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemv_lora_nf4";
    const int mode = fp4::epilogue_mode(name, epilogue);
    if (mode < 0) return FP4_ERR_INVALID_ARGUMENT;
    return fp4::gemv_nf4_entry(name, {.x = x, .W = packed, .scales = absmax, .bias = bias, .residual = residual, .out = out, .M = M, .K = K,
                                      .blocksize = blocksize, .dtype = dtype, .mode = mode, .fused = true, .stream = static_cast<hipStream_t>(stream),
                                      .adapter = {.given = true, .B = lora_B, .t = t, .R = R}});
}

extern "C" int fp4_hip_gemv_lora_multi_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                           const void *B_stack, const int32_t *ids, int64_t n_adapters, const float *t, int64_t R, void *out,
                                           int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemv_lora_multi_nf4";
    const int mode = fp4::epilogue_mode(name, epilogue);
    if (mode < 0) return FP4_ERR_INVALID_ARGUMENT;
    return fp4::gemv_nf4_entry(name, {.x = x, .W = packed, .scales = absmax, .bias = bias, .residual = residual, .out = out, .M = M, .K = K,
                                      .blocksize = blocksize, .dtype = dtype, .mode = mode, .fused = true, .stream = static_cast<hipStream_t>(stream),
                                      .adapter = {.given = true, .stack = true, .B = B_stack, .t = t, .R = R, .ids = ids, .n_adapters = n_adapters}});
}

extern "C" int fp4_hip_gemv_nested_nf4(const void *x, const uint8_t *packed, const uint8_t *absmax_u8, const float *nested_absmax,
                                       const float *code256, float offset, int nested_blocksize, const void *bias, const void *residual,
                                       void *out, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemv_nested_nf4";
    fp4::Nf4Call c{.x = x, .W = packed, .scales = absmax_u8, .bias = bias, .residual = residual, .out = out, .M = M, .K = K,
                   .blocksize = blocksize, .dtype = dtype, .fused = true, .stream = static_cast<hipStream_t>(stream),
                   .nested_stats = {.given = true, .group = nested_absmax, .table = code256, .offset = offset}};
    if (const int rc = fp4::nested_check_args(name, "GEMV", "fp4_hip_gemv_fused_nf4", epilogue, nested_blocksize, c)) return rc;
    // K == 0 never reaches a kernel: the fused form refuses it (not the fast path) before the statistics are looked at
    return fp4::gemv_nf4_entry(name, c);
}

extern "C" int fp4_hip_gemv_lora_nested_nf4(const void *x, const uint8_t *packed, const uint8_t *absmax_u8, const float *nested_absmax,
                                            const float *code256, float offset, int nested_blocksize, const void *bias, const void *residual,
                                            const void *lora_B, const float *t, int64_t R, void *out, int64_t M, int64_t K, int blocksize,
                                            int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemv_lora_nested_nf4";
    fp4::Nf4Call c{.x = x, .W = packed, .scales = absmax_u8, .bias = bias, .residual = residual, .out = out, .M = M, .K = K,
                   .blocksize = blocksize, .dtype = dtype, .fused = true, .stream = static_cast<hipStream_t>(stream),
                   .adapter = {.given = true, .B = lora_B, .t = t, .R = R},
                   .nested_stats = {.given = true, .group = nested_absmax, .table = code256, .offset = offset}};
    if (const int rc = fp4::nested_check_args(name, "GEMV", "fp4_hip_gemv_lora_nf4", epilogue, nested_blocksize, c)) return rc;
    return fp4::gemv_nf4_entry(name, c);
}
