// NF4 product for quant blocks LARGER than the matrix-core step (gfx950, MI355X): 1..64 activation rows against one NF4 weight whose
// absmax covers bs = 128 .. 4096 weights (a power of two dividing K), one pass over the packed weight,
//     out[b][r] = T( sum_k x[b][k] * code[nib(r,k)] * absmax[(r*K+k)/bs] + bias[r] )          then the epilogue of the fused ops
// f32 accumulation, bias added in f32, one rounding to T.  Blocksize 64 is gemm_wide_nf4.hip's (fp4_hip_gemm_fused_nf4): there the
// quant block IS the matrix-core step pair, and that kernel applies one scale per 64 weights.  Here it is not, and the inner loop is
// built on that.
//
// Operand roles are gemm_wide_nf4.hip's: x is the A operand, the weight the B operand of v_mfma_f32_16x16x32_{bf16,f16}, a lane's
// four accumulators of a tile belong to ONE weight row (D column = lane & 15), so a scale is one scalar per lane.  The decode (hi / lo
// halves of every code from one byte-indexed LDS table, fp16's lo products in a tile of their own, scaled by 2^24) is nf4_mfma.h's.
//
// One scale application per quant block.  A "step" is 64 weights (two MFMA k-steps of 32).  A wave's K unit is NS steps: NS = 4
// (256 weights) where K % 256 == 0, NS = 2 (128 weights) otherwise, which happens at bs = 128 with an odd block count only.  A unit
// holds `groups` runs of `gsteps` steps that share one scale:
//     bs = 128, NS = 4:  2 groups of 2 steps (two whole blocks)        bs = 128, NS = 2:  1 group of 2 steps (one block)
//     bs = 256:          1 group of 4 steps (one whole block)          bs >= 512:         1 group of 4 steps (a slice of one block)
// The hi and lo MFMAs of all steps of a group chain into one tile per (row tile, column tile) - 4 * gsteps instructions deep (bf16) -
// and the tile is folded into acc with the group's scale ONCE: per 256 weights, row tile and column tile one fold_lo + 4 FMAs where
// the blocksize-64 kernel issues four, and no tile is zeroed in between.  For bs >= 512 the slices of one block held by different
// waves (or by one wave in different passes) are each scaled by the same absmax and meet in the fixed-order sum below: the scale
// distributes over the slices, and no wave waits for another.  bs and with it (gsteps, groups) is a RUN-TIME parameter (log2 bs): the
// step loop is rolled and tests the group boundary with a wave-uniform mask, so one instantiation serves every block size.
// The price is registers: the tiles of ALL row tiles stay live across the steps of a group (the blocksize-64 kernel loops the row
// tiles inside a step and keeps NT tiles), which the kernel has room for - see the resource table build.py writes.
//
// Scale stream sized to the block.  Per pass a wave fetches ONE scale per weight row and group it touches - rows * groups <= 64
// values, one 4-byte load instruction - instead of rows * NS: a quarter of the blocksize-64 kernel's scale loads at bs >= 256, half at
// bs = 128, and the absmax array itself is bs / 64 times smaller in HBM.  The image row carries `groups` (1 or 2) scales behind its
// bytes; a lane reads the group's scale once per group (ds_read_b32, a broadcast over the 4 lanes of a row), not once per step.
// For bs >= 512 the eight waves' units u = 8p .. 8p + 7 lie in at most 8 * 256 / bs blocks of a row, so waves re-read each other's
// scale.  Each wave still fetches its own: the image is wave-private and ordered by wave barriers alone, and handing one wave's
// fetch to seven others would put a workgroup barrier (or a second, shared image with its own fence) into every pass of the K loop -
// to save 16 or 32 four-byte loads per wave and pass that hit the same cache lines the first wave's fetch brought in.  The weight
// stream (rows * 128 bytes per wave and pass, from HBM) is what the loop waits for; the repeated scale is not.
//
// Work split: gemm_wide_nf4.hip's.  A workgroup of 8 waves owns RT 16-row tiles of W (RT in {1, 2}: 32 rows halve the x traffic from
// L2 and are taken once M >= 24 * CUs, the wide kernels' rule; fp4_hip_set_variant("gemm_blocks_nf4", 1 | 2 | -1) forces either) and all
// NT = ceil(B / 16) column tiles; the waves split K in units (unit u = pass * 8 + wave; a ragged last pass leaves the upper waves
// idle).  The unit's bytes and scales are fetched one pass ahead with row-contiguous 16-byte loads and staged through a wave-private
// LDS image (WeightImage<NS, 16 RT> of wave_image.h, used as it is: NS steps of bytes per row, the scales in the first `groups` slots
// of the row's tail); x fragments come straight from L2, one step ahead.  The eight waves' partial tiles meet in LDS and are added in
// a fixed order: deterministic, no atomics, no workspace.  Rows and byte offsets are 64-bit: M * K may pass 2^32 (M <= 2^30, K <= 2^24).
//
// Epilogues (fp4_hip_gemm_blocks_nf4 has fp4_hip_gemm_fused_nf4's signature): none, residual add (`residual` may alias `out`: each
// element is read, then written, by one thread), silu(gate) * up over interleaved row pairs into out[B][M / 2] (M even) - the final
// pass of gemm_wide_nf4_kernel's FUSED instantiations with store_small / store_nf4_pair.
#include <atomic>

#include "launchers.h"
#include "nf4_mfma.h"
#include "wave_image.h"

namespace fp4 {

namespace {

// Lane (r = l & 15, kb = l >> 4).  Instruction t = 0, 1 of step j takes k = 64j + 32t .. + 31 in natural order: the B operand is the
// packed dword [16t + 4kb, 16t + 4kb + 4) of the step's 32 bytes of weight row r, the A operand x[16nt + r][64 (s0 + j) + 32t + 8kb ..],
// s0 = u * NS the unit's first step.  D: lane holds out[16nt + 4kb + reg][row0 + 16rt + r].
// bshift = log2(bs), 7..12.  `residual` may be null; mode is 0 or kModeSiluMulPairs.
template <int DT, int NT, int RT, int NS>
__global__ __launch_bounds__(512) void gemm_blocks_nf4_kernel(const uint16_t *__restrict__ x, const uint8_t *__restrict__ W,
                                                              const float *__restrict__ absmax, const uint16_t *__restrict__ bias,
                                                              uint16_t *out, int B, int M, int K, int bshift, const uint16_t *residual,
                                                              int mode) {
    constexpr int kRows = 16 * RT;
    using WImg = WeightImage<NS, kRows>;
    constexpr int kImageBytes = 8 * WImg::kBytes;
    constexpr int kTiles = RT * NT;
    constexpr int kPartBytes = 4 * kTiles * 256 * 4;  // four slots: see the reduction below
    // the cross-wave partial sums reuse the images' storage after the K loop; the code table has storage of its own
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[kImageBytes > kPartBytes ? kImageBytes : kPartBytes];
    __shared__ __attribute__((aligned(16))) u32x2 s_code[256];
    float (*s_part)[kTiles * 256] = reinterpret_cast<float (*)[kTiles * 256]>(s_raw);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 15, kb = lane >> 4;
    const int64_t row0 = int64_t(blockIdx.x) * kRows;
    const int nunits = (K >> 6) / NS;
    const int passes = (nunits + 7) >> 3;
    const int nblk = K >> bshift;  // quant blocks per weight row
    // steps per group - 1 (a mask: both are powers of two) and log2(groups per unit)
    const int gmask = ((1 << (bshift - 6)) < NS ? (1 << (bshift - 6)) : NS) - 1;
    const int glog = NS == 4 && bshift == 7 ? 1 : 0;
    const u32x4 *x4 = reinterpret_cast<const u32x4 *>(x);

    // this lane's scale of a unit: group (lane & (groups - 1)) of image row (lane >> glog) % kRows.  With fewer than 64 scales the
    // upper lanes repeat rows: same address, same value, same slot.
    const int sc_g = lane & ((1 << glog) - 1), sc_rr = (lane >> glog) % kRows;
    const int64_t sc_row = row0 + sc_rr < M ? row0 + sc_rr : int64_t(M) - 1;
    const float *sc_src = absmax + sc_row * nblk;
    u32x4 wstage[WImg::kInstr];
    float amstage;
    auto issue_staged = [&](int pass) {  // the weight stream (HBM), then the scale; branch-free, a unit past the end is clamped
        const int u = pass * 8 + wave;
        const int s0 = (u < nunits ? u : nunits - 1) * NS;
#pragma unroll
        for (int i = 0; i < WImg::kInstr; ++i) wstage[i] = __builtin_nontemporal_load(WImg::fetch_unit(W, i, lane, row0, M, K, s0));
        // first weight of the lane's group: 64 * (s0 + sc_g * gsteps); its block is that >> bshift (< nblk: s0 + NS <= K / 64)
        amstage = sc_src[(64 * (s0 + sc_g * (gmask + 1))) >> bshift];
    };
    // the x fragments of one step: rows past B are clamped (computed, never stored)
    int64_t xrow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = 16 * nt + r;
        xrow[nt] = int64_t(n < B ? n : B - 1) * K + 8 * kb;
    }
    auto load_x = [&](u32x4 (&xr)[NT][2], int step) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t e = (xrow[nt] + 64 * int64_t(step)) >> 3;
            xr[nt][0] = x4[e];
            xr[nt][1] = x4[e + 4];
        }
    };
    issue_staged(0);

    // the byte table, once per workgroup, while the first pass's loads fly
    fill_code_table<DT>(s_code, tid);
    __syncthreads();
    const uint8_t *code = reinterpret_cast<const uint8_t *>(s_code);
    uint8_t *img = WImg::at(s_raw, wave);

    f32x4 acc[RT][NT], tile[RT][NT], tile_lo[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = tile[rt][nt] = tile_lo[rt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int p = 0; p < passes; ++p) {
        const int u = p * 8 + wave;
        const bool active = u < nunits;  // wave-uniform
        const int s0 = (active ? u : nunits - 1) * NS;
        u32x4 xcur[NT][2];
        load_x(xcur, s0);
        if (p > 0) __builtin_amdgcn_wave_barrier();  // the previous pass's reads are done before the image is rewritten
#pragma unroll
        for (int i = 0; i < WImg::kInstr; ++i) {
            const int rr = WImg::fetch_row(i, lane);
            if (WImg::inside(rr)) *WImg::unit(img, rr, lane) = wstage[i];
        }
        WImg::scales(img, sc_rr)[sc_g] = amstage;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (p + 1 < passes) issue_staged(p + 1);  // uniform; flies while this pass is decoded and multiplied
        if (!active) continue;

#pragma unroll 1
        for (int j = 0; j < NS; ++j) {
            u32x4 xnext[NT][2];
            if (j + 1 < NS) load_x(xnext, s0 + j + 1);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                uint8_t *wrow = WImg::row(img, 16 * rt + r);
                const uint32_t wq[2] = {*WImg::frag4(wrow, j, kb, 0), *WImg::frag4(wrow, j, kb, 1)};
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const HiLoFrag w = decode8_hi_lo(code, wq[t]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        tile[rt][nt] = mfma16<DT>(xcur[nt][t], w.hi, tile[rt][nt]);
                        if constexpr (kLoShift<DT> == 0)
                            tile[rt][nt] = mfma16<DT>(xcur[nt][t], w.lo, tile[rt][nt]);
                        else
                            tile_lo[rt][nt] = mfma16<DT>(xcur[nt][t], w.lo, tile_lo[rt][nt]);
                    }
                }
            }
            if ((j & gmask) == gmask) {  // wave-uniform: the group's last step - one scale for everything chained since the last fold
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const float am = WImg::scales(img, 16 * rt + r)[j >> (NS == 4 ? 2 - glog : 1)];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const f32x4 v = fold_lo<DT>(tile[rt][nt], tile_lo[rt][nt]);
                        acc[rt][nt].x = __builtin_fmaf(v.x, am, acc[rt][nt].x);
                        acc[rt][nt].y = __builtin_fmaf(v.y, am, acc[rt][nt].y);
                        acc[rt][nt].z = __builtin_fmaf(v.z, am, acc[rt][nt].z);
                        acc[rt][nt].w = __builtin_fmaf(v.w, am, acc[rt][nt].w);
                        tile[rt][nt] = tile_lo[rt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    }
                }
            }
            if (j + 1 < NS) {
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
        const int tl = idx >> 8, e = idx & 255;
        const int wr = e & 15, n_l = e >> 4;
        const int src = tl * 256 + (((n_l >> 2) * 16 + wr) << 2) + (n_l & 3);  // lane (n_l >> 2) * 16 + wr, register n_l & 3
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) t += s_part[w][src];
        const int n = 16 * (tl % NT) + n_l;
        const int64_t row = row0 + 16 * (tl / NT) + wr;
        if (mode & kModeSiluMulPairs) {
            if (!(wr & 1)) {  // an even weight row of the tile (gate); its up row is the next lane's column: src + 4
                float up = 0.0f;
#pragma unroll
                for (int w = 0; w < 4; ++w) up += s_part[w][src + 4];
                if (row < M && n < B) store_nf4_pair<DT, false>(out, bias, residual, nullptr, nullptr, 0, n, row, M, t, up);
            }
        } else if (row < M && n < B) {
            store_small<DT>(out, bias, residual, n, (int)row, M, t);
        }
    }
}

std::atomic<int> g_blocks_nf4_variant{-1};  // sweep hook: 1 / 2 = 16 / 32 weight rows per workgroup, anything else = the heuristic

int log2_exact(int v) {
    int s = 0;
    while ((1 << s) < v) ++s;
    return s;
}

template <int DT, int NT, int RT, int NS>
void launch_blocks_nf4(const Nf4Call &a) {
    hipLaunchKernelGGL((gemm_blocks_nf4_kernel<DT, NT, RT, NS>), dim3((unsigned)((a.M + 16 * RT - 1) / (16 * RT))), dim3(512), 0, a.stream,
                       static_cast<const uint16_t *>(a.x), a.W, static_cast<const float *>(a.scales), static_cast<const uint16_t *>(a.bias),
                       static_cast<uint16_t *>(a.out), (int)a.B, (int)a.M, (int)a.K, log2_exact(a.blocksize),
                       static_cast<const uint16_t *>(a.residual), a.mode);
}

template <int DT, int NT>
void dispatch_blocks_nf4_nt(const Nf4Call &a) {
    // 32 weight rows per workgroup once that still fills three quarters of the chip: gemm_wide_nf4.hip's rule
    const int v = g_blocks_nf4_variant.load(std::memory_order_relaxed);
    const bool rt2 = v == 2 || (v != 1 && a.M >= 24 * device_cu_count());
    const bool ns4 = a.K % 256 == 0;  // otherwise K = 128 * odd at blocksize 128: units of one block
    if (rt2) {
        if (ns4) return launch_blocks_nf4<DT, NT, 2, 4>(a);
        return launch_blocks_nf4<DT, NT, 2, 2>(a);
    }
    if (ns4) return launch_blocks_nf4<DT, NT, 1, 4>(a);
    return launch_blocks_nf4<DT, NT, 1, 2>(a);
}

// one launch of a validated call: 1..64 rows, NT = ceil(B / 16) column tiles, the last one ragged
void dispatch_blocks_nf4(const Nf4Call &a) {
    with_dtype(a.dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        switch ((a.B + 15) / 16) {
            case 1: return dispatch_blocks_nf4_nt<DT, 1>(a);
            case 2: return dispatch_blocks_nf4_nt<DT, 2>(a);
            case 3: return dispatch_blocks_nf4_nt<DT, 3>(a);
            default: return dispatch_blocks_nf4_nt<DT, 4>(a);
        }
    });
}

// nf4_check_args' sibling for the block sizes above 64 (that one's messages are pinned, and say "blocksize 64"): FP4_OK, or the status
// to return with the message set.  An empty problem is FP4_OK whatever the pointers are: the caller returns on it before it launches.
int nf4_blocks_check_args(const char *name, const Nf4Call &c) {
    if (c.B < 0 || c.M < 0 || c.K <= 0 || c.blocksize <= 0) {
        set_error("%s: B=%lld M=%lld K=%lld blocksize=%d (need B, M >= 0, K, blocksize > 0)", name, (long long)c.B, (long long)c.M,
                  (long long)c.K, c.blocksize);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (c.gated() && (c.M & 1)) {
        set_error("%s: the gate|up epilogue needs an even row count, got M=%lld", name, (long long)c.M);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (c.blocksize == 64) {  // each block size has one kernel that owns it
        set_error("%s: blocksize 64 is not covered here; it is fp4_hip_gemm_fused_nf4's", name);
        return FP4_ERR_UNSUPPORTED;
    }
    const uintptr_t align = reinterpret_cast<uintptr_t>(c.W) | reinterpret_cast<uintptr_t>(c.x);
    const bool bs_ok = c.blocksize >= 128 && c.blocksize <= 4096 && (c.blocksize & (c.blocksize - 1)) == 0 && c.K % c.blocksize == 0;
    // the kernel addresses with 64-bit offsets: M * K may pass 2^32; the bounds keep the int step / block arithmetic in range
    if (c.B > 64 || !bs_ok || (c.dtype != FP4_DTYPE_F16 && c.dtype != FP4_DTYPE_BF16) || (align & 15u) != 0 || c.M > (int64_t(1) << 30) ||
        c.K > (int64_t(1) << 24)) {
        set_error("%s: B=%lld M=%lld K=%lld blocksize=%d dtype=%d is not covered (1..64 rows, a power-of-two blocksize in 128..4096 "
                  "dividing K, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM",
                  name, (long long)c.B, (long long)c.M, (long long)c.K, c.blocksize, c.dtype);
        return FP4_ERR_UNSUPPORTED;
    }
    if (c.M == 0 || c.B == 0) return FP4_OK;
    if (!c.x || !c.W || !c.scales || !c.out) {
        set_error("%s: null pointer", name);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    return FP4_OK;
}

}  // namespace

void set_blocks_nf4_variant(int v) { g_blocks_nf4_variant.store(v, std::memory_order_relaxed); }

}  // namespace fp4

extern "C" int fp4_hip_gemm_blocks_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                       void *out, int64_t B, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream) {
    const char *name = "fp4_hip_gemm_blocks_nf4";
    const int mode = fp4::epilogue_mode(name, epilogue);
    if (mode < 0) return FP4_ERR_INVALID_ARGUMENT;
    const fp4::Nf4Call c{.x = x, .W = packed, .scales = absmax, .bias = bias, .residual = residual, .out = out, .B = B, .M = M, .K = K,
                         .blocksize = blocksize, .dtype = dtype, .mode = mode, .fused = true, .stream = static_cast<hipStream_t>(stream)};
    if (const int rc = fp4::nf4_blocks_check_args(name, c)) return rc;
    if (M == 0 || B == 0) return FP4_OK;
    fp4::dispatch_blocks_nf4(c);
    return fp4::check_launch(name);
}
