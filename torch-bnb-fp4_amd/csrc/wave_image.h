// The wave-private LDS images of the 16-row-tile matrix-core kernels - gemm16_mfma_kernel, gemm16_mfma_persist_kernel (gemm_small_fp4.hip),
// gemm_nf4_mfma_kernel (gemm_small_nf4.hip), gemm_wide_nf4_kernel (gemm_wide_nf4.hip) - defined once: writer and reader of an image take
// every constant and every address from here; the loops that fetch, write and read the scales back stay in the kernels, where alone
// they keep each kernel's instruction schedule (profiles/wave_image_layout.txt).  gemm_wide_fp4.hip / gemm_splitk_fp4.hip: another layout.
//
// Weight image.  The MFMA fragment of a weight wants 8 bytes per lane from 16 different rows (32-byte segments per row per load
// instruction); instead each wave pulls its ROWS x (32*NBW)-byte region - NBW 64-weight quant blocks of ROWS rows - with row-contiguous
// 16-byte loads (2*NBW lanes per row, 64 / (2*NBW) rows per instruction) and re-reads it from a wave-private LDS image: no workgroup
// barrier, a wave barrier between its own writes and reads.  Each image row is followed by that row's NBW block scales: the accumulator
// layout needs the scales of 4 rows x NBW blocks per lane, the same values in 16 lanes, so they are fetched once per wave and re-read
// from LDS as broadcasts instead of 8 x 16-byte global loads per lane and tile.  Row stride 32*NBW + 32 bytes: the 8-byte fragment reads
// of 16 rows x 4 k-groups fall on distinct banks per half-wave.
//
// x image (batch <= XS, XS in {4, 8}).  The other operand wants 32 bytes per lane from 16 activation rows, of which only `batch` are real
// - loaded straight from global every 16-row workgroup would pull 16 / batch times its share of x through the texture path (4x the weight
// stream at batch 4).  Instead the wave copies the XS x (64*NBW) activations of its K slice into a wave-private image with row-contiguous
// 16-byte loads (8*NBW units per row) and reads the fragments from there; lanes of the unused columns read a real row (r & (XS - 1):
// broadcast, results never stored).  Row stride 128*NBW + 16 bytes: consecutive rows start four banks apart, so the 16-byte fragment
// reads of the XS rows do not meet on one bank.
#pragma once

#include "mfma_common.h"

namespace fp4 {
namespace {

// ROWS = the rows a wave fetches as one group: 16 (one tile; a wave keeps one image per row tile) or 32 (gemm_wide_nf4_kernel: two tiles as one)
template <int NBW, int ROWS = 16>
struct WeightImage {
    static_assert((ROWS & (ROWS - 1)) == 0, "a row past the image wraps with a mask");
    static constexpr int kStride = 32 * NBW + 32, kBytes = ROWS * kStride;
    static constexpr int kLanesPerRow = 2 * NBW, kRowsPerInstr = 64 / kLanesPerRow, kInstr = (ROWS + kRowsPerInstr - 1) / kRowsPerInstr;
    // the image of `wave`'s row tile `tile` in storage that holds 8 * TILES images back to back
    template <int TILES = 1>
    static __device__ __forceinline__ uint8_t *at(uint8_t *base, int wave, int tile = 0) { return base + (wave * TILES + tile) * ROWS * kStride; }
    // the row whose 16-byte unit `lane` fetches with load instruction i: with NBW = 1 the instructions cover more rows than the image has
    static __device__ __forceinline__ int fetch_row(int i, int lane) { return i * kRowsPerInstr + lane / kLanesPerRow; }
    static __device__ __forceinline__ bool inside(int rr) { return rr < ROWS; }
    // that unit in the packed weight, blocks b0 .. b0 + NBW of weight row row0 + fetch_row: a row past the image wraps (the same address
    // again, written only if inside), a row past M is clamped (computed, never stored)
    template <typename R>
    static __device__ __forceinline__ const u32x4 *fetch_unit(const uint8_t *W, int i, int lane, R row0, int M, int K, int b0) {
        const int rr = fetch_row(i, lane) & (ROWS - 1);
        const int64_t row = row0 + rr < M ? row0 + rr : R(M) - 1;
        return reinterpret_cast<const u32x4 *>(W) + ((row * K) >> 5) + 2 * b0 + (lane % kLanesPerRow);
    }
    // ... and in the image, rr = fetch_row(i, lane)
    static __device__ __forceinline__ uint8_t *row(uint8_t *img, int rr) { return img + rr * kStride; }
    static __device__ __forceinline__ u32x4 *unit(uint8_t *img, int rr, int lane) { return reinterpret_cast<u32x4 *>(row(img, rr) + 16 * (lane % kLanesPerRow)); }
    // lane (r, kb)'s fragment of block j in decode8's k order (FP4, 2..16-row NF4): the 8 bytes [8kb, 8kb + 8) of the block
    static __device__ __forceinline__ const u32x2 *frag8(uint8_t *img, int r, int j, int kb) { return reinterpret_cast<const u32x2 *>(row(img, r) + 32 * j + 8 * kb); }
    static __device__ __forceinline__ void read_frags(uint8_t *img, int r, int kb, u32x2 (&wq)[NBW]) {
#pragma unroll
        for (int j = 0; j < NBW; ++j) wq[j] = *frag8(img, r, j, kb);
    }
    // ... in natural k order (gemm_wide_nf4_kernel): instruction t takes the dword [16t + 4kb, 16t + 4kb + 4) of the image row at `wrow`
    static __device__ __forceinline__ const uint32_t *frag4(uint8_t *wrow, int j, int kb, int t) {
        return reinterpret_cast<const uint32_t *>(wrow + 32 * j + 16 * t + 4 * kb);
    }
    // the NBW block scales behind the bytes of the image row at `wrow` / of image row rr
    static __device__ __forceinline__ float *row_scales(uint8_t *wrow) { return reinterpret_cast<float *>(wrow + 32 * NBW); }
    static __device__ __forceinline__ float *scales(uint8_t *img, int rr) { return row_scales(row(img, rr)); }
};

template <int NBW, int XS>
struct XImage {
    static_assert(XS == 0 || ((XS * NBW) % 8 == 0 && (XS & (XS - 1)) == 0), "x staging: whole 16-byte units per lane");
    static constexpr int kStride = 128 * NBW + 16, kBytes = XS * kStride;
    static constexpr int kUnits = XS ? XS * NBW / 8 : 1;  // 16-byte units of the image per lane
    static __device__ __forceinline__ uint8_t *at(uint8_t *base, int wave) { return base + wave * kBytes; }
    // unit i of `lane`: its activation row and its 16-byte column in the wave's K slice (64 * NBW activations a row)
    static __device__ __forceinline__ int unit_row(int i, int lane) { return (i * 64 + lane) / (8 * NBW); }
    static __device__ __forceinline__ int unit_col(int i, int lane) { return (i * 64 + lane) % (8 * NBW); }
    static __device__ __forceinline__ u32x4 *unit(uint8_t *ximg, int n, int c16) { return reinterpret_cast<u32x4 *>(ximg + n * kStride + 16 * c16); }
    // lane (r, kb)'s fragment t = 0, 1 of block j: x[r][64j + 16kb + 8t ..]
    static __device__ __forceinline__ const u32x4 *frag(uint8_t *ximg, int r, int j, int kb, int t) {
        return reinterpret_cast<const u32x4 *>(ximg + (r & (XS - 1)) * kStride + 128 * j + 32 * kb + 16 * t);
    }
};

}  // namespace
}  // namespace fp4
