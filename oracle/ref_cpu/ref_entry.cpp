// C ABI over the reference's own kernels, run on the CPU through ref_shim.h.  TEST INFRASTRUCTURE ONLY.
//
// The two .inc files are the reference's csrc/dequant_fp4_optimized.cu and csrc/gemv_fp4_optimized.cu up to (not including) their
// first host launcher, byte for byte; oracle/ref_cpu.py writes them into oracle/_ref/ and checks by regular expression that the
// launch geometry restated below is still what the launchers say.  Each file sits in a namespace of its own because both define
// param_large_t and CODE_PARAM.
//
// Built twice: as is (every 16-bit `a * b` and `+=` rounded on its own, the float kernel with -ffp-contract=off), and with
// -DREF_CONTRACT_FMA -ffp-contract=fast -mfma (the per-lane `local_C += a * b` is one multiply-add with one rounding).
#include "ref_shim.h"

#include <algorithm>

namespace ref_dequant_file {
#include "dequant_fp4_optimized.cut.inc"
}
namespace ref_gemv_file {
#include "gemv_fp4_optimized.cut.inc"
}

enum { REF_F16 = 0, REF_F32 = 1, REF_BF16 = 2 };      // oracle/c_oracle.py's dtype codes
enum { REF_KERNEL_CODEBOOK = 0, REF_KERNEL_TREE = 1 };  // oracle/c_oracle.py's table codes

namespace {
int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// dequant_fp4_optimized.cu:175-177 and :215-224:  blocks = CDIV(n, 1024);  kernel<T, 512, 64, 8><<<blocks, 64>>>(..., blocksize / 2, n)
template <class T> void dequant(int kernel, unsigned char *A, float *absmax, T *out, int blocksize, int n) {
    using namespace ref_dequant_file;
    const unsigned blocks = (unsigned)cdiv(n, 1024);
    if (kernel == REF_KERNEL_TREE)
        ref_launch(blocks, 64, [=] { dequantize_blockwise_kernel_fp4<T, 512, 64, 8>(A, absmax, out, (const int)(blocksize / 2), (const int)n); });
    else
        ref_launch(blocks, 64, [=] {
            dequantize_blockwise_codebook_kernel_fp4<T, 512, 64, 8>(A, absmax, out, CODE_PARAM, (const int)(blocksize / 2), (const int)n);
        });
}

// gemv_fp4_optimized.cu:265-266 / :272-274:  num_blocks = CDIV(m, 4);  kernel<T, 128, float><<<num_blocks, 128>>>(m, n, k, A, B,
// absmax, CODE_PARAM, out, lda, ldb, ldc, blocksize), with (:289-294) n = 1, m = lda = ldc = Bshape[0], k = Bshape[1] and
// ldb = CDIV(A.sizes()[1], 2) = CDIV(K, 2) for the [1, K] activation.
template <class T> void gemv16(T *x, unsigned char *B, float *absmax, T *out, int M, int K, int blocksize) {
    using namespace ref_gemv_file;
    ref_launch((unsigned)cdiv(M, 4), 128,
               [=] { gemv_4bit_inference_kernel<T, 128, float>(M, 1, K, x, B, absmax, CODE_PARAM, out, M, cdiv(K, 2), M, blocksize); });
}
void gemv32(float *x, unsigned char *B, float *absmax, float *out, int M, int K, int blocksize) {
    using namespace ref_gemv_file;
    ref_launch((unsigned)cdiv(M, 4), 128,
               [=] { gemv_4bit_inference_kernel_float<float, 128, float>(M, 1, K, x, B, absmax, CODE_PARAM, out, M, cdiv(K, 2), M, blocksize); });
}
}  // namespace

extern "C" {

// 0 = separate roundings, 1 = contracted per-lane multiply-add
int ref_flavour(void) {
#ifdef REF_CONTRACT_FMA
    return 1;
#else
    return 0;
#endif
}

// which_file: 0 = dequant_fp4_optimized.cu, 1 = gemv_fp4_optimized.cu.  The decimal literals as this compiler rounds them.
int ref_code_param(int which_file, float *out16) {
    if (which_file != 0 && which_file != 1) return 1;
    const float *p = which_file == 0 ? ref_dequant_file::CODE_PARAM.param : ref_gemv_file::CODE_PARAM.param;
    std::copy(p, p + 16, out16);
    return 0;
}

// packed: uint8[(n + 1) / 2], absmax: float[ceil(n / blocksize)], out: T[n].
// The kernel reads absmax once per thread BEFORE it knows whether the thread has any byte to load (dequant_fp4_optimized.cu:110,159),
// so the last tile's idle threads index past ceil(n / blocksize).  The operands are therefore copied into buffers that cover whole
// 512-byte tiles; the padding is zero and no output depends on it.
int ref_dequant(int kernel, int dtype, const unsigned char *packed, const float *absmax, void *out, int blocksize, int n) {
    if (n <= 0 || blocksize < 2 || (kernel != REF_KERNEL_CODEBOOK && kernel != REF_KERNEL_TREE)) return 1;
    const long tiles = cdiv(n, 1024);
    std::vector<unsigned char> A((size_t)tiles * 512, 0);
    std::copy(packed, packed + (n + 1) / 2, A.begin());
    std::vector<float> am((size_t)cdiv(tiles * 512, blocksize / 2) + 1, 0.0f);
    std::copy(absmax, absmax + cdiv(n, blocksize), am.begin());
    switch (dtype) {
        case REF_F16: dequant<nv_half>(kernel, A.data(), am.data(), (nv_half *)out, blocksize, n); return 0;
        case REF_BF16: dequant<nv_bfloat16>(kernel, A.data(), am.data(), (nv_bfloat16 *)out, blocksize, n); return 0;
        case REF_F32: dequant<float>(kernel, A.data(), am.data(), (float *)out, blocksize, n); return 0;
    }
    return 1;
}

// x: T[K], packed: uint8[M * K / 2], absmax: float[ceil(M * K / blocksize)], out: T[M].  K % 32 == 0 (the reference's own gate,
// torch_bnb_fp4/__init__.py:593, given blocksize >= 32).
// For M % 4 != 0 the last workgroup's idle warps load absmax[absidx] of rows past M before the `row_B < M` test
// (gemv_fp4_optimized.cu:100-105): packed and absmax are copied into buffers sized for ceil(M / 4) * 4 rows, zero padded.
int ref_gemv(int dtype, const void *x, const unsigned char *packed, const float *absmax, void *out, int M, int K, int blocksize) {
    if (M <= 0 || K <= 0 || K % 32 || blocksize < 1) return 1;
    const long rows = (long)cdiv(M, 4) * 4;
    std::vector<unsigned char> B((size_t)rows * K / 2, 0);
    std::copy(packed, packed + (long)M * K / 2, B.begin());
    std::vector<float> am((size_t)cdiv(rows * K, blocksize) + 1, 0.0f);
    std::copy(absmax, absmax + cdiv((long)M * K, blocksize), am.begin());
    switch (dtype) {
        case REF_F16: gemv16<nv_half>((nv_half *)x, B.data(), am.data(), (nv_half *)out, M, K, blocksize); return 0;
        case REF_BF16: gemv16<nv_bfloat16>((nv_bfloat16 *)x, B.data(), am.data(), (nv_bfloat16 *)out, M, K, blocksize); return 0;
        case REF_F32: gemv32((float *)x, B.data(), am.data(), (float *)out, M, K, blocksize); return 0;
    }
    return 1;
}
}
