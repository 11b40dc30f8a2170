// The host side that the NF4 decode entry points share (gemv_nf4.hip: one row; gemm_small_nf4.hip, gemm_wide_nf4.hip: the matrix
// cores): one call descriptor, the fan-out from its runtime form and dtype to the kernels' template flags, and the argument checks.
//
// An extern "C" entry point fills an Nf4Call by member name and hands it to its entry function as entry(name, call).  What kind
// of call it is - plain, FUSED, with an adapter (LORA), with a stack of adapters (MULTI), with double-quantised statistics (NESTED) -
// is read off the descriptor by lora() / multi() / nested() and turned into template flags in ONE place, with_nf4_form(), which
// offers the six forms the kernels are built in and no other.  Each dispatcher's callable takes the form as a type and spells its
// kernel's own flag order once (the kernels order their trailing flags differently; that is device text and stays).
//
// How to add a form: give the descriptor its operands (a part with a `given` flag), add the flag to Nf4Form and its rule to the
// static_assert there, add the branch to with_nf4_form(), pass the new kernel arguments in the three launch_* functions, and fill the
// part in the new extern "C" functions.  The entry functions change only where the form needs a check of its own.
#pragma once

#include "fp4_call.h"  // with_dtype, epilogue_mode: shared with the FP4 half
#include "lora_nf4.h"
#include "nested_absmax.h"

namespace fp4 {

struct Nf4Call {
    const void *x = nullptr;  // [B][K] of dtype
    const uint8_t *W = nullptr;
    const void *scales = nullptr;  // one per block: float absmax, or with nested.given the uint8 codes of the compressed statistics
    const void *bias = nullptr, *residual = nullptr;
    void *out = nullptr;
    int64_t B = 1, M = 0, K = 0;  // B activation rows (the GEMV: 1)
    int blocksize = 0, dtype = 0;
    int mode = 0;        // 0 or kModeSiluMulPairs
    bool fused = false;  // the entry point takes a residual and an epilogue: the FUSED kernels, also with neither given
    hipStream_t stream = nullptr;
    struct Adapter {
        bool given = false, stack = false;  // stack: B holds n_adapters arrays T[M][R] and ids[b] names the one of activation row b
        const void *B = nullptr;
        const float *t = nullptr;
        int64_t R = 0;
        const int32_t *ids = nullptr;
        int64_t n_adapters = 0;
    } adapter = {};
    struct Nested {
        bool given = false;
        const float *group = nullptr, *table = nullptr;  // one scale per 256 blocks, the 256-entry table
        float offset = 0.0f;
    } nested_stats = {};

    bool lora() const { return adapter.given; }
    bool multi() const { return adapter.given && adapter.stack; }
    bool nested() const { return nested_stats.given; }
    bool gated() const { return mode & kModeSiluMulPairs; }
};

// a form as a type: what with_nf4_form() hands to its callable.  The one statement on the host of which forms exist.
enum : unsigned { kNf4Fused = 1, kNf4Lora = 2, kNf4Multi = 4, kNf4Nested = 8 };
template <unsigned BITS>
struct Nf4Form {
    static constexpr bool fused = BITS & kNf4Fused, lora = BITS & kNf4Lora, multi = BITS & kNf4Multi, nested = BITS & kNf4Nested;
    static_assert((!lora || fused) && (!multi || lora) && (!nested || (fused && !multi)),
                  "the adapter term comes with the fused epilogues, the stack with the adapter term, nested absmax with the fused "
                  "epilogues and without the stack");
};

// runtime form -> template flags: f(Nf4Form<...>{}) for the one form of the six that the descriptor has
template <typename F>
inline void with_nf4_form(const Nf4Call &c, F &&f) {
    if (c.nested())
        c.lora() ? f(Nf4Form<kNf4Fused | kNf4Lora | kNf4Nested>{}) : f(Nf4Form<kNf4Fused | kNf4Nested>{});
    else if (c.multi())
        f(Nf4Form<kNf4Fused | kNf4Lora | kNf4Multi>{});
    else if (c.lora())
        f(Nf4Form<kNf4Fused | kNf4Lora>{});
    else
        c.fused ? f(Nf4Form<kNf4Fused>{}) : f(Nf4Form<0>{});
}

// The adapter's own check, after the operands': FP4_OK (also without an adapter), or the status to return with the message set
inline int nf4_check_adapter(const char *name, const Nf4Call &c) {
    const Nf4Call::Adapter &a = c.adapter;
    if (c.multi()) return lora_check_stack(name, a.B, a.ids, a.n_adapters, a.t, a.R);
    return c.lora() ? lora_check_adapter(name, a.B, a.t, a.R) : FP4_OK;
}

// The argument check of the NF4 matrix-core entry points: FP4_OK, or the status to return with the message set.  An empty problem
// (M == 0 or B == 0) is FP4_OK whatever the pointers are: the caller returns on it before it launches.
inline int nf4_check_args(const char *name, const Nf4Call &c, int max_rows, int k_multiple) {
    if (c.B < 0 || c.M < 0 || c.K <= 0 || c.blocksize <= 0 || (c.lora() && c.adapter.R < 0)) {
        set_error("%s: B=%lld M=%lld K=%lld blocksize=%d (need B, M >= 0, K, blocksize > 0)", name, (long long)c.B, (long long)c.M,
                  (long long)c.K, c.blocksize);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (c.gated() && (c.M & 1)) {
        set_error("%s: the gate|up epilogue needs an even row count, got M=%lld", name, (long long)c.M);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    const uintptr_t align = reinterpret_cast<uintptr_t>(c.W) | reinterpret_cast<uintptr_t>(c.x);
    // the kernels address with 64-bit element offsets: M * K may pass 2^32; the bounds keep the int row / block arithmetic in range
    if (c.B > max_rows || c.blocksize != 64 || (c.K % k_multiple) != 0 || (c.dtype != FP4_DTYPE_F16 && c.dtype != FP4_DTYPE_BF16) ||
        (align & 15u) != 0 || c.M > (int64_t(1) << 30) || c.K > (int64_t(1) << 24)) {
        set_error("%s: B=%lld M=%lld K=%lld blocksize=%d dtype=%d is not covered (1..%d rows, blocksize 64, "
                  "K %% %d == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM",
                  name, (long long)c.B, (long long)c.M, (long long)c.K, c.blocksize, c.dtype, max_rows, k_multiple);
        return FP4_ERR_UNSUPPORTED;
    }
    if (c.M == 0 || c.B == 0) return FP4_OK;
    if (!c.x || !c.W || !c.scales || !c.out || (c.lora() && (!c.adapter.B || !c.adapter.t))) {
        set_error("%s: null pointer", name);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    return FP4_OK;
}

// The first check of the entry points that read the statistics compressed, ahead of the un-nested twin's own: the epilogue (into
// c.mode), then the statistics.  FP4_OK, or the status to return with the message set.  `kind` is what reads the groups ("GEMV",
// "GEMM"), `plain_op` the entry point to run on the expanded statistics instead.
inline int nested_check_args(const char *name, const char *kind, const char *plain_op, int epilogue, int nested_blocksize, Nf4Call &c) {
    if ((c.mode = epilogue_mode(name, epilogue)) < 0) return FP4_ERR_INVALID_ARGUMENT;
    if (nested_blocksize <= 0) {
        set_error("%s: nested_blocksize=%d (need a positive group size)", name, nested_blocksize);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (c.B > 0 && c.M > 0 && c.K > 0 && (!c.nested_stats.group || !c.nested_stats.table)) {  // the codes are checked with the other operands
        set_error("%s: null pointer", name);
        return FP4_ERR_INVALID_ARGUMENT;
    }
    if (nested_blocksize != (1 << kNestedGemvShift)) {
        set_error("%s: nested_blocksize %d is not covered (the %s reads groups of 256 blocks); expand the statistics with "
                  "fp4_hip_absmax_unnest and run %s", name, nested_blocksize, kind, plain_op);
        return FP4_ERR_UNSUPPORTED;
    }
    return FP4_OK;
}

}  // namespace fp4
