"""The argument check shared by the four NF4 matrix-core entry points (csrc/nf4_mfma.h: fp4_hip_gemm_small_nf4, _wide_nf4,
_fused_nf4, _lora_nf4), through the C ABI and without a GPU: every call below is refused, or found empty, before any HIP call.

Each refusal is compared with the WHOLE message and the status.  The strings were recorded from the library as it was when each entry
point had its own copy of the checks: one check serving four entry points has to reproduce all of them byte for byte, in the same
order and with the same status."""
import ctypes

import pytest

import hipabi

OK, INVALID, UNSUPPORTED = hipabi.OK, hipabi.ERR_INVALID, hipabi.ERR_UNSUPPORTED
F16, F32, BF16 = hipabi.F16, hipabi.F32, hipabi.BF16
NONE, GATED = hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS
D = 0x1000  # a 16-byte aligned non-null "pointer": nothing below dereferences it

#          entry point                 most rows, K multiple, takes an epilogue, takes an adapter
ENTRIES = {"fp4_hip_gemm_small_nf4": (16, 512, False, False),
           "fp4_hip_gemm_wide_nf4": (128, 64, False, False),
           "fp4_hip_gemm_fused_nf4": (128, 64, True, False),
           "fp4_hip_gemm_lora_nf4": (64, 64, True, True)}


def _lib():
    l = hipabi.lib()
    if not getattr(l, "_nf4_mfma_args_bound", False):
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        l.fp4_hip_gemm_small_nf4.argtypes = l.fp4_hip_gemm_wide_nf4.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]
        l.fp4_hip_gemm_fused_nf4.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemm_lora_nf4.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, i32, i32, i32, vp]
        for name in ENTRIES:
            getattr(l, name).restype = i32
        l._nf4_mfma_args_bound = True
    return l


def call(entry, x=D, packed=D, absmax=D, out=D, B=4, M=64, K=512, blocksize=64, dtype=BF16, epilogue=NONE, lora_B=D, t=D, R=8):
    """One call of `entry` with a valid, covered argument list except for what the caller overrides (an epilogue or an adapter
    argument given to an entry point that takes none is dropped)."""
    _, _, has_epilogue, has_adapter = ENTRIES[entry]
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    f = getattr(_lib(), entry)
    if has_adapter:
        return f(p(x), p(packed), p(absmax), None, None, p(lora_B), p(t), R, p(out), B, M, K, blocksize, dtype, epilogue, None)
    if has_epilogue:
        return f(p(x), p(packed), p(absmax), None, None, p(out), B, M, K, blocksize, dtype, epilogue, None)
    return f(p(x), p(packed), p(absmax), None, p(out), B, M, K, blocksize, dtype, None)


def refusals(entry):
    """[(label, keyword arguments of `call`)]: every way the shared check refuses."""
    rows, kmul, has_epilogue, has_adapter = ENTRIES[entry]
    cases = [("negative B", dict(B=-1)),
             ("K = 0", dict(K=0)),
             ("blocksize 32", dict(blocksize=32)),
             ("one row too many", dict(B=rows + 1)),
             ("K off the multiple", dict(K=576 if kmul == 512 else 96)),
             ("f32", dict(dtype=F32)),
             ("misaligned x", dict(x=D + 8)),
             ("null x", dict(x=None))]
    if has_epilogue:
        cases += [("odd M, gate|up", dict(M=63, epilogue=GATED)),
                  ("unknown epilogue", dict(epilogue=7))]
    if has_adapter:
        cases += [("negative R", dict(R=-8)),
                  ("null lora_B", dict(lora_B=None))]
    return cases


# (status, fp4_hip_last_error()) of every refusal, recorded before the four entry points shared their check
EXPECTED = {
    "fp4_hip_gemm_small_nf4": {
        "negative B": (INVALID, "fp4_hip_gemm_small_nf4: B=-1 M=64 K=512 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "K = 0": (INVALID, "fp4_hip_gemm_small_nf4: B=4 M=64 K=0 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "blocksize 32": (UNSUPPORTED, "fp4_hip_gemm_small_nf4: B=4 M=64 K=512 blocksize=32 dtype=2 "
                                      "is not covered (1..16 rows, blocksize 64, K % 512 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "one row too many": (UNSUPPORTED, "fp4_hip_gemm_small_nf4: B=17 M=64 K=512 blocksize=64 dtype=2 "
                                          "is not covered (1..16 rows, blocksize 64, K % 512 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "K off the multiple": (UNSUPPORTED, "fp4_hip_gemm_small_nf4: B=4 M=64 K=576 blocksize=64 dtype=2 "
                                            "is not covered (1..16 rows, blocksize 64, K % 512 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "f32": (UNSUPPORTED, "fp4_hip_gemm_small_nf4: B=4 M=64 K=512 blocksize=64 dtype=1 "
                             "is not covered (1..16 rows, blocksize 64, K % 512 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "misaligned x": (UNSUPPORTED, "fp4_hip_gemm_small_nf4: B=4 M=64 K=512 blocksize=64 dtype=2 "
                                      "is not covered (1..16 rows, blocksize 64, K % 512 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "null x": (INVALID, "fp4_hip_gemm_small_nf4: null pointer"),
    },
    "fp4_hip_gemm_wide_nf4": {
        "negative B": (INVALID, "fp4_hip_gemm_wide_nf4: B=-1 M=64 K=512 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "K = 0": (INVALID, "fp4_hip_gemm_wide_nf4: B=4 M=64 K=0 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "blocksize 32": (UNSUPPORTED, "fp4_hip_gemm_wide_nf4: B=4 M=64 K=512 blocksize=32 dtype=2 "
                                      "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "one row too many": (UNSUPPORTED, "fp4_hip_gemm_wide_nf4: B=129 M=64 K=512 blocksize=64 dtype=2 "
                                          "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "K off the multiple": (UNSUPPORTED, "fp4_hip_gemm_wide_nf4: B=4 M=64 K=96 blocksize=64 dtype=2 "
                                            "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "f32": (UNSUPPORTED, "fp4_hip_gemm_wide_nf4: B=4 M=64 K=512 blocksize=64 dtype=1 "
                             "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "misaligned x": (UNSUPPORTED, "fp4_hip_gemm_wide_nf4: B=4 M=64 K=512 blocksize=64 dtype=2 "
                                      "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "null x": (INVALID, "fp4_hip_gemm_wide_nf4: null pointer"),
    },
    "fp4_hip_gemm_fused_nf4": {
        "negative B": (INVALID, "fp4_hip_gemm_fused_nf4: B=-1 M=64 K=512 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "K = 0": (INVALID, "fp4_hip_gemm_fused_nf4: B=4 M=64 K=0 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "blocksize 32": (UNSUPPORTED, "fp4_hip_gemm_fused_nf4: B=4 M=64 K=512 blocksize=32 dtype=2 "
                                      "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "one row too many": (UNSUPPORTED, "fp4_hip_gemm_fused_nf4: B=129 M=64 K=512 blocksize=64 dtype=2 "
                                          "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "K off the multiple": (UNSUPPORTED, "fp4_hip_gemm_fused_nf4: B=4 M=64 K=96 blocksize=64 dtype=2 "
                                            "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "f32": (UNSUPPORTED, "fp4_hip_gemm_fused_nf4: B=4 M=64 K=512 blocksize=64 dtype=1 "
                             "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "misaligned x": (UNSUPPORTED, "fp4_hip_gemm_fused_nf4: B=4 M=64 K=512 blocksize=64 dtype=2 "
                                      "is not covered (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "null x": (INVALID, "fp4_hip_gemm_fused_nf4: null pointer"),
        "odd M, gate|up": (INVALID, "fp4_hip_gemm_fused_nf4: the gate|up epilogue needs an even row count, got M=63"),
        "unknown epilogue": (INVALID, "fp4_hip_gemm_fused_nf4: unknown epilogue 7"),
    },
    "fp4_hip_gemm_lora_nf4": {
        "negative B": (INVALID, "fp4_hip_gemm_lora_nf4: B=-1 M=64 K=512 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "K = 0": (INVALID, "fp4_hip_gemm_lora_nf4: B=4 M=64 K=0 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "blocksize 32": (UNSUPPORTED, "fp4_hip_gemm_lora_nf4: B=4 M=64 K=512 blocksize=32 dtype=2 "
                                      "is not covered (1..64 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "one row too many": (UNSUPPORTED, "fp4_hip_gemm_lora_nf4: B=65 M=64 K=512 blocksize=64 dtype=2 "
                                          "is not covered (1..64 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "K off the multiple": (UNSUPPORTED, "fp4_hip_gemm_lora_nf4: B=4 M=64 K=96 blocksize=64 dtype=2 "
                                            "is not covered (1..64 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "f32": (UNSUPPORTED, "fp4_hip_gemm_lora_nf4: B=4 M=64 K=512 blocksize=64 dtype=1 "
                             "is not covered (1..64 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "misaligned x": (UNSUPPORTED, "fp4_hip_gemm_lora_nf4: B=4 M=64 K=512 blocksize=64 dtype=2 "
                                      "is not covered (1..64 rows, blocksize 64, K % 64 == 0, fp16 / bf16, 16-byte aligned x and packed); use dequant + GEMM"),
        "null x": (INVALID, "fp4_hip_gemm_lora_nf4: null pointer"),
        "odd M, gate|up": (INVALID, "fp4_hip_gemm_lora_nf4: the gate|up epilogue needs an even row count, got M=63"),
        "unknown epilogue": (INVALID, "fp4_hip_gemm_lora_nf4: unknown epilogue 7"),
        "negative R": (INVALID, "fp4_hip_gemm_lora_nf4: B=4 M=64 K=512 blocksize=64 (need B, M >= 0, K, blocksize > 0)"),
        "null lora_B": (INVALID, "fp4_hip_gemm_lora_nf4: null pointer"),
    },
}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_refusal_has_its_status_and_its_whole_message(entry):
    cases = refusals(entry)
    assert [label for label, _ in cases] == list(EXPECTED[entry]), "a case without a recorded message, or the other way round"
    for label, kw in cases:
        rc = call(entry, **kw)
        assert (rc, hipabi.last_error()) == EXPECTED[entry][label], (entry, label)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_an_empty_problem_is_ok_before_any_pointer_is_looked_at_and_leaves_the_message(entry):
    _, _, has_epilogue, _ = ENTRIES[entry]
    assert call(entry, B=-1) == INVALID
    before = hipabi.last_error()
    assert before == EXPECTED[entry]["negative B"][1]
    nulls = dict(x=None, packed=None, absmax=None, out=None, lora_B=None, t=None)
    for epilogue in (NONE, GATED) if has_epilogue else (NONE,):
        assert call(entry, M=0, epilogue=epilogue, **nulls) == OK
        assert call(entry, B=0, epilogue=epilogue, **nulls) == OK
        assert call(entry, B=0, M=0, epilogue=epilogue, **nulls) == OK
    assert hipabi.last_error() == before
    # ... but only an empty problem the entry point covers: the coverage check comes first
    assert call(entry, M=0, blocksize=32, **nulls) == UNSUPPORTED
    assert hipabi.last_error() == EXPECTED[entry]["blocksize 32"][1].replace("M=64", "M=0")
