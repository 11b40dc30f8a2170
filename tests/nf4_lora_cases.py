"""Cases and ctypes bindings of the LoRA entry points (fp4_hip_lora_down, fp4_hip_gemv_lora_nf4, fp4_hip_gemm_lora_nf4) shared by
tests/test_nf4_lora_host.py and tests/test_gpu_nf4_lora.py."""
import ctypes

import nf4_fused_cases as FC
import nf4_ref as R

# the down kernel: K below one 16-byte unit per wave, a ragged single pass, exactly half a pass, one pass and a bit, four passes;
# every rank band; rows on either side of the 8 rows a workgroup takes and of the 4 whose loads fly together
DOWN_K = [32, 992, 4096, 8224, 32768]
DOWN_R = [8, 24, 64, 256]
DOWN_ROWS = [1, 2, 5, 16, 17, 64]

RANKS = [8, 64]          # every batch-1 / batched shape
RANKS_EXTRA = [24, 256]  # one shape per K band count, both table layouts, with and without bias


def batch_rows(K):
    """nf4_fused_cases.rows_for restricted to the 64 rows the adapter forms cover."""
    return [r for r in FC.rows_for(K) if r <= 64]


def lib():
    l = R.lib()
    if not getattr(l, "_nf4_lora_bound", False):
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        l.fp4_hip_lora_down.argtypes = [vp, vp, vp, vp, i64, i64, i64, i32, vp]
        l.fp4_hip_lora_down.restype = i32
        l.fp4_hip_gemv_lora_nf4.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemv_lora_nf4.restype = i32
        l.fp4_hip_gemm_lora_nf4.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemm_lora_nf4.restype = i32
        l._nf4_lora_bound = True
    return l
