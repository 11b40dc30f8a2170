"""Cases and ctypes bindings of the multi-adapter LoRA entry points (fp4_hip_lora_down_multi, fp4_hip_gemm_lora_multi_nf4,
fp4_hip_gemv_lora_multi_nf4) shared by tests/test_nf4_multi_lora_host.py and tests/test_gpu_nf4_multi_lora.py."""
import ctypes

import nf4_lora_cases as LC

N_ADAPTERS = 3
INT32_MAX = 2**31 - 1

# rows on either side of the 4 rows whose loads fly together and of the 8 rows a workgroup of the down kernel takes, of the 16-column
# tiles of the batched kernels, and the most the fused route covers
ROWS = [1, 5, 9, 17, 64]
DOWN_K = [32, 992, 8224]  # below one unit per wave, a ragged single pass, more than one pass
RANKS = [8, 64]

# the five batched shapes: the 2..16-row kernel, the one-tile form and 2..4 column tiles (all of nf4_fused_cases.BATCH_SHAPES)
BATCH_SHAPES = [(100, 64), (34, 576), (258, 2048), (48, 11008), (4096, 4096)]

# ids that name no adapter: negative values, n_adapters itself, the largest int32
NO_ADAPTER = [-1, -7, N_ADAPTERS, INT32_MAX]


def id_patterns(rows, n=N_ADAPTERS):
    """name -> ids for `rows` activation rows over `n` adapters: all equal; sorted runs; an id that changes every row (so it crosses
    the 4-row load groups and the 8-row workgroups of the down kernel and the 16-column tiles of the batched kernels); and a mix
    with ids that name no adapter (-1, -7, n, 2^31 - 1)."""
    mix = [0, -1, n - 1, -7, 1, n, 0, INT32_MAX]
    return {
        "equal": [1 % n] * rows,
        "sorted": [b * n // rows for b in range(rows)],
        "every_row": [b % n for b in range(rows)],
        "with_none": [mix[b % len(mix)] for b in range(rows)],
    }


def valid(i, n=N_ADAPTERS):
    return 0 <= i < n


def lib():
    l = LC.lib()
    if not getattr(l, "_nf4_multi_lora_bound", False):
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        # (x, A_stack, scale_stack, ids, t, Bt, n_adapters, R, K, dtype, stream)
        l.fp4_hip_lora_down_multi.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, i32, vp]
        l.fp4_hip_lora_down_multi.restype = i32
        # (x, packed, absmax, bias, residual, B_stack, ids, n_adapters, t, R, out, B, M, K, blocksize, dtype, epilogue, stream)
        l.fp4_hip_gemm_lora_multi_nf4.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemm_lora_multi_nf4.restype = i32
        # (x, packed, absmax, bias, residual, B_stack, ids, n_adapters, t, R, out, M, K, blocksize, dtype, epilogue, stream)
        l.fp4_hip_gemv_lora_multi_nf4.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemv_lora_multi_nf4.restype = i32
        l._nf4_multi_lora_bound = True
    return l
