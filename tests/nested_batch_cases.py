"""Cases and ctypes bindings of the entry points that read double-quantised absmax in the 1..64-row kernels and beside an adapter
(fp4_hip_gemm_nested_nf4, fp4_hip_gemm_lora_nested_nf4, fp4_hip_gemv_lora_nested_nf4), shared by tests/test_nested_batch_host.py and
tests/test_gpu_nested_batch.py.  The dispatchers of csrc/gemm_small_nf4.hip and csrc/gemm_wide_nf4.hip are restated here; no GPU needed."""
import ctypes

import nf4_wide_cases as WC

CUS = WC.CUS

# ---- the small-batch kernel (1..16 rows, K % 512 == 0): (NBW, XS) ---------------------------------------------------------------------
SMALL_K = [2048, 1024, 512]          # quant blocks per wave over the whole K: 4 / 2 / 1 -> NBW 4 / 2 / 1
SMALL_ROWS = [2, 4, 5, 8, 9, 16]     # x staged for <= 4 rows, for 5..8 rows, not at all
SMALL_M = [16, 33]                   # one whole tile; two tiles and a row tail
SMALL_M_GATED = [16, 34]             # the gate|up epilogue needs an even row count: the tail is one pair
ALL_SMALL_CELLS = {(4, 4), (4, 8), (4, 0), (2, 0), (1, 0)}


def small_cell(rows, M, K, cus=CUS):
    """dispatch_nf4_mfma: (quant blocks per wave and pass, activation rows staged per wave in LDS)."""
    assert 1 <= rows <= 16 and K % 512 == 0
    units, blocks = K // 512, -(-M // 16)
    if units % 4 == 0:
        if rows <= 4:
            return 4, 4
        if rows <= 8 and blocks <= cus:
            return 4, 8
        return 4, 0
    return (2, 0) if units % 2 == 0 else (1, 0)


# ---- the wide kernel: (NT, RT, NBW); RT through the sweep hook fp4_hip_set_variant("gemm_wide_nf4", 1 / 2) ----------------------------
WIDE_K = [768, 320]                  # K % 256 == 0 -> NBW 4 (and K % 512 != 0, so one row stays here); else NBW 1
WIDE_ROWS = [1, 17, 33, 48, 64]      # NT 1, 2, 3, 3, 4
WIDE_M = 33                          # RT 1: two tiles and a tail; RT 2: one workgroup and a tail
WIDE_M_GATED = 34
CHUNKED = [(65, 33, 768), (128, 34, 320)]  # (rows, M, K): two launches through the C ABI


def wide_cell(rows, K, variant):
    nt, _, nbw = WC.cell(rows, WIDE_M, K)
    return nt, variant, nbw


# ---- group geometry: (rows, M, K, what) -----------------------------------------------------------------------------------------------
GEOMETRY = [
    (17, 17, 32768, "two groups per row: a boundary inside every row (wide kernel)"),
    (2, 17, 32768, "two groups per row (small kernel)"),
    (8, 33, 1536, "a boundary inside a tile, mid-row; 33 * 24 blocks is no multiple of 256; a row tail (small kernel)"),
    (17, 64, 320, "a boundary inside a tile, mid-row: 5 blocks per row (wide kernel)"),
    (3, 16, 512, "a single partial group: 128 blocks"),
]

OFFSETS = [-0.0173, 0.0, 0.031]

# ---- LoRA -----------------------------------------------------------------------------------------------------------------------------
LORA_ROWS = [2, 8, 40]
LORA_RANKS = [8, 24]
LORA_SHAPES = [(34, 1024), (34, 320)]  # the small kernel (2, 8 rows) and the wide one (40 rows; every row count where K % 512 != 0)


def lib():
    import hipabi

    l = hipabi.lib()
    if not getattr(l, "_nested_batch_bound", False):
        vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
        # (x, packed, absmax_u8, nested_absmax, code256, offset, nested_blocksize, bias, residual, [lora_B, t, R,] out, [B,] M, K, blocksize,
        #  dtype, epilogue, stream)
        l.fp4_hip_gemm_nested_nf4.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemm_nested_nf4.restype = i32
        l.fp4_hip_gemm_lora_nested_nf4.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, i64, vp, i64, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemm_lora_nested_nf4.restype = i32
        l.fp4_hip_gemv_lora_nested_nf4.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, i64, vp, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemv_lora_nested_nf4.restype = i32
        l._nested_batch_bound = True
    return l
