"""(shape, rows) cases of the fused NF4 epilogue tests (tests/test_gpu_nf4_fused.py); tests/test_nf4_fused_host.py shows, without a
GPU, that they reach every cell of the two dispatchers (nf4_ref.gemv_cell, nf4_wide_cases.cells)."""
import nf4_ref as R
import nf4_wide_cases as C

# batch 1, plain epilogue: the GEMV's own cell cases (odd M allowed)
GEMV_PLAIN = list(R.GEMV_CELL_CASES)

# batch 1, gate|up epilogue: even M, each in the cell of its original; a row tail is 2 rows = one pair
GEMV_GATED = [
    (64, 1024), (1022, 992), (4096, 1024), (4098, 800), (8192, 512), (8194, 736),            # ks 1, G 1, iters 1 / 2 / 4
    (256, 2048), (2046, 1056), (2048, 2048), (2050, 1600), (4096, 2048), (4098, 1088),       # ks 2, G 1
    (512, 4096), (1022, 2080), (1024, 4096), (1026, 3104), (2048, 4096), (2050, 4064),       # ks 4, G 1
    (512, 8224), (1022, 32768), (1024, 14336), (1026, 8224), (2048, 32768), (4098, 4128),    # ks 4, G 2
]

# one shape per K band count for the two table layouts
GEMV_VARIANT_SHAPES = [(1022, 992), (2046, 1056), (1026, 3104), (1026, 8224)]

# 2..128 rows: nf4_wide_cases.SHAPES with odd M raised by one (the gated epilogue needs pairs)
BATCH_SHAPES = [(M + (M & 1), K) for M, K in C.SHAPES]
ROWS_WIDE = [17, 33, 48, 64, 65, 128]
ROWS_SMALL_KERNEL = [2, 5, 16]  # K % 512 == 0: forwarded to the 2..16-row kernel
ROWS_ONE_TILE = [1, 2, 16]      # K % 512 != 0: the one-tile form of the wide kernel


def rows_for(K):
    return ROWS_WIDE + (ROWS_SMALL_KERNEL if K % 512 == 0 else ROWS_ONE_TILE)
