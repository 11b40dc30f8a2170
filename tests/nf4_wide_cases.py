"""The dispatcher of fp4_hip_gemm_wide_nf4 (csrc/gemm_wide_nf4.hip) restated, and the (shape, rows) cases the GPU suite runs.
No GPU needed: tests/test_nf4_wide_batch_host.py checks that the cases reach every cell of the rule."""

CUS = 256  # compute units of an MI355X


def chunks(B):
    """Activation rows of each launch: 1..64 in one, 65..128 as two even chunks of at most 64."""
    if B <= 64:
        return [B]
    first = (B + 1) // 2
    return [first, B - first]


def cell(rows, M, K, cus=CUS):
    """One launch of `rows` <= 64 activation rows: (column tiles NT, 16-row weight tiles per workgroup RT, quant blocks per wave and
    pass NBW), or "small" where the call is forwarded to fp4_hip_gemm_small_nf4."""
    assert 1 <= rows <= 64 and K % 64 == 0
    nt = -(-rows // 16)
    rt = 2 if M >= 24 * cus else 1
    nbw = 4 if K % 256 == 0 else 1
    return nt, rt, nbw


def cells(B, M, K, cus=CUS):
    if B <= 16 and K % 512 == 0:
        return ["small"]
    return [cell(rows, M, K, cus) for rows in chunks(B)]


def ragged_last_pass(K):
    """The eight waves take one unit of NBW blocks each per pass: a last pass with idle waves."""
    nbw = 4 if K % 256 == 0 else 1
    return (K // 64 // nbw) % 8 != 0


ALL_CELLS = {(nt, rt, nbw) for nt in (1, 2, 3, 4) for rt in (1, 2) for nbw in (1, 4)}

ROWS_WIDE = [17, 18, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 127, 128]
ROWS_SMALL = [1, 2, 5, 16]  # run where K % 512 != 0: the one-tile form of the wide kernel

# (M, K): 4096 x 4096; one block; a ragged last pass with one block per wave (9 units) and with four (43, 5 and 3 units); M below and
# off the 16-row and the 32-row tile; K = 11008 and 14336; both workgroup shapes (32 rows per workgroup from M = 6144 on)
SHAPES = [(4096, 4096), (100, 64), (33, 576), (48, 11008), (40, 14336), (7, 1280), (16400, 768), (16390, 320), (257, 2048)]


def rows_for(K):
    return ROWS_WIDE + (ROWS_SMALL if K % 512 != 0 else [])
