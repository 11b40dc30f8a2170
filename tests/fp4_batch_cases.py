"""The dispatcher of fp4_hip_gemm_small / _fused / _ws (1..128 activation rows of fp16 / bf16 against a blocksize-64 FP4 weight,
16-byte aligned operands) restated, and the (shape, rows) cases tests/test_gpu_fp4_batch_dispatch.py runs.  No GPU needed:
tests/test_fp4_batch_dispatch_host.py checks that the cases reach every cell of the rule, that both sides of every threshold land
in different cells and that the kernel sources still state what is restated here.

A cell is what one launch runs:
    ("valu",)                       gemm16_small_kernel (csrc/gemm_small_fp4.hip), up to 8 rows on short K
    ("mfma", rowt, nbw, xstage)     gemm16_mfma_kernel: row tiles per workgroup, quant blocks per wave and pass, x image (4 / 8 rows, 0 = none)
    ("persist", ximg)               gemm16_mfma_persist_kernel (K = 4096): x image for <= 4 / <= 8 rows, 0 = B fragments in registers
    ("wide", nt, cfg)               the one-pass kernels of csrc/gemm_wide_fp4.hip: column tiles, workgroup shape as set_wide_variant names it
    ("splitk", nt, tpw)             gemm16_xstat_kernel + splitk_reduce_kernel (csrc/gemm_splitk_fp4.hip): 16-row tiles per wave
A shape's M is written as a multiple of the device's compute units plus an offset, (mult, off) -> mult * cus + off, so that the
cases mean the same on a partitioned card; (0, m) is an absolute row count."""
from collections import namedtuple

BS = 64


# ---- the sweep hooks (fp4_hip_set_variant) -------------------------------------------------------------------------------------------------
Hooks = namedtuple("Hooks", "small rowt xstage wide_first persist wide_cfg")


def set_small_variant(v):
    """csrc/gemm_small_fp4.hip set_small_variant: (g_small_variant, g_mfma_rowt, g_mfma_xstage, g_small_wide, g_mfma_persist)."""
    small = -1 if v < 0 else (v & 1)
    rowt = 0 if v < 0 else ((v >> 4) & 3)
    rowt = -1 if rowt == 0 else rowt
    xstage = -1 if v < 0 else (0 if (v >> 9) & 1 else 1)
    wide_first = 0 if v < 0 else ((v >> 12) & 1)
    p = (v >> 10) & 3
    persist = -1 if v < 0 else (0 if p == 1 else (1 if p == 2 else -1))
    return small, rowt, xstage, wide_first, persist


def set_wide_variant(v):
    """csrc/gemm_wide_fp4.hip set_wide_variant: g_wide_cfg."""
    return -1 if v < 0 else (5 if v > 5 else v)


def hooks(gemm_small=-1, gemm_wide=-1):
    return Hooks(*set_small_variant(gemm_small), set_wide_variant(gemm_wide))


DEFAULT = hooks()


# ---- one launch ------------------------------------------------------------------------------------------------------------------------------
def valu_covers(B, M, K):
    """dispatch_small: the register budget of the VALU kernel (C = 32-weight chunks per row, nb = x slices per lane)."""
    C, nb = K >> 5, (2 if B <= 2 else (4 if B <= 4 else 8))
    if M * K >= 1 << 32:
        return False
    return C <= 128 or (C <= 256 and nb <= 4) or (C <= 512 and nb <= 2)


def _wide(B, M, K, cus, any_rows, h):
    """gemm_wide_launch: the cell, or None where the call is declined."""
    cfg = h.wide_cfg
    if cfg == 0 or B < 1 or (B <= 16 and not any_rows) or B > 64 or K % 64 != 0 or M < 1:
        return None
    if B * K * 2 >= 1 << 32:
        return None
    if cfg < 0:
        if B <= 16:
            cfg = 3 if M >= 48 * cus else (2 if M >= 20 * cus else 1)
        else:
            cfg = 4 if M >= 96 * cus else (3 if M >= 48 * cus else (2 if M >= 24 * cus else 1))
        if cfg == 1 and B <= 32:
            cfg = 5
    return ("wide", -(-B // 16), cfg)


def _mfma(B, M, K, cus, h):
    """dispatch_mfma."""
    if K % 512:
        return None
    units = K // 512
    rowt = h.rowt if h.rowt > 0 else (2 if (B > 4 and M >= 32 * 256) else 1)
    blocks = -(-M // (16 * rowt))
    persist_auto = (M >= 16384) if B <= 4 else (M > 4096)
    if h.persist != 0 and h.rowt <= 0 and h.xstage != 0 and K == 4096 and (h.persist == 1 or persist_auto):
        return ("persist", 4 if B <= 4 else (8 if B <= 8 else 0))
    xs4 = h.xstage != 0 and B <= 4
    xs8 = h.xstage != 0 and not xs4 and B <= 8 and blocks <= cus
    nbw = 4 if units % 4 == 0 else (2 if units % 2 == 0 else 1)
    xstage = 0
    if nbw >= 4:  # mfma_kernel(): the x images are built for 4 blocks per wave and pass only, the <= 4-row one for one row tile only
        xstage = 4 if (rowt == 1 and xs4) else (8 if xs8 else 0)
    return ("mfma", rowt, nbw, xstage)


def _small(B, M, K, cus, h):
    """gemm_small_entry for 1..16 rows of a 16-bit dtype, blocksize 64 (so K % 64 == 0), aligned operands; None = refused."""
    assert 1 <= B <= 16 and K % BS == 0 and M >= 1
    mfma_ok = K % 512 == 0
    short_few = M <= 2048 and B <= 2 and K <= 4096
    want_mfma = h.small == 1 or (h.small < 0 and not short_few)
    c = None
    if h.wide_first:
        c = _wide(B, M, K, cus, True, h)
    if c is None and mfma_ok and h.small < 0 and not short_few:
        units = K // 512
        if (units & 1) or (units % 4 != 0 and (B >= 5 or M >= 48 * cus)) or (M >= 96 * cus and K >= 8192 and B >= 5) or (
                B >= 13 and K >= 12288 and M <= 16 * cus):
            c = _wide(B, M, K, cus, True, h)
    if c is None and mfma_ok and (want_mfma or B > 8):
        c = _mfma(B, M, K, cus, h)
    if c is None and B <= 8 and K <= 16384 and valu_covers(B, M, K):
        c = ("valu",)
    if c is None and mfma_ok:
        c = _mfma(B, M, K, cus, h)
    if c is None:
        c = _wide(B, M, K, cus, True, h)
    return c


def chunks(B, unit):
    """for_row_chunks (csrc/fp4_call.h): even chunks of at most `unit` rows."""
    n = -(-B // unit)
    per = -(-B // n)
    return [min(per, B - b0) for b0 in range(0, B, per)]


def splitk_bytes(B, M, K, cus):
    """gemm_splitk_workspace_bytes for one launch (blocksize 64, a 16-bit dtype)."""
    if B < 33 or B > 64 or K % 64 != 0 or K < 8192:
        return 0
    if M < 16 or M >= 24 * cus:
        return 0
    if B * K * 2 >= 1 << 32:
        return 0
    return ((K // 64 + 7) // 8) * B * M * 4


def ws_bytes(B, M, K, cus):
    """fp4_hip_gemm_small_ws_bytes: 65..128 rows go through the same workspace as two even chunks."""
    if 64 < B <= 128:
        B = (B + 1) // 2
    return splitk_bytes(B, M, K, cus)


def _splitk(B, M, K, cus):
    slices = (K // 64 + 7) // 8
    tiles, waves = -(-M // 16) * slices, 8 * cus
    return ("splitk", -(-B // 16), max(1, -(-tiles // waves)))


def cells(B, M, K, cus, workspace=False, h=DEFAULT):
    """The launches of one call of 1..128 rows, in order.  `workspace`: fp4_hip_gemm_small_ws with the workspace it asks for."""
    assert 1 <= B <= 128
    if workspace:  # gemm_small_ws_entry
        if B > 64:
            return [c for rows in chunks(B, 64) for c in cells(rows, M, K, cus, True, h)]
        if B >= 33 and splitk_bytes(B, M, K, cus) > 0:
            return [_splitk(B, M, K, cus)]
    if B > 16:  # gemm_small_entry
        c = _wide(B, M, K, cus, False, h) if B <= 64 else None
        if c is not None:
            return [c]
        return [c for rows in chunks(B, 64 if B > 64 else 16) for c in cells(rows, M, K, cus, False, h)]
    return [_small(B, M, K, cus, h)]


def cell(B, M, K, cus, workspace=False, h=DEFAULT):
    """The cell of a call that is one launch."""
    got = cells(B, M, K, cus, workspace, h)
    assert len(got) == 1, (B, M, K, got)
    return got[0]


# ---- forcing a cell from outside ---------------------------------------------------------------------------------------------------------------
def forced(c, B):
    """The fp4_hip_set_variant settings that make a launch of B rows take cell `c` on a shape where the cell is legal
    (legal_cells): {"gemm_small": v, "gemm_wide": v}, a missing key meaning -1.  Split-K cannot be forced: it is taken where the
    caller brings the workspace the library asked for."""
    if c[0] == "valu":
        return {"gemm_small": 0}
    if c[0] == "mfma":  # bit 9 (B fragments straight from global) only where the cell has no x image although the rows would allow one
        return {"gemm_small": 1 | (c[1] << 4) | ((1 << 9) if (c[3] == 0 and B <= 8) else 0)}
    if c[0] == "persist":
        return {"gemm_small": 1 | (2 << 10)}
    if c[0] == "wide":
        return {"gemm_small": 1 << 12, "gemm_wide": c[2]} if B <= 16 else {"gemm_wide": c[2]}
    raise ValueError(c)


def hooks_of(settings):
    return hooks(settings.get("gemm_small", -1), settings.get("gemm_wide", -1))


def legal_cells(B, M, K, cus):
    """Every cell one launch of B <= 64 rows can be forced into on this shape (each kernel family in each row-tile / ring / staging
    form that the shape admits), as the restated dispatcher answers under the forcing settings."""
    out = []

    def add(c):
        got = cell(B, M, K, cus, h=hooks_of(forced(c, B)))
        if got not in out:
            out.append(got)

    if B <= 16:
        if B <= 8 and K <= 16384 and valu_covers(B, M, K):
            add(("valu",))
        if K % 512 == 0:
            for rowt in (1, 2):
                natural = _mfma(B, M, K, cus, hooks(1 | (rowt << 4)))
                add(natural)
                if natural[3] != 0:
                    add(("mfma", rowt, natural[2], 0))
            if K == 4096:
                add(("persist", 4 if B <= 4 else (8 if B <= 8 else 0)))
        for cfg in (5, 2, 3):  # one column tile: 128 rows per workgroup is not built (cfg 4 runs the 64-row kernel)
            add(("wide", 1, cfg))
    else:
        for cfg in (5 if B <= 32 else 1, 2, 3, 4):
            add(("wide", -(-B // 16), cfg))
    return out


# ---- which cells sum alike ---------------------------------------------------------------------------------------------------------------------
def k_partition(c):
    """Which quant blocks of a row one wave sums (in this order, by fmaf into one f32 accumulator per output), and how the waves'
    partial sums meet - read off the kernels.  Two cells with the same answer give the same bits for every output element."""
    if c[0] == "valu":
        return ("valu: the GEMV's register-x geometry, lanes of a row reduced by shuffles",)
    if c[0] == "mfma":  # wave w, pass p: blocks (8 p + w) * nbw + 0 .. nbw - 1; the eight waves' partials added in wave order
        return ("mfma", c[2])
    if c[0] == "persist":  # the same tile arithmetic with nbw = 8 and one pass: wave w owns blocks 8 w .. 8 w + 7
        return ("mfma", 8)
    if c[0] == "wide":
        nt, cfg = c[1], c[2]
        if cfg in (1, 5):  # dispatch_wide_cfg: both numbers name the same kernel
            # <= 2 column tiles: gemm16_wide_auto_kernel, wave w, step t: blocks 2 (8 t + w), 2 (8 t + w) + 1; else gemm16_wide_ring8_kernel,
            # wave w, step s: block 8 s + w
            return ("wide", "WK8 pairs" if nt <= 2 else "WK8")
        return ("wide", "WK4")  # gemm16_wide_ring_kernel<NT, RT = 1 | 2 | 4>: WK = 4 whatever RT, wave slice wk, step s: block 4 s + wk
    if c[0] == "splitk":  # K slices of 8 blocks each, one workgroup per slice, added in slice order by the reducing launch
        return ("splitk",)
    raise ValueError(c)


# Neighbouring cells that cannot differ in any output bit, so that the route test has nothing to tell them apart by (for them only the
# value check applies).  Each names kernels that share ONE K partition and summation order:
EXEMPT = [
    ("mfma rowt", "gemm16_mfma_kernel<NBW, ROWT = 1 | 2>: acc[rt] of a row tile is summed over the same passes and blocks, and s_part "
                  "is reduced in the same wave order, whichever tile of the workgroup the row is in"),
    ("mfma xstage", "gemm16_mfma_kernel<XS = 4 | 8 | 0> (and the persistent kernel's three forms): the B fragment is pair_up8 of the same "
                    "16 bytes of x, read back from the LDS image or straight from global"),
    ("wide ring", "gemm16_wide_ring_kernel<NT, RT = 1 | 2 | 4> (cfg 2 / 3 / 4): WR = 2, WK = 4 in all three; acc[rt][nt] of a tile is its own "
                  "chain over the blocks 4 s + wk, and wide_epilogue adds the four slices in the same order"),
    ("wide cfg 1 = 5", "dispatch_wide_cfg sends cfg 1 and cfg 5 to the same kernel"),
]


def exempt(a, b):
    """The EXEMPT entry that covers the pair of cells, or None."""
    if a[0] == b[0] == "mfma" and a[2] == b[2]:
        return EXEMPT[0] if a[1] != b[1] else EXEMPT[1]
    if a[0] == b[0] == "persist":
        return EXEMPT[1]
    if a[0] == b[0] == "wide" and a[1] == b[1]:
        if a[2] in (2, 3, 4) and b[2] in (2, 3, 4):
            return EXEMPT[2]
        if a[2] in (1, 5) and b[2] in (1, 5):
            return EXEMPT[3]
    return None


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def rows_of(m, cus):
    mult, off = m
    return mult * cus + off


def m_id(m):
    mult, off = m
    if mult == 0:
        return str(off)
    return f"{mult}cus" + (f"{off:+d}" if off else "")


# A threshold of the dispatcher: `rule` as the source spells it, the two neighbouring row counts (below, and on or past it), K and
# the row counts B at which the two sides take different cells.  `probe` is the side on which both cells can be run (the split-K
# path exists below its threshold only).
Threshold = namedtuple("Threshold", "name K lo hi Bs probe")

THRESHOLDS = [
    Threshold("short_few: M <= 2048", 4096, (0, 2048), (0, 2049), (2,), "hi"),
    Threshold("persist_auto: B <= 4, M >= 16384", 4096, (0, 16383), (0, 16384), (4,), "hi"),
    Threshold("persist_auto: B > 4, M > 4096", 4096, (0, 4096), (0, 4097), (5, 16), "hi"),
    Threshold("rowt: B > 4 && M >= 32 * 256", 2048, (0, 8191), (0, 8192), (5, 16), "hi"),
    Threshold("xs8: blocks <= cus", 2048, (16, 0), (16, 1), (8,), "hi"),
    Threshold("pre-emption: units % 4 != 0 && M >= 48 * cus", 1024, (48, -1), (48, 0), (4,), "hi"),
    Threshold("wide, B <= 16: M >= 20 * cus (units = 2)", 1024, (20, -1), (20, 0), (5,), "hi"),
    Threshold("wide, B <= 16: M >= 48 * cus (units = 2)", 1024, (48, -1), (48, 0), (5,), "hi"),
    Threshold("wide, B <= 16: M >= 20 * cus (odd units)", 512, (20, -1), (20, 0), (1, 16), "hi"),
    Threshold("wide, B <= 16: M >= 48 * cus (odd units)", 512, (48, -1), (48, 0), (1, 16), "hi"),
    Threshold("pre-emption: M >= 96 * cus && K >= 8192 && B >= 5", 8192, (96, -1), (96, 0), (5,), "hi"),
    Threshold("pre-emption: B >= 13 && K >= 12288 && M <= 16 * cus", 12288, (16, 0), (16, 1), (13,), "hi"),
    Threshold("wide, B > 16: M >= 24 * cus (K = 576)", 576, (24, -1), (24, 0), (17, 32, 33, 64), "hi"),
    Threshold("wide, B > 16: M >= 48 * cus (K = 576)", 576, (48, -1), (48, 0), (17, 32, 33, 64), "hi"),
    Threshold("wide, B > 16: M >= 96 * cus (K = 576)", 576, (96, -1), (96, 0), (17, 32, 33, 64), "hi"),
    Threshold("wide, B > 16: M >= 24 * cus (K = 4096)", 4096, (24, -1), (24, 0), (17, 32, 33, 64), "hi"),
    Threshold("wide, B > 16: M >= 48 * cus (K = 4096)", 4096, (48, -1), (48, 0), (17, 32, 33, 64), "hi"),
    Threshold("wide, B > 16: M >= 96 * cus (K = 4096)", 4096, (96, -1), (96, 0), (17, 32, 33, 64), "hi"),
    Threshold("split-K: M < 24 * cus", 8192, (24, -1), (24, 0), (33, 64), "lo"),
]
WS_THRESHOLD = THRESHOLDS[-1]  # the one whose calls bring a workspace

# (M, K) -> extra row counts beside the thresholds' own: the controls that stay in one cell across a threshold (B = 3 at short_few,
# B = 4 at rowt and at 96 * cus, B = 12 at the 13-row rule, B = 5 at 48 * cus with units = 2), the 100-row call, the split-K shape with
# four tiles per wave and the decode workload's own shapes
EXTRA = [
    ((0, 2048), 4096, (3,)), ((0, 2049), 4096, (3,)),
    ((0, 8191), 2048, (4,)), ((0, 8192), 2048, (4,)),
    ((48, 0), 1024, (5,)), ((48, -1), 1024, (5,)),
    ((20, -1), 1024, (4,)), ((20, 0), 1024, (4,)),
    ((96, -1), 8192, (4,)), ((96, 0), 8192, (4,)),
    ((16, 0), 12288, (12,)), ((16, 1), 12288, (12,)),
    ((48, 0), 4096, (100,)),
    ((0, 4096), 14336, (64,)),
    ((0, 14336), 4096, (2, 8, 16, 32, 64)), ((0, 28672), 4096, (2, 8, 16, 32, 64)),
]
# calls that bring a workspace: both sides of 24 * cus; tpw = ceil(tiles / (8 * cus)) = 1 (8 * cus rows of K = 8192: exactly one tile per
# wave), 2 (one row more), 3 (24 * cus - 1) and 4 (4096 x 14336)
WS_SHAPES = [((24, -1), 8192, (33, 64)), ((24, 0), 8192, (33, 64)), ((8, 0), 8192, (33, 64)), ((8, 1), 8192, (33, 64)),
             ((0, 4096), 14336, (33, 64))]
EPILOGUE_SHAPES = [((0, 28672), 4096)]  # also run with the gate|up epilogue and a residual


Shape = namedtuple("Shape", "m K Bs ws_Bs epilogues")


def SHAPES():
    """One entry per weight shape, in a fixed order: (m, K, row counts of the plain calls, row counts of the workspace calls,
    whether the epilogues run)."""
    table = {}
    for t in THRESHOLDS:
        for m in (t.lo, t.hi):
            e = table.setdefault((m, t.K), (set(), set()))
            e[0].update(t.Bs)  # (the workspace calls' row counts are plain calls too: the one-pass kernels at the same shape)
            if t is WS_THRESHOLD:
                e[1].update(t.Bs)
    for m, K, Bs in EXTRA:
        table.setdefault((m, K), (set(), set()))[0].update(Bs)
    for m, K, Bs in WS_SHAPES:
        e = table.setdefault((m, K), (set(), set()))
        e[0].update(Bs)
        e[1].update(Bs)
    return [Shape(m, K, tuple(sorted(b)), tuple(sorted(w)), (m, K) in EPILOGUE_SHAPES) for (m, K), (b, w) in table.items()]


def shape_id(s):
    return f"{m_id(s.m)}x{s.K}"


def CASES(cus):
    """(B, M, K, workspace) of every call the GPU file makes with the default dispatch."""
    out = []
    for s in SHAPES():
        M = rows_of(s.m, cus)
        out += [(B, M, s.K, False) for B in s.Bs] + [(B, M, s.K, True) for B in s.ws_Bs]
    return out


def reach_key(c):
    """The cell as the reach test counts it.  Split-K's tiles per wave is a launch argument, not a template: 1, 2 and 3 are the states
    of its weight ring (at most 3 slots, 2 loads ahead), from 4 on the loop is in its steady state."""
    return ("splitk", c[1], min(c[2], 4)) if c[0] == "splitk" else c


def all_cells():
    """Every cell the default dispatch can return (tests/test_fp4_batch_dispatch_host.py enumerates the restatement over a grid of
    shapes and finds exactly these).  Not among them, because no heuristic picks them: one block per wave and pass on the 16-row
    matrix-core kernel (odd K / 512 goes to the one-pass kernels), two blocks with two row tiles (two blocks stay below 5 rows)."""
    out = {("valu",)}
    out |= {("mfma", 1, 4, 4), ("mfma", 1, 4, 8), ("mfma", 1, 4, 0), ("mfma", 2, 4, 8), ("mfma", 2, 4, 0), ("mfma", 1, 2, 0)}
    out |= {("persist", x) for x in (4, 8, 0)}
    out |= {("wide", 1, cfg) for cfg in (5, 2, 3)} | {("wide", 2, cfg) for cfg in (5, 2, 3, 4)}
    out |= {("wide", nt, cfg) for nt in (3, 4) for cfg in (1, 2, 3, 4)}
    out |= {("splitk", nt, tpw) for nt in (3, 4) for tpw in (1, 2, 3, 4)}
    return out
