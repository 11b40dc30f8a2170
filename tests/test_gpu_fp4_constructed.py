"""The FP4 GEMV / small-batch / wide / split-K kernels on CONSTRUCTED inputs, through the C ABI (tests/fp4_constructed.py).

1. Placement: one-hot activations over a weight whose nibble is a known function of (row, k), so that every output is ONE product
   code[nibble(r, k)] * absmax[r][k // 64] * x and a wrong byte, nibble, row, block or activation index shows as a wrong factor,
   not as noise under a sum over K terms.  Every kernel variant the library builds, every dtype.
2. Scales and special values: powers of two over 30 binades in one row, zero scales, one infinite scale, a NaN / Inf activation
   row in a batch (a bad block or row spoils only its own outputs), activations beyond fp16's range of products, fp16 subnormals.
3. Guard regions around every output (and the split-K workspace), operands at shifted addresses, repeats, residual aliasing out,
   and refused calls that must leave the output untouched.

The bar is the project's own (gpu_util.assert_within_bar): |y - y*| <= 1.01 ulp_T(y*)/2 + 1e-5 sum_k |x_k w_rk| against a float64
reference.  Each test prints its worst |err| / tol ("fp4-constructed | ..." lines; profiles/fp4_constructed_inputs.txt keeps them)."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import fp4_constructed as C
import hipabi
from gpu_util import NPDT, assert_within_bar, dev, to_dev, torch_values
from oracle import fp4_oracle as o
from test_gpu_gemv import WS_SHAPE

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT16 = [BF16, F16]
DTYPES = DT16 + [F32]
NONE, GATED = hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS
BS = 64
M_PLACE = 257  # one full byte cycle plus a ragged row

LDS = lambda r, w, u: r | (w << 8) | (u << 16)  # noqa: E731  (the codes of tests/test_gpu_gemv.py)
REGX = lambda it, bands=0: (1 << 24) | (bands << 8) | it  # noqa: E731


@contextlib.contextmanager
def forced(**variants):
    """fp4_hip_set_variant for the duration of a block; None = leave the heuristic alone."""
    live = {k: v for k, v in variants.items() if v is not None}
    try:
        for kernel, v in live.items():
            hipabi.set_variant(kernel, v)
        yield
    finally:
        for kernel in live:
            hipabi.set_variant(kernel, -1)


def report(section, family, dtype, y, exact, scale, out_dtype=None):
    """Prints the worst |err| / tol of a result and holds it to the bar."""
    out_dtype = out_dtype or dtype
    got = y.double().cpu().numpy().reshape(exact.shape)
    tol = C.bar(exact, scale, NPDT[out_dtype])
    ratio = float((np.abs(got - exact) / tol).max())
    print(f"fp4-constructed | {section} | {family} | {NPDT[dtype]} | worst err/tol {ratio:.3f}")
    assert_within_bar(y.reshape(exact.shape), exact, scale, out_dtype)
    return got


def sentinel_filled(shape, dtype):
    n = int(np.prod(shape))
    return C.guarded(n, dtype, 0, dev())[0].view(*shape)


def pad16(n):
    return (n + 15) // 16 * 16 + 16


@functools.lru_cache(maxsize=4)
def placement_weight(M, K, bs=BS):
    return to_dev(C.byte_cycle_weight(M, K)), to_dev(C.placement_scales(M, K, bs))


# ======================================================================================================================================
# 1. placement
# ======================================================================================================================================
def gemv_one_hot(family, M, K, dtype, variant=None, bs=BS, partial=False, x_offset=0):
    """One launch per one-hot position; the outputs are stacked in one sentinel-filled buffer (rows padded, so a store past a row's
    end lands in a pad that is checked) and copied back once."""
    P, A = placement_weight(M, K, bs)
    pos = np.array(C.one_hot_positions(K), dtype=np.int64)
    val = np.array([C.one_hot_value(0, int(k)) for k in pos])
    n = pos.size
    X = torch.zeros(n, K + 8, dtype=dtype, device=dev())
    X[:, x_offset:x_offset + K] = torch_values(C.one_hot_rows(pos, val, K), dtype)
    out_dtype = F32 if partial else dtype
    OUT = sentinel_filled((n, pad16(M)), out_dtype)
    with forced(gemv=variant):
        for i in range(n):
            if partial:
                hipabi.gemv_partial(X[i, x_offset:x_offset + K], P, A, M, K, bs, out=OUT[i, :M])
            else:
                hipabi.gemv(X[i, x_offset:x_offset + K], P, A, M, K, bs, out=OUT[i, :M])
    exact = C.closed_form(M, K, pos, val, bs)
    got = report("placement", f"{family} M{M} K{K}", dtype, OUT[:, :M], exact, np.abs(exact), out_dtype)
    assert (got[exact == 0] == 0).all()  # a +-0 code gives +-0, whatever the scale
    assert C.untouched(OUT[:, M:].contiguous())


GEMV_PLACEMENT = ([("default", None, M_PLACE, K) for K in (64, 512, 2048, 4096)] +
                  [("lds-1-4-2", LDS(1, 4, 2), M_PLACE, 4096), ("lds-1-8-2", LDS(1, 8, 2), M_PLACE, 4096)] +
                  [(f"regx-{it}", REGX(it), M_PLACE, K) for it in (1, 2, 4) for K in (1024, 2048, 4096)] +
                  [(f"bands-5-{it}", REGX(it, 5), M_PLACE, 5120) for it in (1, 2, 4)] +
                  [(f"bands-6-{it}", REGX(it, 6), M_PLACE, 6144) for it in (1, 2, 4)] +
                  [("bands-7-2", REGX(2, 7), M_PLACE, 7168), ("bands-8-2", REGX(2, 8), M_PLACE, 8192), ("bands-8-4", REGX(4, 8), M_PLACE, 8192)] +
                  [("lds-fallback", None, 9, 32768), ("lds-fallback-forced-regx", REGX(2), 9, 32768)] +
                  # deeper register-x slices (2, 3, 4 x groups per lane: K = 8192 on four bands, 11008, 16384), two slices per lane on
                  # five bands (10240) and on seven (14336; 28672: four) - the x permutation of every slice after the first
                  [("regx-2-deep", REGX(2), 9, K) for K in (8192, 11008, 16384)] +
                  [("bands-5-2-deep", REGX(2, 5), 9, 10240), ("bands-7-4-deep", REGX(4, 7), 9, 14336), ("bands-7-2-deep", REGX(2, 7), 9, 28672)])


def _f32_runs_its_own_kernel(family):
    """With f32 activations a forced code only sets the f32 register-x kernel's row pairs (its low byte): the LDS and band codes would
    re-run kernels that regx-1 / 2 / 4 already name, so f32 is run where the code means something for it."""
    return family in ("default", "regx-1", "regx-2", "regx-4", "lds-fallback", "regx-2-deep")


GEMV_PLACEMENT_CASES = [(f, v, m, k, d) for f, v, m, k in GEMV_PLACEMENT for d in DTYPES if d != F32 or _f32_runs_its_own_kernel(f)]


@pytest.mark.parametrize("family,variant,M,K,dtype", GEMV_PLACEMENT_CASES, ids=[f"{f}-K{k}-{NPDT[d]}" for f, _, _, k, d in GEMV_PLACEMENT_CASES])
def test_placement_gemv_every_variant(family, variant, M, K, dtype):
    """fp4_hip_gemv, every 16-bit geometry forced.  f32 activations take kernels of their own (the f32 register-x kernel with 1 / 2 / 4
    row pairs per group, the f32 LDS kernel above K = 16384 or forced with 0, below)."""
    gemv_one_hot(f"gemv {family}", M, K, dtype, variant)


def test_placement_gemv_f32_lds_kernel():
    for K in (64, 4096):
        gemv_one_hot("gemv f32-lds", M_PLACE, K, F32, 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
def test_placement_gemv_generic_path(dtype):
    """The generic kernel: blocksize 32 at K = 96 does not reach it (K % 32 == 0 and 32 divides 96 is the fast path) but is the
    smallest shape with more than one scale per 64 weights; an x view at a 2-byte (f32: 4-byte) offset does."""
    gemv_one_hot("gemv bs32-K96", M_PLACE, 96, dtype, None, bs=32)
    gemv_one_hot("gemv generic (x off 16-byte alignment)", M_PLACE, 512, dtype, None, x_offset=1)
    gemv_one_hot("gemv generic (x off 16-byte alignment), bs32-K96", M_PLACE, 96, dtype, None, bs=32, x_offset=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("K", [64, 512, 2048, 4096])
def test_placement_gemv_partial(K, dtype):
    """fp4_hip_gemv_partial: the raw f32 accumulator, so tol = 1e-5 |exact| with no half-ulp term."""
    gemv_one_hot("gemv_partial default", M_PLACE, K, dtype, None, partial=True)


def batch_one_hot(family, M, K, B, dtype, call, bs=BS):
    """B one-hot rows per launch over the same positions; then the first launch again with x at a 16-byte offset inside a larger
    buffer, which must give the same bits."""
    pos, val = C.one_hot_batches(K, B)
    x = torch_values(C.one_hot_rows(pos, val, K), dtype)  # [L, B, K]
    L = pos.shape[0]
    OUT = sentinel_filled((L, pad16(B * M)), dtype)
    for l in range(L):
        call(x[l], OUT[l, :B * M].view(B, M))
    exact = C.closed_form(M, K, pos, val, bs)
    y = OUT[:, :B * M].reshape(L, B, M)
    got = report("placement", f"{family} B{B} M{M} K{K}", dtype, y, exact, np.abs(exact))
    assert (got[exact == 0] == 0).all()
    assert C.untouched(OUT[:, B * M:].contiguous())
    big = torch.zeros(B * K + 64, dtype=dtype, device=dev())
    big[8:8 + B * K] = x[0].reshape(-1)
    again = sentinel_filled((B, M), dtype)
    call(big[8:8 + B * K].view(B, K), again)
    assert torch.equal(again, y[0])


def small_call(M, K, bs=BS, **variants):
    P, A = placement_weight(M, K, bs)

    def call(x, out):
        with forced(**variants):
            hipabi.gemm_small(x, P, A, M, K, bs, out=out)
    return call


B_SMALL = [1, 2, 4, 5, 8, 9, 16]
SMALL_PLACEMENT = ([("valu", 0, M_PLACE, K, [b for b in B_SMALL if b <= 8]) for K in (512, 4096)] +
                   [(f"mfma-rt{rt}", 1 | (rt << 4), M_PLACE, K, B_SMALL) for rt in (1, 2) for K in (512, 1024, 2048, 4096)] +
                   [("mfma-persist", 1 | (2 << 10), M, 4096, B_SMALL) for M in (33, M_PLACE)] +
                   [("mfma-direct", 1 | (1 << 9), M_PLACE, K, B_SMALL) for K in (512, 4096)] +
                   [("default-ragged-K", None, M_PLACE, K, B_SMALL) for K in (192, 1472)] +  # up to 8 rows: the VALU kernel; above: one-pass
                   [("one-pass-one-tile", 1 << 12, M_PLACE, K, B_SMALL) for K in (192, 1472)])


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("family,variant,M,K,rows", SMALL_PLACEMENT, ids=[f"{f}-M{m}-K{k}" for f, _, m, k, _ in SMALL_PLACEMENT])
def test_placement_small_batch(family, variant, M, K, rows, dtype):
    """fp4_hip_gemm_small, 1..16 rows: the VALU kernel, the one-shot matrix-core kernel with 1 / 2 row tiles, its persistent form, B
    fragments straight from global (bit 9), and K % 512 != 0 in the default dispatch (one-pass kernels with a ragged last step)."""
    for B in rows:
        batch_one_hot(f"small {family}", M, K, B, dtype, small_call(M, K, gemm_small=variant))


VALU_BLOCKSIZES = [(96, 32), (256, 128), (512, 256), (4096, 4096)]  # (K, blocksize): 3 scales a row .. 1; four chunks a scale .. 128


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: NPDT[d])
def test_placement_small_batch_valu_kernel_at_other_blocksizes(dtype):
    """gemm16_small_kernel (variant 0 forced) takes the blocksize at run time and reads its scale through a buffer descriptor at
    chunk >> (log2(blocksize) - 5); everything above runs it at 64.  The placement scales of neighbouring blocks and of neighbouring rows
    differ by a power of two, so a wrong shift or a wrong descriptor size shows as a wrong power of two (or as the 0 of a load the
    descriptor clamped).  This is the kernel a layer of such a blocksize reaches under small_batch_fused."""
    for K, bs in VALU_BLOCKSIZES:
        for B in (2, 5, 8):
            batch_one_hot(f"small valu bs{bs}", M_PLACE, K, B, dtype, small_call(M_PLACE, K, bs, gemm_small=0), bs)


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("M", [M_PLACE, 17])
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_placement_wide_batch(cfg, M, dtype):
    """17..64 rows on the one-pass kernels, every workgroup shape: K = 192 has fewer steps than the weight ring is deep, 1472 a ragged
    last step.  (cfg 5 names the barrier-free 16-row kernel, which holds up to 32 rows; cfg 1 reaches the same kernel up to 32 rows,
    so cfg 5 is run at 17 rows only and adds the code, not a kernel.)"""
    for K in (192, 1024, 1472, 4096):
        for B in ([17] if cfg == 5 else [17, 33, 49, 64]):
            batch_one_hot(f"wide cfg{cfg}", M, K, B, dtype, small_call(M, K, gemm_wide=cfg))


def ws_bytes(B, M, K, dtype):
    l = hipabi.lib()
    l.fp4_hip_gemm_small_ws_bytes.restype = ctypes.c_int64
    l.fp4_hip_gemm_small_ws_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    return l.fp4_hip_gemm_small_ws_bytes(B, M, K, BS, hipabi.DT[dtype])


def test_ws_shape_is_the_smallest_split_k_shape():
    rows, M, K = WS_SHAPE
    assert ws_bytes(rows, M, K, BF16) == (K // 64 // 8) * rows * M * 4 > 0
    assert ws_bytes(rows - 1, M, K, BF16) == 0 and ws_bytes(rows, M - 1, K, BF16) == 0 and ws_bytes(rows, M, K - 64, BF16) == 0


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("M", [16, 17, 40])
@pytest.mark.parametrize("K", [8192, 8256])
def test_placement_split_k(K, M, dtype):
    """fp4_hip_gemm_small_ws on split-K shapes (partial sums through the workspace, then the reducing launch), the workspace exactly
    as large as fp4_hip_gemm_small_ws_bytes asks; 8256 leaves a ragged last K slice."""
    P, A = placement_weight(M, K)
    for B in (33, 64):
        asked = ws_bytes(B, M, K, dtype)
        assert asked == -(-(K // 64) // 8) * B * M * 4 > 0
        wsbuf, ws = C.guarded(asked, torch.uint8, 4096, dev())

        def call(x, out):
            C.refill(wsbuf)
            assert hipabi.gemm_small_ws(x, P, A, M, K, BS, workspace=ws, out=out)[1] == asked
            # the partial sums went through the workspace (a workspace the library turns down would quietly give the one-pass kernels)
            assert not C.untouched(wsbuf, 4096, 4096 + asked) and C.guards_intact(wsbuf, asked, 4096)
        batch_one_hot("split-k", M, K, B, dtype, call)


# ======================================================================================================================================
# families for sections 2 and 3: (entry point, forced variants, rows) at one shape
# ======================================================================================================================================
class Family:
    def __init__(self, name, entry, B=1, M=20, K=2048, gated=True, dtypes=DT16, misaligned=False, bs=BS, **variants):
        self.name, self.entry, self.B, self.M, self.K, self.gated, self.dtypes = name, entry, B, M, K, gated, dtypes
        self.misaligned, self.bs, self.variants = misaligned, bs, variants

    def __repr__(self):
        return self.name

    def call(self, x, P, A, M=None, K=None, bias=None, residual=None, epilogue=NONE, out=None, workspace=None):
        M, K = M or self.M, K or self.K
        with forced(**self.variants):
            if self.entry == "gemv":
                if residual is None and epilogue == NONE:
                    return hipabi.gemv(x.reshape(-1), P, A, M, K, self.bs, bias, out=None if out is None else out.reshape(-1))
                return hipabi.gemv_fused(x.reshape(-1), P, A, M, K, self.bs, bias, None if residual is None else residual.reshape(-1),
                                         epilogue, out=None if out is None else out.reshape(-1))
            if self.entry == "partial":
                assert bias is None and residual is None and epilogue == NONE
                return hipabi.gemv_partial(x.reshape(-1), P, A, M, K, self.bs, out=None if out is None else out.reshape(-1))
            if self.entry == "small":
                if residual is None and epilogue == NONE:
                    return hipabi.gemm_small(x, P, A, M, K, self.bs, bias, out=out)
                return hipabi.gemm_small_fused(x, P, A, M, K, self.bs, bias, residual, epilogue, out=out)
            assert self.entry == "ws"
            return hipabi.gemm_small_ws(x, P, A, M, K, self.bs, bias, residual, epilogue, workspace=workspace, out=out)[0]

    @property
    def out_dtype(self):
        return F32 if self.entry == "partial" else None


SCALE_FAMILIES = (
    [Family("gemv default", "gemv", dtypes=DTYPES), Family("gemv f32-lds", "gemv", dtypes=[F32], gemv=0),
     Family("gemv generic", "gemv", dtypes=DTYPES, misaligned=True),
     Family("gemv lds-1-4-2", "gemv", gated=False, gemv=LDS(1, 4, 2)), Family("gemv lds-1-8-2", "gemv", gated=False, gemv=LDS(1, 8, 2))] +
    [Family(f"gemv regx-{it}", "gemv", dtypes=DTYPES, gemv=REGX(it)) for it in (1, 2, 4)] +
    [Family("gemv_partial default", "partial", dtypes=DTYPES),
     Family("small valu", "small", B=5, gemm_small=0), Family("small mfma-rt1", "small", B=5, gemm_small=1 | (1 << 4)),
     Family("small mfma-rt2", "small", B=5, gemm_small=1 | (2 << 4)), Family("small mfma-direct", "small", B=5, gemm_small=1 | (1 << 9)),
     Family("small mfma-persist x-image", "small", B=5, K=4096, gemm_small=1 | (2 << 10)),
     Family("small mfma-persist register-x", "small", B=9, K=4096, gemm_small=1 | (2 << 10)),
     Family("small one-pass one-tile", "small", B=5, gemm_small=1 << 12)] +
    [Family(f"wide cfg{cfg}", "small", B=33, gemm_wide=cfg) for cfg in (1, 2, 3, 4)] +
    [Family("wide cfg1 two tiles", "small", B=17, gemm_wide=1),  # up to 32 rows: the barrier-free 16-row kernel (what cfg 5 names)
     Family("chunked 16-row launches", "small", B=33, gemm_wide=0), Family("split-k", "ws", B=33, M=16, K=8192)])
SCALE_CASES = [(f, d) for f in SCALE_FAMILIES for d in f.dtypes]
scale_cases = pytest.mark.parametrize("fam,dtype", SCALE_CASES, ids=[f"{f.name}-{NPDT[d]}".replace(" ", "_") for f, d in SCALE_CASES])


@functools.lru_cache(maxsize=8)
def random_bytes(M, K):
    return np.random.default_rng(M * 7919 + K).integers(0, 256, M * K // 2, dtype=np.uint8)


def scale_inputs(fam, dtype, absmax, x=None, seed=0):
    """Device operands of a family's shape with random packed bytes and the given scales; x defaults to N(0, 1) rows.  Returns
    (x_t as the kernel sees it, P, A, float64 product, sum |x w|)."""
    M, K, B = fam.M, fam.K, fam.B
    packed = random_bytes(M, K)
    if x is None:
        x = np.random.default_rng(seed + B).standard_normal((B, K)).astype(np.float32)
    x_t = torch_values(x, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        w = o.dequantize_f32(packed, absmax, BS, M * K).astype(np.float64).reshape(M, K)
        x64 = x_t.double().cpu().numpy()
        exact, scale = x64 @ w.T, np.abs(x64) @ np.abs(w).T
    if fam.misaligned:  # an element offset takes x off 16-byte alignment: the generic kernel
        holder = torch.zeros(B * K + 8, dtype=dtype, device=dev())
        holder[1:1 + B * K] = x_t.reshape(-1)
        x_t = holder[1:1 + B * K].view(B, K)
    return x_t, to_dev(packed), to_dev(absmax), exact, scale


def uniform_scales(M, K, seed=1):
    return np.random.default_rng(seed).uniform(0.005, 0.055, M * K // BS).astype(np.float32)


@scale_cases
def test_scales_powers_of_two_over_thirty_binades(fam, dtype):
    nb = fam.M * fam.K // BS
    absmax = np.ldexp(np.float32(1.0), ((7 * np.arange(nb)) % 31 - 20).astype(np.int32)).astype(np.float32)
    per_row = absmax.reshape(fam.M, -1)
    assert (per_row.min(axis=1) == 2.0**-20).all() and (per_row.max(axis=1) == 2.0**10).all()
    x_t, P, A, exact, scale = scale_inputs(fam, dtype, absmax)
    report("powers of two", fam.name, dtype, fam.call(x_t, P, A), exact, scale, fam.out_dtype)


@scale_cases
def test_scales_zero_blocks_and_a_zero_row(fam, dtype):
    absmax = uniform_scales(fam.M, fam.K)
    absmax[0::3] = 0.0
    absmax.reshape(fam.M, -1)[4] = 0.0
    x_t, P, A, exact, scale = scale_inputs(fam, dtype, absmax)
    got = report("zero scales", fam.name, dtype, fam.call(x_t, P, A), exact, scale, fam.out_dtype)
    assert (got.reshape(fam.B, fam.M)[:, 4] == 0).all()


@scale_cases
def test_scales_one_infinite_block_spoils_its_row_only(fam, dtype):
    absmax = uniform_scales(fam.M, fam.K)
    x_t, P, A, exact, scale = scale_inputs(fam, dtype, absmax)
    bad = absmax.copy()
    bad.reshape(fam.M, -1)[5, 3] = np.inf
    y = fam.call(x_t, P, to_dev(bad))
    got = y.double().cpu().numpy().reshape(fam.B, fam.M)
    assert not np.isfinite(got[:, 5]).any()
    keep = [r for r in range(fam.M) if r != 5]
    assert np.isfinite(got[:, keep]).all()
    report("one infinite scale", fam.name, dtype, y.reshape(fam.B, fam.M)[:, keep], exact[:, keep], scale[:, keep], fam.out_dtype)


BATCH_CASES = [(f, d) for f, d in SCALE_CASES if f.B > 1]


@pytest.mark.parametrize("fam,dtype", BATCH_CASES, ids=[f"{f.name}-{NPDT[d]}".replace(" ", "_") for f, d in BATCH_CASES])
def test_a_nan_or_inf_activation_row_spoils_its_own_outputs_only(fam, dtype):
    """NaN at one k of activation row 1, +Inf at one k of the last row - the row the kernels' column clamp duplicates into the unused
    columns of a 16-wide tile."""
    B, M, K = fam.B, fam.M, fam.K
    absmax = uniform_scales(M, K)
    x = np.random.default_rng(B).standard_normal((B, K)).astype(np.float32)
    _, P, A, exact, scale = scale_inputs(fam, dtype, absmax, x)
    x[1, 70], x[B - 1, K - 3] = np.nan, np.inf
    y = fam.call(torch_values(x, dtype), P, A)
    got = y.double().cpu().numpy().reshape(B, M)
    assert not np.isfinite(got[[1, B - 1]]).any()
    keep = [b for b in range(B) if b not in (1, B - 1)]
    assert np.isfinite(got[keep]).all()
    report("activation isolation", fam.name, dtype, y.reshape(B, M)[keep], exact[keep], scale[keep], fam.out_dtype)


@pytest.mark.parametrize("fam,dtype", [(f, d) for f, d in SCALE_CASES if d != F32],
                         ids=[f"{f.name}-{NPDT[d]}".replace(" ", "_") for f, d in SCALE_CASES if d != F32])
def test_large_activations(fam, dtype):
    """bf16 activations of 3e5 / 1e5 (beyond fp16's range) and fp16 ones of 6e4 (12 |code| x passes 65504), alternating in sign,
    under scales of 2^-12: every product the kernels form on the way must be an f32 one."""
    B, M, K = fam.B, fam.M, fam.K
    k, b = np.arange(K)[None, :], np.arange(B)[:, None]
    sign = np.where((k // 2 + k + b) % 2 == 0, 1.0, -1.0)
    mag = np.where(k % 2 == 0, 3.0e5, 1.0e5) if dtype == BF16 else np.full((1, K), 6.0e4)
    absmax = np.full(M * K // BS, 2.0**-12, np.float32)
    x_t, P, A, exact, scale = scale_inputs(fam, dtype, absmax, (sign * mag).astype(np.float32))
    assert np.abs(exact).max() < 3.0e4  # well inside fp16
    report("large activations", fam.name, dtype, fam.call(x_t, P, A), exact, scale, fam.out_dtype)


# fp16 subnormal activations.  The contract is sum_k x[k] code absmax with f32 arithmetic, which does not flush, so the expectation is
# the float64 product at the usual bar; a family whose instruction flushes subnormal fp16 inputs would be listed here, with the
# flushed row's expectation pinned to what the header then documents.  None does: v_dot2_f32_f16 (GEMV, VALU small batch), the fp16
# v_mfma_f32_16x16x32 (matrix-core, one-pass and split-K kernels) and the generic kernel's f32 FMAs all keep subnormal fp16 inputs on
# gfx950 under the library's build flags (measured: profiles/fp4_constructed_inputs.txt, every family at 0.47-0.70 of the bar; a flushed row would be 0 against |exact| of 1..70).
FLUSHES_F16_SUBNORMAL_X = frozenset()


@pytest.mark.parametrize("fam", [f for f in SCALE_FAMILIES if F16 in f.dtypes], ids=lambda f: f.name.replace(" ", "_"))
def test_fp16_subnormal_activations(fam):
    B, M, K = fam.B, fam.M, fam.K
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((B, K)) * 2.0**-12).astype(np.float32)  # mostly normal fp16 values
    sub = B // 2
    x[sub] = (rng.integers(16, 513, K) * rng.choice([-1.0, 1.0], K) * 2.0**-24).astype(np.float32)
    absmax = np.full(M * K // BS, 2.0**16, np.float32)
    x_t, P, A, exact, scale = scale_inputs(fam, F16, absmax, x)
    xs = x_t.reshape(B, K)[sub].float().abs()
    assert float(xs.max()) < 2.0**-14 and float(xs.min()) >= 2.0**-20  # every element of the row IS a subnormal, none was rounded away
    assert np.abs(exact[sub]).min() > 2.0**-14 and np.abs(exact).max() < 6.0e4  # normal outputs
    if fam.name in FLUSHES_F16_SUBNORMAL_X:
        exact[sub], scale[sub] = 0.0, 0.0
    report("fp16 subnormal activations", fam.name, F16, fam.call(x_t, P, A), exact, scale, fam.out_dtype)


# ======================================================================================================================================
# 3. guards, shifted operands, repeats, aliasing, refusals
# ======================================================================================================================================
M_GUARD = (1, 5, 33, 66, 257)
GUARD_FAMILIES = (
    [Family("gemv default", "gemv", K=64, dtypes=DTYPES), Family("gemv f32-lds", "gemv", K=64, dtypes=[F32], gated=False, gemv=0),
     # the generic kernel (x off 16-byte alignment: four rows per 256-thread block, an M tail in the last block), also at blocksize 32
     Family("gemv generic", "gemv", K=64, gated=False, dtypes=DTYPES, misaligned=True),
     Family("gemv generic bs32", "gemv", K=96, bs=32, gated=False, dtypes=DTYPES, misaligned=True),
     Family("gemv_partial generic", "partial", K=64, gated=False, dtypes=DTYPES, misaligned=True),
     Family("gemv lds-1-4-2", "gemv", K=4096, gated=False, gemv=LDS(1, 4, 2)), Family("gemv lds-1-8-2", "gemv", K=4096, gated=False, gemv=LDS(1, 8, 2))] +
    [Family(f"gemv regx-{it}", "gemv", K=1024, dtypes=DTYPES, gemv=REGX(it)) for it in (1, 2, 4)] +
    [Family(f"gemv bands-5-{it}", "gemv", K=5120, gemv=REGX(it, 5)) for it in (1, 2, 4)] +
    [Family(f"gemv bands-6-{it}", "gemv", K=6144, gemv=REGX(it, 6)) for it in (1, 2, 4)] +
    [Family("gemv bands-7-2", "gemv", K=7168, gemv=REGX(2, 7)), Family("gemv bands-8-2", "gemv", K=8192, gemv=REGX(2, 8)),
     Family("gemv bands-8-4", "gemv", K=8192, gemv=REGX(4, 8)), Family("gemv lds-fallback", "gemv", K=32768, gated=False),
     Family("gemv_partial default", "partial", K=64, gated=False, dtypes=DTYPES),
     Family("small valu", "small", B=(1, 3, 7), K=512, gemm_small=0),
     Family("small mfma-rt1", "small", B=(1, 3, 7, 16), K=512, gemm_small=1 | (1 << 4)),
     Family("small mfma-rt2", "small", B=(1, 3, 7, 16), K=512, gemm_small=1 | (2 << 4)),
     Family("small mfma-direct", "small", B=(1, 3, 7, 16), K=512, gemm_small=1 | (1 << 9)),
     Family("small mfma-persist", "small", B=(1, 3, 7, 16), K=4096, gemm_small=1 | (2 << 10)),
     Family("small default-ragged-K", "small", B=(1, 3, 7, 16), K=192)] +
    [Family(f"wide cfg{cfg}", "small", B=(17, 33, 49, 64), K=192, gemm_wide=cfg) for cfg in (1, 2, 3, 4)] +
    [Family("chunked 16-row launches", "small", B=(17, 33, 49, 64, 100), K=512, gemm_wide=0),
     Family("two chunks of one-pass launches", "small", B=(100,), K=192),
     Family("split-k", "ws", B=(33, 64, 100), K=8192), Family("ws entry below split-k", "ws", B=(3, 17), K=8192)])
GUARD_CASES = [(f, d) for f in GUARD_FAMILIES for d in f.dtypes]


def ulps16(a, b):
    def line(t):
        v = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(v >= 0x8000, 0x8000 - v, v)
    return (line(a) - line(b)).abs()


def placed(t, offset_elems):
    """A copy of t at an element offset inside a larger (16-byte aligned) buffer."""
    holder = torch.zeros(t.numel() + 2 * offset_elems + 8, dtype=t.dtype, device=t.device)
    assert holder.data_ptr() % 16 == 0
    view = holder[offset_elems:offset_elems + t.numel()]
    view.copy_(t.reshape(-1))
    return view.view(t.shape)


def shifted(t, offset_elems):
    """A copy of t at a non-zero 16-byte-aligned offset inside a larger buffer."""
    view = placed(t, offset_elems)
    assert offset_elems > 0 and view.data_ptr() % 16 == 0
    return view


def guard_case(fam, M, B, dtype):
    K, bs = fam.K, fam.bs
    rng = np.random.default_rng(1000 * M + B)
    packed = random_bytes(M, K)
    absmax = np.random.default_rng(M).uniform(0.005, 0.055, M * K // bs).astype(np.float32)
    x_t = torch_values(rng.standard_normal((B, K)).astype(np.float32), dtype)
    b_t = torch_values(rng.standard_normal(M).astype(np.float32) * 0.1, dtype)
    r_t = torch_values(rng.standard_normal((B, M)).astype(np.float32), dtype)
    P, A = to_dev(packed), to_dev(absmax)
    w = o.dequantize_f32(packed, absmax, bs, M * K).astype(np.float64).reshape(M, K)
    x64 = x_t.double().cpu().numpy()
    exact, scale = x64 @ w.T, np.abs(x64) @ np.abs(w).T
    if fam.misaligned:  # one element off 16-byte alignment (2 bytes; f32: 4), here and in the shifted copy below: the generic kernel
        x_t = placed(x_t, 1)
        assert x_t.data_ptr() % 16 == x_t.element_size()
    out_dtype = fam.out_dtype or dtype
    g = C.guard_elems(M)
    what = (fam.name, M, B, NPDT[dtype])
    kw = {}
    wsbuf = None
    if fam.entry == "ws":  # the workspace: exactly the asked size, between guards of its own
        asked = ws_bytes(B, M, K, dtype)
        chunk = B if B <= 64 else (B + 1) // 2
        assert (asked > 0) == (33 <= chunk <= 64 and M >= 16), what
        wsbuf, ws = C.guarded(asked, torch.uint8, 4096, dev())
        kw = dict(workspace=ws if asked else None)
    split_k = wsbuf is not None and asked > 0

    def run(x, P_, A_, bias, residual, epilogue, n_out, out=None):
        """One call into a guarded out (or the given one); checks the guards; returns (buffer, out view)."""
        buf = None
        if out is None:
            buf, out = C.guarded(n_out, out_dtype, g, dev())
        if split_k:
            C.refill(wsbuf)
        fam.call(x, P_, A_, M, K, bias=bias, residual=residual, epilogue=epilogue, out=out.view(B, -1), **kw)
        if split_k:  # the split-K kernels ran: a workspace the library turns down would quietly give the one-pass kernels
            assert not C.untouched(wsbuf, 4096, 4096 + asked), what + ("workspace unused", epilogue)
        if buf is not None:
            assert C.guards_intact(buf, n_out, g), what + ("out guards", epilogue)
        if wsbuf is not None:
            assert C.guards_intact(wsbuf, wsbuf.numel() - 8192, 4096), what + ("workspace guards", epilogue)
        return buf, out.view(B, -1)

    # the bare sum: bar + guards
    buf, plain = run(x_t, P, A, None, None, NONE, B * M)
    assert_within_bar(plain, exact, scale, out_dtype)
    # shifted operands and a repeat into the re-filled buffer: same bits
    xs, Ps, As = (placed(x_t, 9) if fam.misaligned else shifted(x_t, 8)), shifted(P, 16), shifted(A, 4)
    assert not fam.misaligned or xs.data_ptr() % 16 == xs.element_size()
    first = plain.clone()
    C.refill(buf)
    run(xs, Ps, As, None, None, NONE, B * M, out=plain)
    assert torch.equal(plain, first) and C.guards_intact(buf, B * M, g), what + ("shifted / repeated",)
    if fam.entry == "partial":
        return
    # bias + residual (EPILOGUE_NONE): rounded op by rounded op on top of what the entry point gives without the residual
    if fam.entry == "gemv":
        if dtype == F32:
            want = (first.cpu().numpy() + b_t.cpu().numpy()) + r_t.cpu().numpy()
        else:
            want = o.linear_epilogue(first.float().cpu().numpy(), NPDT[dtype], b_t.float().cpu().numpy(), r_t.float().cpu().numpy())
    else:
        _, with_bias = run(x_t, P, A, b_t, None, NONE, B * M)
        bv = b_t.double().cpu().numpy()
        assert_within_bar(with_bias, exact + bv, scale + np.abs(bv), dtype)  # F.linear: bias before the one rounding
        want = o.linear_epilogue(with_bias.float().cpu().numpy(), NPDT[dtype], None, r_t.float().cpu().numpy())
    buf, fused = run(x_t, P, A, b_t, r_t, NONE, B * M)
    assert np.array_equal(fused.float().cpu().numpy().view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), what + ("bias + residual",)
    bs_, rs = shifted(b_t, 8), shifted(r_t, 8)
    first = fused.clone()
    C.refill(buf)
    run(xs, Ps, As, bs_, rs, NONE, B * M, out=fused)
    assert torch.equal(fused, first) and C.guards_intact(buf, B * M, g), what + ("fused, shifted / repeated",)
    # residual aliasing out: h = h + Linear(a) in place, inside a guarded buffer
    hbuf, h = C.guarded(B * M, dtype, g, dev())
    h.copy_(r_t.reshape(-1))
    run(x_t, P, A, b_t, h.view(B, M), NONE, B * M, out=h)
    assert torch.equal(h.view(B, M), first) and C.guards_intact(hbuf, B * M, g), what + ("residual aliases out",)
    # gate | up: B * M / 2 outputs and nothing more
    if fam.gated and M % 2 == 0 and dtype != F32:
        gu_in = fam.call(x_t, P, A, M, K, bias=b_t, **kw).view(B, M)  # rows 2i / 2i+1 = gate_i / up_i, each already T(+ bias)
        ref = torch.nn.functional.silu(gu_in[:, 0::2]) * gu_in[:, 1::2]
        rh = r_t[:, :M // 2].contiguous()
        buf, gu = run(x_t, P, A, b_t, None, GATED, B * M // 2)
        d = ulps16(gu, ref)
        assert int(d.max()) <= 1, what + ("gated vs torch", int(d.max()))
        buf, gur = run(x_t, P, A, b_t, rh, GATED, B * M // 2)
        assert torch.equal(gur, gu + rh), what + ("gated + residual: one more rounded add",)
        first = gur.clone()
        C.refill(buf)
        run(xs, Ps, As, bs_, shifted(rh, 8), GATED, B * M // 2, out=gur)
        assert torch.equal(gur, first) and C.guards_intact(buf, B * M // 2, g), what + ("gated, shifted / repeated",)
        hbuf, h = C.guarded(B * M // 2, dtype, g, dev())
        h.copy_(rh.reshape(-1))
        run(x_t, P, A, b_t, h.view(B, M // 2), GATED, B * M // 2, out=h)
        assert torch.equal(h.view(B, M // 2), first) and C.guards_intact(hbuf, B * M // 2, g), what + ("gated, residual aliases out",)


@pytest.mark.parametrize("fam,dtype", GUARD_CASES, ids=[f"{f.name}-{NPDT[d]}".replace(" ", "_") for f, d in GUARD_CASES])
def test_guards_shifted_operands_repeats_and_aliasing(fam, dtype):
    """Every variant and entry point at its smallest K, M in {1, 5, 33, 66, 257}: the output sits between sentinel guards of at least
    max(4096, 2 M) elements (the gated epilogue writes B M / 2 elements and nothing more; the split-K workspace has guards too),
    shifted operands and a repeat give the same bits, and `residual` may alias `out`."""
    for M in M_GUARD:
        for B in (fam.B if isinstance(fam.B, tuple) else (fam.B,)):
            guard_case(fam, M, B, dtype)


# ---- refused and empty calls ---------------------------------------------------------------------------------------------------------
def raw_batch(entry, x, P, A, bias, residual, out, B, M, K, bs, dtype, epilogue=NONE, ws=None):
    """fp4_hip_gemm_small / _fused / _ws with every argument explicit (null pointers, row counts the operands do not have)."""
    l, p = hipabi.lib(), hipabi._ptr
    dt = hipabi.DT[dtype]
    if entry == "small":
        assert epilogue == NONE and residual is None
        return l.fp4_hip_gemm_small(p(x), p(P), p(A), p(bias), p(out), B, M, K, bs, dt, hipabi._stream())
    if entry == "fused":
        return l.fp4_hip_gemm_small_fused(p(x), p(P), p(A), p(bias), p(residual), p(out), B, M, K, bs, dt, epilogue, hipabi._stream())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    l.fp4_hip_gemm_small_ws.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp, i64, vp]
    return l.fp4_hip_gemm_small_ws(p(x), p(P), p(A), p(bias), p(residual), p(out), B, M, K, bs, dt, epilogue, p(ws),
                                   0 if ws is None else ws.numel(), hipabi._stream())


@pytest.mark.parametrize("entry", ["small", "fused", "ws"])
def test_refused_and_empty_batch_calls_leave_out_untouched(entry):
    M, K = 66, 512
    P = to_dev(random_bytes(M, 576))  # enough bytes for either K
    A, A128 = to_dev(uniform_scales(M, 576)), torch.ones(M * K // 128, device=dev())
    x16 = torch.ones(129, 576, dtype=BF16, device=dev())
    x32 = torch.ones(9, K, dtype=F32, device=dev())
    buf, out = C.guarded(129 * M, BF16, C.guard_elems(M), dev())
    wsbuf, ws = C.guarded(1 << 20, torch.uint8, 4096, dev())
    OK, INVALID, UNSUPPORTED = hipabi.OK, hipabi.ERR_INVALID, hipabi.ERR_UNSUPPORTED
    call = lambda x, B, M_=M, K_=K, bs=BS, dtype=BF16, epi=NONE, P_=P, A_=A, out_=out: raw_batch(  # noqa: E731
        entry, x, P_, A_, None, None, out_, B, M_, K_, bs, dtype, epi, ws if entry == "ws" else None)
    assert call(x16, 0) == OK and call(x16, 4, M_=0) == OK and call(x16, 40, M_=0) == OK  # empty: nothing to do
    assert call(x16, 129) == INVALID and "0 <= B <= 128" in hipabi.last_error()
    assert call(x16, -1) == INVALID
    assert call(x32, 9, dtype=F32) == UNSUPPORTED and "dequant + GEMM" in hipabi.last_error()
    assert call(x16, 12, bs=128, A_=A128) == UNSUPPORTED and "dequant + GEMM" in hipabi.last_error()
    for B in (4, 40):  # 40 rows: the null pointer must be caught before the first of the chunked launches as well
        assert call(None, B) == INVALID and "null pointer" in hipabi.last_error()
        assert call(x16, B, P_=None) == INVALID and call(x16, B, A_=None) == INVALID and call(x16, B, out_=None) == INVALID
    with forced(gemm_wide=0):
        # no kernel takes 12 rows at K % 512 != 0 once the one-pass kernels are off; 100 rows are two chunks of 50, each split into
        # 16-row launches of the same refused shape: the refusal comes before any chunk has written
        assert call(x16, 12, K_=576) == UNSUPPORTED and "not covered" in hipabi.last_error()
        assert call(x16, 100, K_=576) == UNSUPPORTED
    if entry != "small":
        assert call(x16, 4, M_=65, epi=GATED) == INVALID and "even row count" in hipabi.last_error()
        assert call(x16, 40, M_=65, epi=GATED) == INVALID
        assert call(x32, 4, dtype=F32, epi=GATED) == UNSUPPORTED
        assert call(x16, 4, epi=7) == INVALID
    torch.cuda.synchronize()
    assert C.untouched(buf) and C.untouched(wsbuf)


def test_refused_and_empty_gemv_calls_leave_out_untouched():
    M, K = 66, 512
    P, A = to_dev(random_bytes(M, K)), to_dev(uniform_scales(M, K))
    x16, x32 = torch.ones(K, dtype=BF16, device=dev()), torch.ones(K, dtype=F32, device=dev())
    buf, out = C.guarded(M, F32, C.guard_elems(M), dev())  # wide enough for every dtype below
    l, p, s = hipabi.lib(), hipabi._ptr, hipabi._stream
    OK, INVALID, UNSUPPORTED = hipabi.OK, hipabi.ERR_INVALID, hipabi.ERR_UNSUPPORTED
    fused = lambda x, M_, dt, epi, P_=P, out_=out: l.fp4_hip_gemv_fused(p(x), p(P_), p(A), None, None, p(out_), M_, K, BS, dt, epi, s())  # noqa: E731
    assert fused(x16, 0, hipabi.BF16, NONE) == OK and fused(x16, 0, hipabi.BF16, GATED) == OK
    assert fused(x16, 65, hipabi.BF16, GATED) == INVALID and "even row count" in hipabi.last_error()
    assert fused(x32, M, hipabi.F32, GATED) == UNSUPPORTED and "not available" in hipabi.last_error()
    assert fused(x16, M, hipabi.BF16, 7) == INVALID
    assert fused(x16, M, 5, NONE) == UNSUPPORTED
    assert fused(None, M, hipabi.BF16, NONE) == INVALID and fused(x16, M, hipabi.BF16, NONE, P_=None) == INVALID
    assert fused(x16, M, hipabi.BF16, NONE, out_=None) == INVALID
    with forced(gemv=LDS(1, 4, 2)):  # a pair's rows sit in different waves of the LDS geometry
        assert fused(x16, M, hipabi.BF16, GATED) == UNSUPPORTED
    assert l.fp4_hip_gemv(p(x16), p(P), p(A), None, p(out), -1, K, BS, hipabi.BF16, s()) == INVALID
    assert l.fp4_hip_gemv(p(x16), p(P), p(A), None, p(out), M, 511, BS, hipabi.BF16, s()) == INVALID
    assert l.fp4_hip_gemv_partial(p(x16), p(P), p(A), p(out), 0, K, BS, hipabi.BF16, s()) == OK
    assert l.fp4_hip_gemv_partial(None, p(P), p(A), p(out), M, K, BS, hipabi.BF16, s()) == INVALID
    assert l.fp4_hip_gemv_partial(p(x16), p(P), p(A), None, M, K, BS, hipabi.BF16, s()) == INVALID
    torch.cuda.synchronize()
    assert C.untouched(buf)
