"""The NF4 kernels on CONSTRUCTED inputs, through the C ABI (tests/nf4_constructed.py; the NF4 side of
tests/test_gpu_fp4_constructed.py, same structure and names).

1. Placement: one-hot activations over the byte-cycle weight under the placement scales, so that every output is ONE product
   CODE[nibble(r, k)] * absmax[r][k // bs] * x and a wrong byte, nibble, row, block or activation index shows as a wrong factor.
   The batch-1 kernel in each of its 12 dispatch cells, both table layouts, three dtypes (f32 also BY VALUE against the kernel's
   f32 restatement), the generic kernel, the fused / LoRA / nested GEMV, the 1..16-row and the 17..128-row matrix-core kernels, the
   batched adapter form and the down projection (one-hot x over a dyadic A: exact in f32).
2. Scales and special values: powers of two over 30 binades in one row, zero scales, one infinite scale, non-finite activations
   (a bad row of a batch spoils its own outputs only; a bad activation at batch 1 makes EVERY output non-finite - dead lanes
   re-read the last chunk of x under a zero scale), activations beyond fp16's range of products, fp16 subnormal activations.
3. Guard regions of guard_elems(M) around every batch-1 output, operands at shifted addresses, repeats.

The bar is the project's own (gpu_util.assert_within_bar): |y - y*| <= 1.01 ulp_T(y*)/2 + 1e-5 sum |x w| against a float64
reference; for the adapter entry points sum |x w| includes sum_j |B_rj| |t_j| (t is given, so the term is one more f32
accumulation of the same kind).  Each test prints its worst |err| / tol ("nf4-constructed | ..." lines;
profiles/nf4_constructed_inputs.txt keeps them).

Families left out of a section, and why:
* the gated epilogue has no f32 (the entry points refuse it), so every gated case is 16-bit;
* fp4_hip_gemm_small_nf4 / _wide_nf4 / _fused_nf4 / _lora_nf4 take no f32, so the batch families are 16-bit;
* fp4_hip_lora_down has no absmax: the scale section does not apply to it (its per-row factor is covered by the placement test);
* large activations: f32 has nothing to overflow on the way, as in the FP4 file."""
import functools

import numpy as np
import pytest
import torch

import hipabi
import nested_ref as N
import nf4_constructed as C
import nf4_ref as R
import test_gpu_nf4_gemv as NG
import test_gpu_nf4_small_batch as SB
import test_gpu_nf4_wide_batch as WB
from gpu_util import NPDT, assert_within_bar, dev, to_dev, torch_values
from oracle import fp4_oracle as o
from test_gpu_fp4_constructed import forced, pad16, placed, sentinel_filled, shifted, ulps16
from test_gpu_nested import gemv_nested
from test_gpu_nf4_fused import bs_of, gemm_fused, gemv_fused
from test_gpu_nf4_lora import down, gemm_lora, gemv_lora

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT16 = [BF16, F16]
DTYPES = DT16 + [F32]
NONE, GATED = hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS
BS = 64
M_PLACE = 257  # one full byte cycle plus a ragged row (and a ragged 16-row tile)
LAYOUTS = [0, 1]  # fp4_hip_set_variant("gemv_nf4", v): the 16-entry f32 table, the 256-entry pair table


@pytest.fixture(autouse=True)
def _heuristics_restored():
    yield
    hipabi.set_variant("gemv_nf4", -1)
    hipabi.set_variant("gemm_wide_nf4", -1)


def report(section, family, dtype, y, exact, scale, out_dtype=None):
    """Prints the worst |err| / tol of a result and holds it to the bar."""
    out_dtype = out_dtype or dtype
    got = y.double().cpu().numpy().reshape(exact.shape)
    tol = C.bar(exact, scale, NPDT[out_dtype])
    ratio = float((np.abs(got - exact) / tol).max())
    print(f"nf4-constructed | {section} | {family} | {NPDT[dtype]} | worst err/tol {ratio:.3f}")
    assert_within_bar(y.reshape(exact.shape), exact, scale, out_dtype)
    return got


@functools.lru_cache(maxsize=4)
def byte_cycle(M, K):
    return to_dev(C.byte_cycle_weight(M, K))


@functools.lru_cache(maxsize=4)
def placement_absmax(M, K, bs):
    return to_dev(C.placement_scales(M, K, bs))


def as_np(t):
    return t.float().cpu().numpy()


# ======================================================================================================================================
# 1. placement
# ======================================================================================================================================
def gemv_one_hot(family, call, M, K, dtype, bs, absmax=None, x_offset=0):
    """One launch per one-hot position; the outputs are stacked in one sentinel-filled buffer (rows padded, so a store past a row's
    end lands in a pad that is checked) and copied back once.  Returns (x rows as the kernel saw them, OUT, pos, val)."""
    pos = np.array(C.one_hot_positions(K), dtype=np.int64)
    val = np.array([C.one_hot_value(0, int(k)) for k in pos])
    n = pos.size
    X = torch.zeros(n, K + 8, dtype=dtype, device=dev())
    X[:, x_offset:x_offset + K] = torch_values(C.one_hot_rows(pos, val, K), dtype)
    xs = [X[i, x_offset:x_offset + K] for i in range(n)]
    OUT = sentinel_filled((n, pad16(M)), dtype)
    for i in range(n):
        call(xs[i], OUT[i, :M])
    exact = C.closed_form_nf4(M, K, pos, val, bs, absmax=absmax)
    got = report("placement", f"{family} M{M} K{K}", dtype, OUT[:, :M], exact, np.abs(exact))
    assert (got[exact == 0] == 0).all()  # code 7 is 0.0: whatever the scale
    assert C.untouched(OUT[:, M:].contiguous())
    return xs, OUT, pos, val


CELL_IDS = [f"{m}x{k}-ks{R.gemv_cell(m, k)[0]}-G{R.gemv_cell(m, k)[1]}-it{R.gemv_cell(m, k)[2]}" for m, k in C.GEMV_PLACEMENT_CASES]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["table16", "pair-table"])
@pytest.mark.parametrize("M,K", C.GEMV_PLACEMENT_CASES, ids=CELL_IDS)
def test_placement_gemv_every_cell(M, K, layout, dtype):
    """fp4_hip_gemv_nf4 in each of the 12 (ks, G, iters) cells, at a shape with a row tail and a partial last pass.  f32: the result
    also EQUALS fl32(fl32(code * x) * absmax) by value - a one-hot row leaves that one rounding (every other term is an exact zero,
    the scale a power of two, and the sums over lanes, passes and K bands add zeros)."""
    bs = bs_of(K)
    P, A = byte_cycle(M, K), placement_absmax(M, K, bs)
    with forced(gemv_nf4=layout):
        _, OUT, pos, val = gemv_one_hot(f"gemv cell {R.gemv_cell(M, K)} layout {layout}", lambda x, out: R.gemv(x, P, A, M, K, bs, out=out), M, K, dtype, bs)
    if dtype == F32:
        assert np.array_equal(OUT[:, :M].cpu().numpy(), C.gemv_f32_restatement(M, K, pos, val, bs))  # zeros compare equal whatever their sign


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
def test_placement_gemv_generic_path(dtype):
    """The generic kernel with the NF4 table: x off 16-byte alignment at blocksize 32, and K % 32 != 0 with a blocksize of 50."""
    for M, K, bs, off in ((37, 96, 32, 1), (33, 250, 50, 0), (33, 250, 50, 1)):
        P, A = byte_cycle(M, K), placement_absmax(M, K, bs)
        gemv_one_hot(f"gemv generic bs{bs} x+{off}", lambda x, out: R.gemv(x, P, A, M, K, bs, out=out), M, K, dtype, bs, x_offset=off)


FUSED_SHAPES = [(66, 1024), (66, 4096)]  # KSPLIT 1 (a pair meets through readlane) and KSPLIT 4 (through s_part)


def exact_rows(M, dtype):
    """bias[r] = (r - 33) / 4 and residual[r] = 16 (r + 1): distinct per row and exact in every T (M <= 257)."""
    r = np.arange(M, dtype=np.float64)
    return torch_values((r - 33) / 4, dtype), torch_values(16 * (r + 1), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("M,K", FUSED_SHAPES, ids=[f"{m}x{k}" for m, k in FUSED_SHAPES])
def test_placement_gemv_fused(M, K, dtype):
    """fp4_hip_gemv_fused_nf4: the bare sum at the bar; with a per-row bias and residual bit for bit the oracle's rounded adds on
    it (a wrong epilogue row would add another row's bias); the gated epilogue within 1 ulp of torch's silu * up of the bare rows."""
    P, A = byte_cycle(M, K), placement_absmax(M, K, BS)
    bias, res = exact_rows(M, dtype)
    assert len(set(as_np(bias).tolist())) == M == len(set(as_np(res).tolist()))
    xs, OUT, pos, _ = gemv_one_hot("gemv_fused", lambda x, out: gemv_fused(x, P, A, M, K, BS, out=out), M, K, dtype, BS)
    n = len(xs)
    FULL = sentinel_filled((n, pad16(M)), dtype)
    for i in range(n):
        gemv_fused(xs[i], P, A, M, K, BS, bias, res, out=FULL[i, :M])
    plain = as_np(OUT[:, :M])
    want = (plain + as_np(bias)) + as_np(res) if dtype == F32 else o.linear_epilogue(plain, NPDT[dtype], as_np(bias), as_np(res))
    assert np.array_equal(as_np(FULL[:, :M]).view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
    assert C.untouched(FULL[:, M:].contiguous())
    if dtype == F32:
        return  # the gated epilogue has no f32
    GU = sentinel_filled((n, pad16(M // 2)), dtype)
    for i in range(n):
        gemv_fused(xs[i], P, A, M, K, BS, None, None, GATED, out=GU[i, :M // 2])
    ref = torch.nn.functional.silu(OUT[:, 0:M:2]) * OUT[:, 1:M:2]
    assert int(ulps16(GU[:, :M // 2], ref).max()) <= 1 and C.untouched(GU[:, M // 2:].contiguous())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("Rr", [8, 24, 256])
@pytest.mark.parametrize("M,K", FUSED_SHAPES, ids=[f"{m}x{k}" for m, k in FUSED_SHAPES])
def test_placement_gemv_lora_one_hot_t(M, K, Rr, dtype):
    """fp4_hip_gemv_lora_nf4 with x = 0 and t one-hot at every j: out[r] = T(lora_B[r][j] * t_j), exact in T, so equality by value.
    KSPLIT 1 adds the delta in the wave; KSPLIT 4 sends it through its own s_part column.  (f32 with a random base sum:
    tests/test_gpu_nf4_lora.py::test_one_hot_adapter_adds_t_in_one_f32_add.)"""
    P, A = byte_cycle(M, K), placement_absmax(M, K, BS)
    b = C.lora_b(M, Rr)
    lB = torch_values(b, dtype)
    x = torch.zeros(K, dtype=dtype, device=dev())
    val = np.array([C.one_hot_value(0, j) for j in range(Rr)])
    T = to_dev(np.diag(val).astype(np.float32))
    exact = b.astype(np.float64).T * val[:, None]  # [j, r]
    for layout in LAYOUTS:
        OUT = sentinel_filled((Rr, pad16(M)), dtype)
        with forced(gemv_nf4=layout):
            for j in range(Rr):
                gemv_lora(x, P, A, M, K, lB, T[j], BS, out=OUT[j, :M])
        got = report("placement", f"gemv_lora M{M} K{K} R{Rr} layout {layout}", dtype, OUT[:, :M], exact, np.abs(exact))
        assert np.array_equal(got, exact) and C.untouched(OUT[:, M:].contiguous())


NESTED_SHAPES = [(200, 96, 32), (40, 1024, 64)]  # three blocks per row: group boundaries fall mid-row; 16 rows per group


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["table16", "pair-table"])
@pytest.mark.parametrize("offset", C.NESTED_OFFSETS)
@pytest.mark.parametrize("M,K,bs", NESTED_SHAPES, ids=[f"{m}x{k}-bs{b}" for m, k, b in NESTED_SHAPES])
def test_placement_gemv_nested(M, K, bs, offset, layout, dtype):
    """fp4_hip_gemv_nested_nf4 on a custom table whose expansion is exact: at the bar against the closed form, and bit-equal to
    fp4_hip_gemv_fused_nf4 on the host-expanded statistics."""
    nb = M * K // bs
    q, nested, code, off = C.nested_statistics(nb, offset)
    expanded = N.unnest(q, nested, code, off, C.NESTED_GROUP)
    P, qd, nd, cd, Ad = byte_cycle(M, K), to_dev(q), to_dev(nested), to_dev(code), to_dev(expanded)
    with forced(gemv_nf4=layout):
        xs, OUT, _, _ = gemv_one_hot(f"gemv_nested bs{bs} offset {offset} layout {layout}",
                                     lambda x, out: gemv_nested(x, P, qd, nd, cd, off, M, K, bs, out=out), M, K, dtype, bs, absmax=expanded)
        FUSED = sentinel_filled(tuple(OUT.shape), dtype)
        for i, x in enumerate(xs):
            gemv_fused(x, P, Ad, M, K, bs, out=FUSED[i, :M])
    assert torch.equal(OUT, FUSED)


def batch_one_hot(family, M, K, B, dtype, call):
    """B one-hot rows per launch over the same positions; then the first launch again with x at a 16-byte offset inside a larger
    buffer, which must give the same bits."""
    pos, val = C.one_hot_batches(K, B)
    x = torch_values(C.one_hot_rows(pos, val, K), dtype)  # [L, B, K]
    L = pos.shape[0]
    OUT = sentinel_filled((L, pad16(B * M)), dtype)
    for l in range(L):
        call(x[l], OUT[l, :B * M].view(B, M))
    exact = C.closed_form_nf4(M, K, pos, val)
    y = OUT[:, :B * M].reshape(L, B, M)
    got = report("placement", f"{family} B{B} M{M} K{K}", dtype, y, exact, np.abs(exact))
    assert (got[exact == 0] == 0).all()
    assert C.untouched(OUT[:, B * M:].contiguous())
    big = torch.zeros(B * K + 64, dtype=dtype, device=dev())
    big[8:8 + B * K] = x[0].reshape(-1)
    again = sentinel_filled((B, M), dtype)
    call(big[8:8 + B * K].view(B, K), again)
    assert torch.equal(again, y[0])


def batch_call(entry, M, K):
    P, A = byte_cycle(M, K), placement_absmax(M, K, BS)

    def call(x, out):
        B = x.numel() // K
        if entry == "fused":
            return gemm_fused(x, P, A, M, K, out=out)
        rc = (SB if entry == "small" else WB).call(x, P, A, out, B, M, K)
        assert rc == hipabi.OK, (rc, hipabi.last_error())
    return call


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("entry", ["small", "fused"])
@pytest.mark.parametrize("K", [512, 1024, 2048])
def test_placement_small_batch(K, entry, dtype):
    """fp4_hip_gemm_small_nf4 / fp4_hip_gemm_fused_nf4 at 1..16 rows: K / 512 = 1, 2, 4 blocks per wave; 16 rows load x directly,
    8 and 4 rows through the x image (at K = 2048)."""
    for B in (1, 4, 8, 16):
        batch_one_hot(f"{entry} 1..16 rows", M_PLACE, K, B, dtype, batch_call(entry, M_PLACE, K))


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("entry", ["wide", "fused"])
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("M", [M_PLACE, 17])
def test_placement_wide_batch(M, variant, entry, dtype):
    """fp4_hip_gemm_wide_nf4 / fp4_hip_gemm_fused_nf4 at 17..128 rows, 16 and 32 weight rows per workgroup: K = 64 and 192 are one
    and three blocks (NBW 1), 256 four (NBW 4), 576 a ragged last pass; 100 rows are two chunks of 50.  3 and 16 rows at K = 192:
    the one-tile form."""
    with forced(gemm_wide_nf4=variant):
        for K in (64, 192, 256, 576):
            for B in (17, 33, 49, 64, 100) + ((3, 16) if K == 192 else ()):
                batch_one_hot(f"{entry} wide v{variant}", M, K, B, dtype, batch_call(entry, M, K))


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("Rr", [8, 24, 256])
@pytest.mark.parametrize("K", [512, 192])
def test_placement_gemm_lora_one_hot_t(K, Rr, dtype):
    """fp4_hip_gemm_lora_nf4 with x = 0 and a one-hot row of t per activation row, at a different j per row: 2 and 16 rows run the
    16-row kernel (K = 512) or the one-tile form (K = 192), 17 and 64 rows the wide kernel."""
    M = 66
    P, A = byte_cycle(M, K), placement_absmax(M, K, BS)
    b = C.lora_b(M, Rr)
    lB = torch_values(b, dtype)
    for B in (2, 16, 17, 64):
        x = torch.zeros(B, K, dtype=dtype, device=dev())
        pos, val = C.deal(range(Rr), B)  # [L, B]: the j of each row
        L = pos.shape[0]
        T = to_dev(C.one_hot_rows(pos, val, Rr))  # f32 [L, B, R]
        OUT = sentinel_filled((L, pad16(B * M)), dtype)
        for l in range(L):
            gemm_lora(x, P, A, M, K, lB, T[l], out=OUT[l, :B * M].view(B, M))
        exact = b.astype(np.float64).T[pos] * val[..., None]  # [L, B, M]
        got = report("placement", f"gemm_lora B{B} K{K} R{Rr}", dtype, OUT[:, :B * M].reshape(L, B, M), exact, np.abs(exact))
        assert np.array_equal(got, exact) and C.untouched(OUT[:, B * M:].contiguous())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("Rr", [8, 256])
@pytest.mark.parametrize("K", [8, 64, 4096, 8192, 8200])
def test_placement_lora_down(K, Rr, dtype):
    """fp4_hip_lora_down on one-hot x: t[b][j] = scale[j] * A[j][k] * x, one exact f32 product, so equality by value.  K = 8 is one
    unit (255 clamped threads), 8192 exactly one pass, 8200 a second pass of one unit; 1, 5, 9 rows leave clamped rows in a group of
    four, 9 and 64 rows more than one workgroup per adapter row."""
    a, s = C.lora_a(Rr, K), C.down_scale(Rr)
    A, scale = torch_values(a, dtype), to_dev(s)
    g = C.guard_elems(Rr)
    for rows in (1, 5, 8, 9, 64):
        pos, val = C.deal(C.down_positions(K), rows)
        L = pos.shape[0]
        x = torch_values(C.one_hot_rows(pos, val, K), dtype)
        buf, t = C.guarded(L * rows * Rr, F32, g, dev())
        t = t.view(L, rows, Rr)
        for l in range(L):
            down(x[l], A, scale, t[l])
        exact = s.astype(np.float64)[None, None, :] * a.astype(np.float64).T[pos] * val[..., None]  # [L, rows, R]
        got = report("placement", f"lora_down R{Rr} K{K} rows{rows}", dtype, t, exact, np.abs(exact), F32)
        assert np.array_equal(got, exact) and C.guards_intact(buf, L * rows * Rr, g)


# ======================================================================================================================================
# families for sections 2 and 3: (entry point, forced variants, rows) at one small shape
# ======================================================================================================================================
class Family:
    """entry: gemv / fused / lora / nested (batch 1), small / wide / gemm_fused / gemm_lora (B rows)."""

    def __init__(self, name, entry, B=1, M=20, K=2048, dtypes=DT16, bs=BS, misaligned=False, Rr=24, **variants):
        self.name, self.entry, self.B, self.M, self.K, self.dtypes, self.bs = name, entry, B, M, K, dtypes, bs
        self.misaligned, self.Rr, self.variants = misaligned, Rr, variants

    def __repr__(self):
        return self.name

    @property
    def lora(self):
        return self.entry in ("lora", "gemm_lora")

    def adapter(self, dtype, t=None):
        """(lora_B T[M, R] with an all-zero row 4, t f32[B, R], float64 delta [B, M], sum_j |B_rj| |t_j| [B, M])."""
        rng = np.random.default_rng(self.Rr + self.B)
        b = (rng.integers(-8, 9, (self.M, self.Rr)) / 16.0).astype(np.float32)
        if self.M > 4:
            b[4] = 0.0
        t = rng.standard_normal((self.B, self.Rr)).astype(np.float32) if t is None else np.asarray(t, np.float32)
        with np.errstate(invalid="ignore"):
            return torch_values(b, dtype), to_dev(t), t.astype(np.float64) @ b.astype(np.float64).T, np.abs(t.astype(np.float64)) @ np.abs(b.astype(np.float64)).T

    def call(self, x, P, absmax, lB=None, t=None, bias=None, residual=None, epilogue=NONE, out=None):
        """absmax: a device tensor, or for the nested entry the (q, nested, code256, offset) device statistics."""
        M, K, B, bs, e = self.M, self.K, self.B, self.bs, self.entry
        with forced(**self.variants):
            if e == "gemv":
                assert residual is None and epilogue == NONE
                return R.gemv(x.reshape(-1), P, absmax, M, K, bs, bias, out=out)
            if e == "fused":
                return gemv_fused(x.reshape(-1), P, absmax, M, K, bs, bias, residual, epilogue, out=out)
            if e == "lora":
                return gemv_lora(x.reshape(-1), P, absmax, M, K, lB, t.reshape(-1), bs, bias, residual, epilogue, out=out)
            if e == "nested":
                q, nested, code, off = absmax
                return gemv_nested(x.reshape(-1), P, q, nested, code, off, M, K, bs, bias, residual, epilogue, out=out)
            if e == "gemm_fused":
                return gemm_fused(x, P, absmax, M, K, bs, bias, residual, epilogue, out=out)
            if e == "gemm_lora":
                return gemm_lora(x, P, absmax, M, K, lB, t, bs, bias, residual, epilogue, out=out)
            assert e in ("small", "wide") and residual is None and epilogue == NONE
            out = torch.empty(B, M, dtype=x.dtype, device=x.device) if out is None else out
            rc = (SB if e == "small" else WB).call(x, P, absmax, out, B, M, K, bias=bias)
            assert rc == hipabi.OK, (rc, hipabi.last_error())
            return out


# K = 2048: ks 2 (pairs of rows meet through s_part); 1024: ks 1; small: 4 blocks per wave, the 8-row x image (B 5) and direct x
# (B 16, K 512); wide: 16 / 32 weight rows per workgroup at three column tiles, the one-tile form at K % 512 != 0
SCALE_FAMILIES = (
    [Family("gemv table16", "gemv", dtypes=DTYPES, gemv_nf4=0), Family("gemv pair-table", "gemv", dtypes=DTYPES, gemv_nf4=1),
     Family("gemv ks1", "gemv", K=1024, dtypes=DTYPES), Family("gemv generic", "gemv", dtypes=DTYPES, misaligned=True),
     Family("gemv_fused", "fused", dtypes=DTYPES), Family("gemv_lora", "lora", dtypes=DTYPES), Family("gemv_lora ks1 R256", "lora", K=1024, Rr=256, dtypes=DTYPES),
     Family("gemv_nested table16", "nested", dtypes=DTYPES, gemv_nf4=0), Family("gemv_nested pair-table", "nested", dtypes=DTYPES, gemv_nf4=1),
     Family("small x-image", "small", B=5), Family("small direct", "small", B=16, K=512),
     Family("wide v1", "wide", B=33, gemm_wide_nf4=1), Family("wide v2", "wide", B=33, gemm_wide_nf4=2),
     Family("wide one-tile", "wide", B=5, K=192), Family("wide two chunks", "wide", B=100, K=192),
     Family("gemm_fused 16-row kernel", "gemm_fused", B=5), Family("gemm_fused wide", "gemm_fused", B=33),
     Family("gemm_lora 16-row kernel", "gemm_lora", B=5), Family("gemm_lora wide", "gemm_lora", B=33), Family("gemm_lora one-tile", "gemm_lora", B=5, K=192)])
SCALE_CASES = [(f, d) for f in SCALE_FAMILIES for d in f.dtypes]
case_ids = lambda cases: [f"{f.name}-{NPDT[d]}".replace(" ", "_") for f, d in cases]  # noqa: E731
scale_cases = pytest.mark.parametrize("fam,dtype", SCALE_CASES, ids=case_ids(SCALE_CASES))


@functools.lru_cache(maxsize=8)
def random_bytes(M, K):
    return np.random.default_rng(M * 7919 + K).integers(0, 256, M * K // 2, dtype=np.uint8)


def dev_absmax(fam, absmax):
    if fam.entry == "nested":
        q, nested, code, off = C.tabled_statistics(absmax)
        return to_dev(q), to_dev(nested), to_dev(code), off
    return to_dev(absmax)


def scale_inputs(fam, dtype, absmax, x=None, t=None, seed=0):
    """Device operands of a family's shape with random packed bytes and the given scales; x defaults to N(0, 1) rows.  Returns
    (x_t as the kernel sees it, keyword operands of fam.call, float64 result, sum |x w| (+ sum |B| |t|))."""
    M, K, B = fam.M, fam.K, fam.B
    packed = random_bytes(M, K)
    if x is None:
        x = np.random.default_rng(seed + B).standard_normal((B, K)).astype(np.float32)
    x_t = torch_values(x, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        w = R.dequantize_f32(packed, absmax, fam.bs, M * K).astype(np.float64).reshape(M, K)
        x64 = x_t.double().cpu().numpy()
        exact, scale = x64 @ w.T, np.abs(x64) @ np.abs(w).T
    kw = dict(P=to_dev(packed), absmax=dev_absmax(fam, absmax))
    if fam.lora:
        kw["lB"], kw["t"], delta, dscale = fam.adapter(dtype, t)
        with np.errstate(invalid="ignore"):
            exact, scale = exact + delta, scale + dscale
    if fam.misaligned:  # an element offset takes x off 16-byte alignment: the generic kernel
        x_t = placed(x_t, 1)
    return x_t, kw, exact, scale


def tabled_uniform_scales(M, K, bs=BS, seed=1):
    """Scales in [0.005, 0.055) drawn from 200 values, so that the nested families can hold them in a 256-entry table."""
    rng = np.random.default_rng(seed)
    return rng.choice(rng.uniform(0.005, 0.055, 200).astype(np.float32), M * K // bs)


@scale_cases
def test_scales_powers_of_two_over_thirty_binades(fam, dtype):
    nb = fam.M * fam.K // fam.bs
    absmax = np.ldexp(np.float32(1.0), ((7 * np.arange(nb)) % 31 - 20).astype(np.int32)).astype(np.float32)
    per_row = absmax.reshape(fam.M, -1)
    if per_row.shape[1] >= 31:
        assert (per_row.min(axis=1) == 2.0**-20).all() and (per_row.max(axis=1) == 2.0**10).all()
    else:  # K = 192 / 512: three / eight blocks per row, 7 binades apart
        assert (per_row.max(axis=1) / per_row.min(axis=1) >= 2.0**14).all()
    x_t, kw, exact, scale = scale_inputs(fam, dtype, absmax)
    report("powers of two", fam.name, dtype, fam.call(x_t, **kw), exact, scale)


@scale_cases
def test_scales_zero_blocks_and_a_zero_row(fam, dtype):
    absmax = tabled_uniform_scales(fam.M, fam.K, fam.bs)
    absmax[0::3] = 0.0
    absmax.reshape(fam.M, -1)[4] = 0.0
    x_t, kw, exact, scale = scale_inputs(fam, dtype, absmax)
    got = report("zero scales", fam.name, dtype, fam.call(x_t, **kw), exact, scale)
    assert (got.reshape(fam.B, fam.M)[:, 4] == 0).all()  # (the adapter families' lora_B has a zero row 4)


@scale_cases
def test_scales_one_infinite_block_spoils_its_row_only(fam, dtype):
    absmax = tabled_uniform_scales(fam.M, fam.K, fam.bs)
    x_t, kw, exact, scale = scale_inputs(fam, dtype, absmax)
    bad = absmax.copy()
    bad.reshape(fam.M, -1)[5, -1 if fam.K == 192 else 3] = np.inf
    kw["absmax"] = dev_absmax(fam, bad)
    y = fam.call(x_t, **kw)
    got = y.double().cpu().numpy().reshape(fam.B, fam.M)
    assert not np.isfinite(got[:, 5]).any()
    keep = [r for r in range(fam.M) if r != 5]
    assert np.isfinite(got[:, keep]).all()
    report("one infinite scale", fam.name, dtype, y.reshape(fam.B, fam.M)[:, keep], exact[:, keep], scale[:, keep])


BATCH_CASES = [(f, d, via) for f, d in SCALE_CASES if f.B > 1 for via in (("x", "t") if f.lora else ("x",))]


@pytest.mark.parametrize("fam,dtype,via", BATCH_CASES, ids=[f"{f.name}-{NPDT[d]}-via-{v}".replace(" ", "_") for f, d, v in BATCH_CASES])
def test_a_nan_or_inf_activation_row_spoils_its_own_outputs_only(fam, dtype, via):
    """NaN at one k of activation row 1, +Inf at a k of the last chunk of the last row - the row the kernels' clamp duplicates into
    the unused rows of a tile.  fp4_hip_gemm_lora_nf4 also through a non-finite row of t."""
    B, M, K = fam.B, fam.M, fam.K
    absmax = tabled_uniform_scales(M, K, fam.bs)
    x = np.random.default_rng(B).standard_normal((B, K)).astype(np.float32)
    _, kw, exact, scale = scale_inputs(fam, dtype, absmax, x)
    if via == "x":
        x[1, 70], x[B - 1, K - 3] = np.nan, np.inf
    else:
        t = kw["t"].cpu().numpy()
        t[1, 3], t[B - 1, fam.Rr - 1] = np.nan, np.inf
        kw["t"] = to_dev(t)
    y = fam.call(torch_values(x, dtype), **kw)
    got = y.double().cpu().numpy().reshape(B, M)
    assert not np.isfinite(got[[1, B - 1]]).any()  # (via t: a zero entry of lora_B gives 0 * NaN or 0 * Inf, non-finite as well)
    keep = [b for b in range(B) if b not in (1, B - 1)]
    assert np.isfinite(got[keep]).all()
    report("activation isolation", f"{fam.name} via {via}", dtype, y.reshape(B, M)[keep], exact[keep], scale[keep])


# ---- batch 1: a non-finite activation makes every output non-finite -----------------------------------------------------------------------
def b1(name, entry, K, **kw):
    return Family(name, entry, M=37, K=K, bs=32, dtypes=DTYPES, **kw)


B1_FAMILIES = [b1(f"{n} K{K}", e, K, **kw) for K in (96, 4128)  # C = 3 of a 32-chunk pass; C = 129 of a 256-chunk pass
               for n, e, kw in (("gemv table16", "gemv", dict(gemv_nf4=0)), ("gemv pair-table", "gemv", dict(gemv_nf4=1)),
                                ("gemv generic", "gemv", dict(misaligned=True)), ("gemv_fused", "fused", {}), ("gemv_lora", "lora", {}),
                                ("gemv_nested", "nested", {}))]
B1_CASES = [(f, d) for f in B1_FAMILIES for d in f.dtypes]


@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("where", ["first chunk", "last chunk"])
@pytest.mark.parametrize("fam,dtype", B1_CASES, ids=case_ids(B1_CASES))
def test_a_non_finite_activation_makes_every_batch_1_output_non_finite(fam, dtype, where, value):
    """Every row's sum holds the term x[k] * w[r][k], so no output may come back finite; whether it is NaN or a signed infinity is
    unspecified (include/torch_bnb_fp4_hip.h): in the last chunk of a K whose last pass is partial the value also reaches every row
    through the dead lanes' 0 * x."""
    M, K = fam.M, fam.K
    x = np.random.default_rng(K).standard_normal((1, K)).astype(np.float32)
    x[0, 5 if where == "first chunk" else K - 3] = value
    x_t, kw, _, _ = scale_inputs(fam, dtype, tabled_uniform_scales(M, K, fam.bs), x)
    got = fam.call(x_t, **kw).double().cpu().numpy()
    assert got.shape == (M,) and not np.isfinite(got).any(), (fam.name, int(np.isfinite(got).sum()))


@pytest.mark.parametrize("fam,dtype", [(f, d) for f, d in SCALE_CASES if d != F32], ids=case_ids([(f, d) for f, d in SCALE_CASES if d != F32]))
def test_large_activations(fam, dtype):
    """bf16 activations of 3e5 / 1e5 (beyond fp16's range) and fp16 ones of 6e4, alternating in sign, under scales of 2^-12: every
    product formed on the way must be an f32 one.  On the fp16 matrix-core paths the lo * 2^24 tile sees |lo| x up to 4096 * 6e4."""
    B, M, K = fam.B, fam.M, fam.K
    k, b = np.arange(K)[None, :], np.arange(B)[:, None]
    sign = np.where((k // 2 + k + b) % 2 == 0, 1.0, -1.0)
    mag = np.where(k % 2 == 0, 3.0e5, 1.0e5) if dtype == BF16 else np.full((1, K), 6.0e4)
    absmax = np.full(M * K // fam.bs, 2.0**-12, np.float32)
    x_t, kw, exact, scale = scale_inputs(fam, dtype, absmax, (sign * mag).astype(np.float32))
    assert np.abs(exact).max() < 3.0e4  # well inside fp16
    report("large activations", fam.name, dtype, fam.call(x_t, **kw), exact, scale)


# fp16 subnormal activations.  The contract is sum_k x[k] code absmax with f32 arithmetic, which does not flush, so the expectation is
# the float64 product at the usual bar; a family whose instruction flushes subnormal fp16 inputs would be listed here, with the flushed
# row's expectation pinned to what the header then documents.  The batch-1 kernels widen x to f32 before the first multiply; the
# matrix-core kernels feed x to v_mfma_f32_16x16x32_f16 as loaded (their own care about subnormal INPUTS covers the lo table only).
# None flushes (measured: profiles/nf4_constructed_inputs.txt, every family at 0.41-0.88 of the bar; a flushed row would be 0 against
# |exact| of 0.1 and more).
FLUSHES_F16_SUBNORMAL_X = frozenset()


def subnormal_rows(B, K):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((B, K)) * 2.0**-12).astype(np.float32)  # mostly normal fp16 values
    x[B // 2] = (rng.integers(16, 513, K) * rng.choice([-1.0, 1.0], K) * 2.0**-24).astype(np.float32)
    return x, B // 2


@pytest.mark.parametrize("fam", [f for f in SCALE_FAMILIES if F16 in f.dtypes], ids=lambda f: f.name.replace(" ", "_"))
def test_fp16_subnormal_activations(fam):
    B, M, K = fam.B, fam.M, fam.K
    x, sub = subnormal_rows(B, K)
    absmax = np.full(M * K // fam.bs, 2.0**16, np.float32)
    x_t, kw, exact, scale = scale_inputs(fam, F16, absmax, x)
    xs = x_t.reshape(B, K)[sub].float().abs()
    assert float(xs.max()) < 2.0**-14 and float(xs.min()) >= 2.0**-20  # every element of the row IS a subnormal, none was rounded away
    assert np.abs(exact[sub]).min() > 2.0**-14 and np.abs(exact).max() < 6.0e4  # normal outputs
    if fam.name in FLUSHES_F16_SUBNORMAL_X:
        exact[sub], scale[sub] = 0.0, 0.0
    report("fp16 subnormal activations", fam.name, F16, fam.call(x_t, **kw), exact, scale)


# ---- the down projection's special values -----------------------------------------------------------------------------------------------
def down_case(dtype, x, K=2048, Rr=24, seed=5):
    """(device x, A, scale, float64 t*, the bar's sum |scale_j| |A_jk| |x_k|) for activation rows x [B, K]."""
    rng = np.random.default_rng(seed)
    A = torch_values((rng.standard_normal((Rr, K)) / 32).astype(np.float32), dtype)
    s = C.down_scale(Rr)
    x_t = torch_values(x, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        x64, a64 = x_t.double().cpu().numpy(), A.double().cpu().numpy()
        return x_t, A, to_dev(s), (x64 @ a64.T) * s, (np.abs(x64) @ np.abs(a64).T) * np.abs(s)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("K", [2048, 8200])
def test_lora_down_a_nan_or_inf_activation_row_spoils_its_own_outputs_only(K, dtype):
    """Rows past the batch are clamped to the last row and a unit past the end of K re-reads the last unit of x under a zeroed A:
    +Inf in the last unit of the last row reaches 0 * Inf in its own row's sums only."""
    B = 5
    x = np.random.default_rng(B).standard_normal((B, K)).astype(np.float32)
    _, A, scale, exact, bound = down_case(dtype, x, K)
    x[1, 70], x[B - 1, K - 3] = np.nan, np.inf
    t = down(torch_values(x, dtype), A, scale)
    got = t.double().cpu().numpy()
    assert not np.isfinite(got[[1, B - 1]]).any()
    keep = [0, 2, 3]
    assert np.isfinite(got[keep]).all()
    report("activation isolation", f"lora_down K{K}", dtype, t[keep], exact[keep], bound[keep], F32)


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: NPDT[d])
def test_lora_down_large_activations(dtype):
    B, K = 5, 2048
    k, b = np.arange(K)[None, :], np.arange(B)[:, None]
    sign = np.where((k // 2 + k + b) % 2 == 0, 1.0, -1.0)
    mag = np.where(k % 2 == 0, 3.0e5, 1.0e5) if dtype == BF16 else np.full((1, K), 6.0e4)
    x_t, A, scale, exact, bound = down_case(dtype, (sign * mag).astype(np.float32))
    report("large activations", "lora_down", dtype, down(x_t, A, scale), exact, bound, F32)


def test_lora_down_fp16_subnormal_activations():
    x, sub = subnormal_rows(5, 2048)
    x_t, A, scale, exact, bound = down_case(F16, x)
    xs = x_t[sub].float().abs()
    assert float(xs.max()) < 2.0**-14 and float(xs.min()) >= 2.0**-20
    if "lora_down" in FLUSHES_F16_SUBNORMAL_X:
        exact[sub], bound[sub] = 0.0, 0.0
    report("fp16 subnormal activations", "lora_down", F16, down(x_t, A, scale), exact, bound, F32)


# ======================================================================================================================================
# 3. guards, shifted operands, repeats
# ======================================================================================================================================
M_GUARD = (1, 5, 33, 66, 257)
# every (ks, G) at the guard Ms (where iters is 1), then the generic kernel; every cell's placement case is run as it stands, below
GEMV_GUARD_SHAPES = ([(M, K, bs_of(K), False) for K in (992, 1056, 2080, 8224) for M in M_GUARD] +
                     [(M, K, bs, True) for K, bs in ((96, 32), (250, 50)) for M in M_GUARD])


def guard_inputs(M, K, bs, dtype, misaligned=False):
    rng = np.random.default_rng(1000 * M + K)
    packed = rng.integers(0, 256, M * K // 2, dtype=np.uint8)
    absmax = tabled_uniform_scales(M, K, bs, seed=M)
    x_t = torch_values(rng.standard_normal(K).astype(np.float32), dtype)
    w = R.dequantize_f32(packed, absmax, bs, M * K).astype(np.float64).reshape(M, K)
    x64 = x_t.double().cpu().numpy()
    if misaligned:
        x_t = placed(x_t, 1)
    return x_t, to_dev(packed), to_dev(absmax), w @ x64, np.abs(w) @ np.abs(x64)


def guarded_gemv(M, K, bs, dtype, x_t, P, A, exact, scale, misaligned=False):
    g = C.guard_elems(M)
    buf, out = C.guarded(M, dtype, g, dev())
    R.gemv(x_t, P, A, M, K, bs, out=out)
    assert C.guards_intact(buf, M, g), (M, K)
    assert_within_bar(out, exact, scale, dtype)
    first = out.clone()
    C.refill(buf)
    R.gemv(placed(x_t, 9) if misaligned else shifted(x_t, 8), shifted(P, 16), shifted(A, 4), M, K, bs, out=out)
    assert torch.equal(out, first) and C.guards_intact(buf, M, g), (M, K, "shifted / repeated")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["table16", "pair-table"])
def test_guards_plain_gemv_shifted_operands_and_repeats(layout, dtype):
    """fp4_hip_gemv_nf4: out between sentinel guards of guard_elems(M) >= max(4096, 2 M) elements, the bar, then shifted operands
    and a repeat into the re-filled buffer: the same bits."""
    for M, K, bs, misaligned in GEMV_GUARD_SHAPES:
        if misaligned and layout:
            continue  # the generic kernel has one table
        with forced(gemv_nf4=layout):
            guarded_gemv(M, K, bs, dtype, *guard_inputs(M, K, bs, dtype, misaligned), misaligned=misaligned)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["table16", "pair-table"])
@pytest.mark.parametrize("M,K", C.GEMV_PLACEMENT_CASES, ids=CELL_IDS)
def test_guards_plain_gemv_every_cell(M, K, layout):
    """The same in each of the 12 dispatch cells (iters 2 and 4 need thousands of rows, so the float64 reference is formed on the
    device, as tests/test_gpu_nf4_gemv.py forms it)."""
    bs = bs_of(K)
    P, A = NG._random_nf4(M * K, bs, 7919 * M + K)
    xs = [torch_values(np.random.default_rng(K).standard_normal(K).astype(np.float32), d) for d in DTYPES]
    exact, scale = NG.device_products(P, A, M, K, bs, xs)
    with forced(gemv_nf4=layout):
        for i, dtype in enumerate(DTYPES):
            guarded_gemv(M, K, bs, dtype, xs[i], P, A, exact[i].cpu().numpy(), scale[i].cpu().numpy())


GUARD_FAMILIES = [Family(f"{n} K{K}", e, K=K, dtypes=DTYPES) for K in (1024, 4096) for n, e in (("gemv_fused", "fused"), ("gemv_lora", "lora"), ("gemv_nested", "nested"))]
GUARD_CASES = [(f, d) for f in GUARD_FAMILIES for d in f.dtypes]


@pytest.mark.parametrize("fam,dtype", GUARD_CASES, ids=case_ids(GUARD_CASES))
def test_guards_fused_lora_and_nested_gemv(fam, dtype):
    """The 64-element guards of tests/test_gpu_nf4_fused.py / _lora.py / test_gpu_nested.py are less than a row at most shapes:
    here out sits between guard_elems(M) sentinels, for the plain epilogue with bias and residual (bit for bit the rounded adds on the
    bare sum) and for the gated one (M / 2 outputs and nothing more), and a repeat with shifted operands gives the same bits."""
    for M in M_GUARD:
        fam.M = M
        x_t, P, _, exact, scale = guard_inputs(M, fam.K, fam.bs, dtype)
        kw = dict(P=P, absmax=dev_absmax(fam, tabled_uniform_scales(M, fam.K, fam.bs, seed=M)))
        if fam.lora:
            kw["lB"], kw["t"], delta, dscale = fam.adapter(dtype)
            exact, scale = exact + delta[0], scale + dscale[0]
        rng = np.random.default_rng(M)
        b_t, r_t = torch_values(rng.standard_normal(M).astype(np.float32) * 0.1, dtype), torch_values(rng.standard_normal(M).astype(np.float32), dtype)
        g = C.guard_elems(M)
        buf, out = C.guarded(M, dtype, g, dev())
        fam.call(x_t, out=out, **kw)
        assert C.guards_intact(buf, M, g)
        assert_within_bar(out, exact, scale, dtype)
        bare = as_np(out)
        C.refill(buf)
        fam.call(x_t, bias=b_t, residual=r_t, out=out, **kw)
        want = (bare + as_np(b_t)) + as_np(r_t) if dtype == F32 else o.linear_epilogue(bare, NPDT[dtype], as_np(b_t), as_np(r_t))
        assert np.array_equal(as_np(out).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)) and C.guards_intact(buf, M, g)
        first = out.clone()
        C.refill(buf)
        kws = dict(kw, P=shifted(kw["P"], 16))
        if fam.entry != "nested":
            kws["absmax"] = shifted(kw["absmax"], 4)
        fam.call(shifted(x_t, 8), bias=shifted(b_t, 8), residual=shifted(r_t, 8), out=out, **kws)
        assert torch.equal(out, first) and C.guards_intact(buf, M, g)
        if M % 2 == 0 and dtype != F32:
            gbuf, gout = C.guarded(M // 2, dtype, g, dev())
            fam.call(x_t, epilogue=GATED, out=gout, **kw)
            y = torch.from_numpy(bare).to(dtype).to(dev())
            assert int(ulps16(gout, torch.nn.functional.silu(y[0::2]) * y[1::2]).max()) <= 1 and C.guards_intact(gbuf, M // 2, g)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NPDT[d])
def test_guards_lora_down(dtype):
    K, Rr = 4096, 24
    g = C.guard_elems(Rr)
    for rows in (1, 9, 64):
        x = np.random.default_rng(rows).standard_normal((rows, K)).astype(np.float32)
        x_t, A, scale, exact, bound = down_case(dtype, x, K, Rr)
        buf, t = C.guarded(rows * Rr, F32, g, dev())
        down(x_t, A, scale, t.view(rows, Rr))
        assert C.guards_intact(buf, rows * Rr, g)
        assert_within_bar(t.view(rows, Rr), exact, bound, F32)
        first = t.clone()
        C.refill(buf)
        down(shifted(x_t, 8), shifted(A, 8), shifted(scale, 4), t.view(rows, Rr))
        assert torch.equal(t, first) and C.guards_intact(buf, rows * Rr, g)
