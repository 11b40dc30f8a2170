"""The fused NF4 decode epilogues (fp4_hip_gemv_fused_nf4, fp4_hip_gemm_fused_nf4) through the C ABI, the torch ops and the modules.

The sums are covered by test_gpu_nf4_gemv.py / test_gpu_nf4_small_batch.py / test_gpu_nf4_wide_batch.py (float64 bar).  What is
new is elementwise, so it is held to the bars of tests/test_gpu_fused.py:
* plain epilogue: BIT FOR BIT the oracle's rounded adds (oracle.linear_epilogue) on what the plain entry point returns for the same
  operands - the fused kernel must form the same sum;
* gate|up epilogue: <= 1 ulp of T from torch's silu(g) * u (+ r) on the plain entry point's gate / up rows, >= 99.9 % identical
  at batch 1 (>= 99.8 % batched, and against the numpy oracle, whose exp may differ from the device's by an f32 ulp).
The (shape, rows) cases are tests/nf4_fused_cases.py's; tests/test_nf4_fused_host.py shows they reach every dispatcher cell."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st
from torch import nn

import hipabi
import nf4_fused_cases as FC
import nf4_ref as R
from gpu_util import NPDT, bits, dev
from oracle import fp4_oracle as o
from test_gpu_nf4_wide_batch import gemm as gemm_wide

pytestmark = pytest.mark.gpu
DT16 = [torch.bfloat16, torch.float16]
BS = 64
NONE, GATED = hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS
SENTINEL = 0x7BCD  # a finite bit pattern in both 16-bit formats that no test output equals by accident
GUARD = 64
COMMON = dict(deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)


def _lib():
    l = R.lib()
    if not getattr(l, "_nf4_fused_bound", False):
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        l.fp4_hip_gemv_fused_nf4.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemv_fused_nf4.restype = i32
        l.fp4_hip_gemm_fused_nf4.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemm_fused_nf4.restype = i32
        l._nf4_fused_bound = True
    return l


def gemv_fused(x, P, A, M, K, bs=BS, bias=None, residual=None, epilogue=NONE, out=None, expect_ok=True, dtype=None):
    if out is None:
        out = torch.empty(M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = _lib().fp4_hip_gemv_fused_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(A), hipabi._ptr(bias), hipabi._ptr(residual),
                                       hipabi._ptr(out), M, K, bs, hipabi.DT[dtype or x.dtype], epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def gemm_fused(x, P, A, M, K, bs=BS, bias=None, residual=None, epilogue=NONE, out=None, expect_ok=True, dtype=None, B=None):
    B = x.numel() // K if B is None else B
    if out is None:
        out = torch.empty(B, M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = _lib().fp4_hip_gemm_fused_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(A), hipabi._ptr(bias), hipabi._ptr(residual),
                                       hipabi._ptr(out), B, M, K, bs, hipabi.DT[dtype or x.dtype], epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def bs_of(K):
    """The blocksize of the batch-1 cases, as tests/test_gpu_nf4_gemv.py picks it: 64 where it divides K, else 32 (the fast path needs
    a blocksize that divides K)."""
    return 64 if K % 64 == 0 else 32


@functools.lru_cache(maxsize=8)
def weight(M, K, bs=BS):
    """Random NF4 bytes and scales on the device, made once per shape and only read."""
    g = torch.Generator(device=dev()).manual_seed(31 * M + K)
    packed = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev(), generator=g)
    absmax = torch.rand(M * K // bs, device=dev(), generator=g) * 0.05 + 0.005
    return packed, absmax


def rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(shape, device=dev(), generator=g) * scale).to(dtype)


def as_np(t):
    return t.float().cpu().numpy()


def ulps(a, b):
    """Distance of two 16-bit float tensors in units in the last place, on the device."""
    def line(t):
        v = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(v >= 0x8000, 0x8000 - v, v)
    return (line(a) - line(b)).abs()


def assert_close_ulp(got, ref, frac, what):
    d = ulps(got, ref)
    same = float((d == 0).float().mean())
    print(f"{what}: max ulp {int(d.max())}, identical {same:.5f} (bar: <= 1 ulp, >= {frac})")
    assert int(d.max()) <= 1 and same >= frac, (what, int(d.max()), same)


def guarded(n, dtype):
    """A sentinel-filled buffer with `n` elements between two guard regions; (whole buffer, the view a kernel writes)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=dev()).view(dtype)
    return buf, buf[GUARD:GUARD + n]


def untouched(buf, lo=0, hi=None):
    return bool((buf.view(torch.int16)[lo:hi] == SENTINEL).all())


def guards_intact(buf, n):
    return untouched(buf, 0, GUARD) and untouched(buf, GUARD + n, None)


# ---- batch 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", FC.GEMV_PLAIN, ids=[f"{m}x{k}" for m, k in FC.GEMV_PLAIN])
def test_gemv_bias_residual_epilogue_is_bit_exact(M, K):
    bs = bs_of(K)
    P, A = weight(M, K, bs)
    for dtype in DT16 + [torch.float32]:
        x, b, r = rand(K, dtype, K), rand(M, dtype, M, 0.1), rand(M, dtype, M + 1)
        for use_bias, use_res in ((False, True), (True, True), (True, False), (False, False)):
            plain = R.gemv(x, P, A, M, K, bs)  # no bias: the epilogue is redone from the bare sum
            buf, out = guarded(M, dtype) if dtype != torch.float32 else (None, None)
            got = gemv_fused(x, P, A, M, K, bs, b if use_bias else None, r if use_res else None, out=out)
            if dtype == torch.float32:  # plain f32 adds: sum, + bias, + residual
                want = as_np(plain)
                want = want + as_np(b) if use_bias else want
                want = want + as_np(r) if use_res else want
            else:
                want = o.linear_epilogue(as_np(plain), NPDT[dtype], as_np(b) if use_bias else None, as_np(r) if use_res else None)
                assert guards_intact(buf, M)
            assert np.array_equal(as_np(got).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (dtype, use_bias, use_res)
        # in place: residual aliases out (h = h + Linear(a)); and the same call twice gives the same bits
        h = r.clone()
        gemv_fused(x, P, A, M, K, bs, b, h, out=h)
        once = gemv_fused(x, P, A, M, K, bs, b, r)
        assert torch.equal(h, once) and torch.equal(once, gemv_fused(x, P, A, M, K, bs, b, r))


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,K", FC.GEMV_GATED, ids=[f"{m}x{k}" for m, k in FC.GEMV_GATED])
def test_gemv_gate_up_epilogue(M, K, with_bias):
    bs = bs_of(K)
    P, A = weight(M, K, bs)
    for dtype in DT16:
        x = rand(K, dtype, K, 2.0)  # gate values spread over a few units: silu is exercised off its linear part
        b = rand(M, dtype, M, 0.1) if with_bias else None
        r = rand(M // 2, dtype, M + 1)
        plain = R.gemv(x, P, A, M, K, bs, b)  # rows 2i = gate_i, 2i+1 = up_i, each already T(+bias)
        g, u = plain[0::2].contiguous(), plain[1::2].contiguous()
        buf, out = guarded(M // 2, dtype)
        got = gemv_fused(x, P, A, M, K, bs, b, None, GATED, out=out)
        assert guards_intact(buf, M // 2)
        got_r = gemv_fused(x, P, A, M, K, bs, b, r, GATED)
        ref = torch.nn.functional.silu(g) * u
        assert_close_ulp(got, ref, 0.999, (M, K, dtype, "gated vs torch"))
        assert_close_ulp(got_r, ref + r, 0.999, (M, K, dtype, "gated + residual vs torch"))
        want = o.silu_mul_epilogue(as_np(g), as_np(u), NPDT[dtype])
        want_t = torch.from_numpy(np.asarray(want, np.float32)).to(dtype).to(dev())
        assert torch.equal(want_t.float().cpu(), torch.from_numpy(np.asarray(want, np.float32)))  # the oracle's values are exact in T
        assert_close_ulp(got, want_t, 0.998, (M, K, dtype, "gated vs oracle"))
        # in place, and twice
        h = r.clone()
        gemv_fused(x, P, A, M, K, bs, b, h, GATED, out=h)
        assert torch.equal(h, got_r) and torch.equal(got_r, gemv_fused(x, P, A, M, K, bs, b, r, GATED))


def test_gemv_gate_up_against_float64_end_to_end():
    """The whole fused launch against float64, want = silu(g*) * u* with g*, u* the exact sums (nf4_ref.gemv_exact).  Tolerance:
    2^-8 * 1.02 * (3 |want| + 1.1 |g*| |u*|)  - the rounding chain of tests/test_gpu_fused.py's end-to-end item (g, u, silu and the
    product each carry <= half a bf16 ulp; |d silu / dg| <= 1.1) - plus the NF4 GEMV bar 1e-5 * S on both sums carried through the
    product, 1e-5 * (1.1 |u*| S_g + |silu(g*)| S_u), S = sum |x w| of the row, plus 1e-6."""
    M, K = 2048, 4096
    P, A = weight(M, K)
    x = rand(K, torch.bfloat16, 7)
    got = as_np(gemv_fused(x, P, A, M, K, BS, None, None, GATED)).astype(np.float64)
    exact, S = R.gemv_exact(as_np(x), P.cpu().numpy(), A.cpu().numpy(), M, K, BS)
    g, u, Sg, Su = exact[0::2], exact[1::2], S[0::2], S[1::2]
    sil = g / (1.0 + np.exp(-g))
    want = sil * u
    tol = 2.0**-8 * 1.02 * (3 * np.abs(want) + 1.1 * np.abs(g) * np.abs(u)) + 1e-5 * (1.1 * np.abs(u) * Sg + np.abs(sil) * Su) + 1e-6
    ratio = float((np.abs(got - want) / tol).max())
    print(f"end to end vs float64: worst |err| / tol = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("variant", [0, 1])
def test_gemv_both_table_layouts(variant):
    try:
        hipabi.set_variant("gemv_nf4", variant)
        for M, K in FC.GEMV_VARIANT_SHAPES:
            bs = bs_of(K)
            P, A = weight(M, K, bs)
            for dtype in DT16:
                x, b, r = rand(K, dtype, K, 2.0), rand(M, dtype, M, 0.1), rand(M, dtype, M + 1)
                plain = R.gemv(x, P, A, M, K, bs)
                want = o.linear_epilogue(as_np(plain), NPDT[dtype], as_np(b), as_np(r))
                got = gemv_fused(x, P, A, M, K, bs, b, r)
                assert np.array_equal(as_np(got).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (variant, M, K, dtype)
                pb = R.gemv(x, P, A, M, K, bs, b)
                ref = torch.nn.functional.silu(pb[0::2]) * pb[1::2] + r[: M // 2]
                assert_close_ulp(gemv_fused(x, P, A, M, K, bs, b, r[: M // 2].contiguous(), GATED), ref, 0.999, (variant, M, K, dtype))
    finally:
        hipabi.set_variant("gemv_nf4", -1)


def test_gemv_refusals_leave_out_untouched():
    M, K = 64, 1024
    P, A = weight(M, K)
    x16 = rand(K + 8, torch.bfloat16, 1)
    buf, out = guarded(M, torch.bfloat16)
    # gated + f32
    x32 = rand(K, torch.float32, 1)
    out32 = torch.full((M,), 123.0, device=dev())
    assert gemv_fused(x32, P, A, M, K, BS, None, None, GATED, out=out32, expect_ok=False) == hipabi.ERR_UNSUPPORTED
    assert "not available" in hipabi.last_error() and bool((out32 == 123.0).all())
    # K % 32 != 0 (blocksize 16 divides it), both epilogues; misaligned x, both epilogues
    for epi in (GATED, NONE):
        assert gemv_fused(x16[:1008], P, A, M, 1008, 16, None, None, epi, out=out, expect_ok=False) == hipabi.ERR_UNSUPPORTED
        assert "not available" in hipabi.last_error()
        assert gemv_fused(x16[1:K + 1], P, A, M, K, BS, None, None, epi, out=out, expect_ok=False) == hipabi.ERR_UNSUPPORTED
    assert gemv_fused(x16[:K], P, A, M - 1, K, BS, None, None, GATED, out=out, expect_ok=False) == hipabi.ERR_INVALID
    assert "even row count" in hipabi.last_error()
    assert gemv_fused(x16[:K], P, A, M, K, BS, None, None, 7, out=out, expect_ok=False) == hipabi.ERR_INVALID
    assert gemv_fused(x16[:K], P, A, 0, K, BS, None, None, GATED, out=out) is out
    torch.cuda.synchronize()
    assert untouched(buf)


# ---- 2..128 rows ---------------------------------------------------------------------------------------------------------------------
def _batched_case(M, K, dtype, rows_list):
    P, A = weight(M, K)
    xs = rand((128, K), dtype, K + 3)
    b = rand(M, dtype, M, 0.1)
    rs = rand((128, M), dtype, M + 5)  # distinct per element: a wrong row stride or chunk offset cannot pass
    for B in rows_list:
        x, r = xs[:B].contiguous(), rs[:B].contiguous()
        plain = gemm_wide(x, P, A, M, K, bias=b)
        buf, out = guarded(B * M, dtype)
        got = gemm_fused(x, P, A, M, K, BS, b, r, out=out.view(B, M))
        assert guards_intact(buf, B * M)
        want = o.linear_epilogue(as_np(plain), NPDT[dtype], None, as_np(r))
        assert np.array_equal(as_np(got).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (M, K, B, dtype)
        assert torch.equal(gemm_fused(x, P, A, M, K, BS, b, None), plain)
        assert torch.equal(gemm_fused(x, P, A, M, K, BS, None, None), gemm_wide(x, P, A, M, K))
        h = r.clone()
        gemm_fused(x, P, A, M, K, BS, b, h, out=h)
        assert torch.equal(h, got)
        # gate | up
        rh = rs[:B, : M // 2].contiguous()
        buf, out = guarded(B * (M // 2), dtype)
        gu = gemm_fused(x, P, A, M, K, BS, b, None, GATED, out=out.view(B, M // 2))
        assert guards_intact(buf, B * (M // 2)) and gu.shape == (B, M // 2)
        gur = gemm_fused(x, P, A, M, K, BS, b, rh, GATED)
        ref = torch.nn.functional.silu(plain[:, 0::2]) * plain[:, 1::2]
        assert_close_ulp(gu, ref, 0.998, (M, K, B, dtype, "gated"))
        assert_close_ulp(gur, ref + rh, 0.998, (M, K, B, dtype, "gated + residual"))
        h = rh.clone()
        gemm_fused(x, P, A, M, K, BS, b, h, GATED, out=h)
        assert torch.equal(h, gur) and torch.equal(gur, gemm_fused(x, P, A, M, K, BS, b, rh, GATED))


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("M,K", FC.BATCH_SHAPES, ids=[f"{m}x{k}" for m, k in FC.BATCH_SHAPES])
def test_batched_epilogues_every_tile_count_chunking_and_cell(M, K, dtype):
    _batched_case(M, K, dtype, FC.rows_for(K))


@pytest.mark.parametrize("variant,shape", [(1, (16400, 768)), (2, (258, 2048))])
def test_batched_both_forced_workgroup_shapes(variant, shape):
    """fp4_hip_set_variant("gemm_wide_nf4", 1 / 2): 16 rows per workgroup on a tall weight, 32 on a short one whose last tile is partial."""
    try:
        hipabi.set_variant("gemm_wide_nf4", variant)
        for dtype in DT16:
            _batched_case(*shape, dtype, [17, 64, 65])
    finally:
        hipabi.set_variant("gemm_wide_nf4", -1)


def test_batched_refusals_leave_out_untouched():
    M, K = 64, 1024
    P, A = weight(M, K)
    x = rand((4, K + 8), torch.bfloat16, 2).reshape(-1)
    buf, out = guarded(4 * M, torch.bfloat16)
    call = lambda *a, **k: gemm_fused(*a, out=out, expect_ok=False, **k)
    for epi in (NONE, GATED):
        assert call(x, P, A, M, K, 32, None, None, epi, B=4) == hipabi.ERR_UNSUPPORTED and "not covered" in hipabi.last_error()
        assert call(x, P, A, M, 992, 64, None, None, epi, B=4) == hipabi.ERR_UNSUPPORTED           # K % 64 != 0
        assert call(x[1:], P, A, M, K, 64, None, None, epi, B=4) == hipabi.ERR_UNSUPPORTED          # misaligned x
        assert call(x, P, A, M, K, 64, None, None, epi, B=4, dtype=torch.float32) == hipabi.ERR_UNSUPPORTED
        assert call(x, P, A, M, K, 64, None, None, epi, B=129) == hipabi.ERR_UNSUPPORTED
        assert call(x, P, A, 0, K, 64, None, None, epi, B=4) == hipabi.OK
    assert call(x, P, A, M - 1, K, 64, None, None, GATED, B=4) == hipabi.ERR_INVALID and "even row count" in hipabi.last_error()
    assert call(x, P, A, M, K, 64, None, None, 5, B=4) == hipabi.ERR_INVALID
    torch.cuda.synchronize()
    assert untouched(buf)


# ---- ops and modules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16)
def test_torch_ops_equal_the_c_abi_bit_for_bit(dtype):
    import torch_bnb_fp4 as pkg

    for M, K in ((1026, 3104), (258, 2048)):
        bs = bs_of(K)
        P, A = weight(M, K, bs)
        Bt = P.reshape(-1, 1).t()
        b = rand(M, dtype, M, 0.1)
        for rows in (1, 5, 40):
            if rows > 1 and K % 64:
                continue
            x = rand((rows, K), dtype, rows, 2.0)
            for epi in (NONE, GATED):
                r = rand((rows, M // 2 if epi == GATED else M), dtype, 9)
                if rows == 1:
                    got = pkg.ext.gemv_nf4_fused(x, Bt, A, bs, [M, K], b, r, epi)
                    want = gemv_fused(x.reshape(-1), P, A, M, K, bs, b, r.reshape(-1), epi).reshape(1, -1)
                    assert torch.equal(got, want)
                if K % 64 == 0:
                    got = pkg.ext.gemm_nf4_fused(x, Bt, A, BS, [M, K], b, r, epi)
                    assert torch.equal(got, gemm_fused(x, P, A, M, K, BS, b, r, epi))
                    assert got.shape == (rows, M // 2 if epi == GATED else M)
    with pytest.raises(RuntimeError, match="not available"):
        pkg.ext.gemv_nf4_fused(rand((1, 1008), dtype, 1), weight(64, 1024, 16)[0].reshape(-1, 1).t(), weight(64, 1024, 16)[1], 16, [64, 1008], None, None, NONE)
    with pytest.raises(RuntimeError, match="not covered"):
        pkg.ext.gemm_nf4_fused(rand((4, 992), dtype, 1), weight(64, 1024)[0].reshape(-1, 1).t(), weight(64, 1024)[1], 64, [64, 992], None, None, NONE)


class _MLP(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = nn.Linear(H, I), nn.Linear(H, I), nn.Linear(I, H)
        self.act_fn = nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


def test_fused_nf4_mlp_matches_the_unfused_modules_and_replays_from_a_graph():
    import torch_bnb_fp4 as pkg

    H, I = 512, 1408
    torch.manual_seed(11)
    root = nn.Sequential(_MLP(H, I).to(torch.bfloat16))
    root = pkg.recursively_replace_with_fp4_linear(root, as_dtype=torch.bfloat16, device=dev(), quant_type="nf4")
    mlp = root[0]
    gate, up, down = mlp.gate_proj, mlp.up_proj, mlp.down_proj
    assert all(l.quant_data.nf4 for l in (gate, up, down))
    unfused = lambda h: h + down(torch.nn.functional.silu(gate(h)) * up(h))
    h = rand((1, H), torch.bfloat16, 5)
    want = unfused(h)
    assert pkg.fuse_gated_mlps(root) == 0
    assert pkg.fuse_gated_mlps(root, nf4=True) == 1
    fused_mlp = root[0]
    assert isinstance(fused_mlp, pkg.FusedGatedMLP) and type(fused_mlp.gate_up) is pkg.FusedNF4Linear
    dn = pkg.FusedNF4Linear.from_linear(down)
    gu = fused_mlp.gate_up
    assert gu.out_features == I
    # batch 1: a 1-ulp silu difference can pass through down's sum
    for got in (h + fused_mlp(h), dn(gu(h), residual=h)):
        d = ulps(got, want)
        print(f"fused NF4 MLP, batch 1: max ulp {int(d.max())}, identical {float((d == 0).float().mean()):.4f}")
        assert got.shape == want.shape and int(d.max()) <= 2 and float((d == 0).float().mean()) >= 0.99
    # 2 and 24 rows: the batched kernels with the same epilogues (the FP4 test's batched tolerance)
    for rows in (2, 24):
        hb = rand((rows, H), torch.bfloat16, rows, 0.5)
        wantb = unfused(hb)
        for gotb in (hb + fused_mlp(hb), dn(gu(hb), residual=hb)):
            assert gotb.shape == wantb.shape and (gotb.float() - wantb.float()).abs().max() <= 2e-2 * wantb.float().abs().max()
    # 65+ rows: the unfused sequence (dequant + GEMM over the interleaved weight), same semantics
    hb = rand((70, H), torch.bfloat16, 70, 0.5)
    gotb, wantb = dn(gu(hb), residual=hb), unfused(hb)
    assert gotb.shape == wantb.shape and (gotb.float() - wantb.float()).abs().max() <= 2e-2 * wantb.float().abs().max()
    # graph replay equals eager
    step = pkg.GraphedStep(lambda t: dn(gu(t), residual=t), h)
    for scale in (1.0, 0.75, -0.5):
        assert torch.equal(step(h * scale), dn(gu(h * scale), residual=h * scale))
    step8 = pkg.GraphedStep(lambda t: dn(gu(t), residual=t), rand((8, H), torch.bfloat16, 8))
    h8 = rand((8, H), torch.bfloat16, 88)
    assert torch.equal(step8(h8), dn(gu(h8), residual=h8))


@settings(max_examples=100, **COMMON)
@given(M2=st.integers(1, 2048), u=st.integers(1, 128), rows=st.integers(1, 64), gated=st.booleans(), with_bias=st.booleans(),
       with_res=st.booleans(), dtype=st.sampled_from(DT16))
def test_hypothesis_draws(M2, u, rows, gated, with_bias, with_res, dtype):
    """Any even M <= 4096, K % 64 == 0 up to 8192, 1..64 rows: the fused call against the plain entry point followed by torch's own
    ops.  Plain epilogue: equal bits.  Gated: <= 1 ulp, and at most 0.2 % + 3 elements off (the 99.8 % bar, with room for the few
    elements of a small draw: one differing element of M/2 = 2 is no more evidence than one of 2000)."""
    M, K = 2 * M2, 64 * u
    g = torch.Generator(device=dev()).manual_seed(M * 131 + u)
    P = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev(), generator=g)
    A = torch.rand(M * K // BS, device=dev(), generator=g) * 0.05 + 0.005
    x = rand((rows, K), dtype, rows + u, 2.0)
    b = rand(M, dtype, M, 0.1) if with_bias else None
    r = rand((rows, M // 2 if gated else M), dtype, 3) if with_res else None
    if rows == 1:
        plain = R.gemv(x.reshape(-1), P, A, M, K, BS, b).reshape(1, M)
        got = gemv_fused(x.reshape(-1), P, A, M, K, BS, b, None if r is None else r.reshape(-1), GATED if gated else NONE).reshape(1, -1)
    else:
        plain = gemm_wide(x, P, A, M, K, bias=b)
        got = gemm_fused(x, P, A, M, K, BS, b, r, GATED if gated else NONE)
    want = torch.nn.functional.silu(plain[:, 0::2]) * plain[:, 1::2] if gated else plain
    if r is not None:
        want = want + r
    if gated:
        d = ulps(got, want)
        assert int(d.max()) <= 1 and int((d != 0).sum()) <= 0.002 * d.numel() + 3, (M, K, rows, int(d.max()), int((d != 0).sum()))
    else:
        assert torch.equal(got, want), (M, K, rows)
