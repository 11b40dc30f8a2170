"""LoRA adapters beside NF4 weights on the GPU: fp4_hip_lora_down, fp4_hip_gemv_lora_nf4, fp4_hip_gemm_lora_nf4 through the C ABI,
the torch ops, LoRANF4Linear and attach_lora / load_lora_adapter.

Checker: float64 on the device.  y* = W x + B (s A x) from the exact f32 weights (device_products of tests/test_gpu_nf4_gemv.py, the
adapter terms added here in float64).  Bars - both terms are the project's GEMV bar, applied per f32 accumulation:
* down kernel:  |t - t*| <= 2^-24 * 1.01 * |t*| + 1e-5 * |scale_j| * sum_k |A_jk x_k|;
* fused ops:    |y - y*| <= ulp_T(y*)/2 * 1.01 + 1e-5 * sum_k |x_k w_rk| + 2e-5 * sum_j |B_rj| |scale_j| sum_k |A_jk x_k|
  (2e-5: the adapter passes through two f32 accumulations);
* the layer's unfused fallback rounds the base once before the adapter joins: the first term becomes ulp/2 * 1.01 * (|base*| + |y*|).
Adapters are of the base's magnitude (A ~ N(0,1)/sqrt(K), B ~ 0.05 N(0,1), s = 2: median |delta| / |y| about 0.4), so a wrong
adapter term cannot hide in the tolerance.  Elementwise epilogues and identities are held bit for bit."""
import json
import math

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nf4_fused_cases as FC
import nf4_lora_cases as LC
import nf4_ref as R
from gpu_util import dev
from test_gpu_nf4_fused import (GATED, NONE, as_np, assert_close_ulp, bs_of, gemm_fused, gemv_fused, guarded, guards_intact, rand,
                                untouched, weight)
from test_gpu_nf4_gemv import device_products

pytestmark = pytest.mark.gpu
DT16 = [torch.bfloat16, torch.float16]
DT3 = DT16 + [torch.float32]
HALF = {torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8, torch.float32: 2.0**-24}
BS = 64
S = 2.0


@pytest.fixture(autouse=True)
def _nf4_variant():
    hipabi.set_variant("gemv_nf4", -1)
    yield
    hipabi.set_variant("gemv_nf4", -1)


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def down(x, A, scale, t=None, expect_ok=True):
    K = A.shape[1]
    rows = x.numel() // K
    if t is None:
        t = torch.empty(rows, A.shape[0], dtype=torch.float32, device=x.device)
    rc = LC.lib().fp4_hip_lora_down(hipabi._ptr(x), hipabi._ptr(A), hipabi._ptr(scale), hipabi._ptr(t), rows, A.shape[0], K,
                                    hipabi.DT[x.dtype], hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return t
    return rc


def gemv_lora(x, P, Am, M, K, lB, t, bs=BS, bias=None, residual=None, epilogue=NONE, out=None, expect_ok=True, Rr=None):
    if out is None:
        out = torch.empty(M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = LC.lib().fp4_hip_gemv_lora_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(Am), hipabi._ptr(bias), hipabi._ptr(residual),
                                        hipabi._ptr(lB), hipabi._ptr(t), lB.shape[1] if Rr is None else Rr, hipabi._ptr(out), M, K, bs,
                                        hipabi.DT[x.dtype], epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def gemm_lora(x, P, Am, M, K, lB, t, bs=BS, bias=None, residual=None, epilogue=NONE, out=None, expect_ok=True, Rr=None, B=None):
    B = x.numel() // K if B is None else B
    if out is None:
        out = torch.empty(B, M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = LC.lib().fp4_hip_gemm_lora_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(Am), hipabi._ptr(bias), hipabi._ptr(residual),
                                        hipabi._ptr(lB), hipabi._ptr(t), lB.shape[1] if Rr is None else Rr, hipabi._ptr(out), B, M, K, bs,
                                        hipabi.DT[x.dtype], epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def adapter(M, K, r, dtype, seed):
    """A ~ N(0,1)/sqrt(K) [r, K], B ~ 0.05 N(0,1) [M, r] in ``dtype``, scale = 2 for every row."""
    return rand((r, K), dtype, seed, 1.0 / math.sqrt(K)), rand((M, r), dtype, seed + 1, 0.05), torch.full((r,), S, device=dev())


def adapter_terms(x, A, lB, scale):
    """float64 (B (s A x), |B| (|s| |A| |x|)) for the rows of x: [rows, M] each."""
    xd = x.double().reshape(-1, A.shape[1])
    t = (xd @ A.double().t()) * scale.double()
    ta = (xd.abs() @ A.double().abs().t()) * scale.double().abs()
    return t @ lB.double().t(), ta @ lB.double().abs().t()


def check(y, exact, s1, s2, dtype, what, base=None, weights_rounded=False):
    """``base``: the unfused fallback's bar.  ``weights_rounded``: the base came from dequant + GEMM, whose weights are rounded to
    T before the product - each |x_k w_rk| is off by at most ulp_T/2 of itself, so the bar gains ulp_T/2 * sum_k |x_k w_rk|."""
    first = exact.abs() if base is None else exact.abs() + base.abs()
    tol = HALF[dtype] * 1.01 * first + 1e-5 * s1 + 2e-5 * s2 + 1e-30
    if weights_rounded:
        tol = tol + HALF[dtype] * s1
    err = (y.double().reshape(exact.shape) - exact).abs()
    worst = float((err / tol).max())
    print(f"{what}: worst |err| / tol = {worst:.3f}")
    assert worst <= 1.0, (what, worst, int((err / tol).argmax()))


# ---- the down projection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT3, ids=str)
def test_down_kernel_every_k_rank_and_row_count(dtype):
    for K in LC.DOWN_K:
        x = rand((64, K), dtype, K)
        A = rand((256, K), dtype, K + 1, 1.0 / math.sqrt(K))
        scale = rand((256,), torch.float32, K + 2, 2.0)  # per row, both signs
        exact = x.double() @ A.double().t() * scale.double()
        bound = x.double().abs() @ A.double().abs().t() * scale.abs().double()
        worst = 0.0
        for Rr in LC.DOWN_R:
            for rows in LC.DOWN_ROWS:
                buf = torch.full((rows * Rr + 128,), float("nan"), device=dev())
                t = down(x[:rows], A[:Rr], scale[:Rr], buf[64:64 + rows * Rr].view(rows, Rr))
                assert bool(buf[:64].isnan().all()) and bool(buf[64 + rows * Rr:].isnan().all())
                tol = 2.0**-24 * 1.01 * exact[:rows, :Rr].abs() + 1e-5 * bound[:rows, :Rr] + 1e-30
                err = (t.double() - exact[:rows, :Rr]).abs()
                assert bool((err <= tol).all()), (K, Rr, rows, float((err / tol).max()))
                worst = max(worst, float((err / tol).max()))
        print(f"lora_down {dtype} K={K}: worst |err| / tol = {worst:.3f}")


def test_down_kernel_is_deterministic_and_refuses_what_it_does_not_cover():
    K = 4096
    x, A, scale = rand((17, K), torch.bfloat16, 1), rand((24, K), torch.bfloat16, 2, 1.0 / 64), torch.full((24,), S, device=dev())
    assert torch.equal(down(x, A, scale), down(x, A, scale))
    # a row of t depends on its own row of x only, whatever the batch it sits in
    assert torch.equal(down(x, A, scale)[3], down(x[3:4].contiguous(), A, scale)[0])
    t = torch.full((17, 24), 7.0, device=dev())
    assert down(x, A[:12], scale, t, expect_ok=False) == hipabi.ERR_UNSUPPORTED                      # rank 12
    assert down(x.reshape(-1)[4:4 + 16 * K], A, scale, t, expect_ok=False) == hipabi.ERR_UNSUPPORTED  # misaligned x
    assert LC.lib().fp4_hip_lora_down(hipabi._ptr(x), hipabi._ptr(A), hipabi._ptr(scale), hipabi._ptr(t), 65, 24, K, hipabi.BF16,
                                      hipabi._stream()) == hipabi.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((t == 7.0).all())


# ---- batch 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", FC.GEMV_PLAIN, ids=[f"{m}x{k}" for m, k in FC.GEMV_PLAIN])
def test_gemv_plain_epilogue_every_cell(M, K):
    bs = bs_of(K)
    P, Am = weight(M, K, bs)
    xs = [rand(K, dt, K) for dt in DT3]
    exact, s1 = device_products(P, Am, M, K, bs, xs)
    for i, dtype in enumerate(DT3):
        for Rr in LC.RANKS:
            A, lB, scale = adapter(M, K, Rr, dtype, 7 * Rr + i)
            d, s2 = adapter_terms(xs[i], A, lB, scale)
            t = down(xs[i], A, scale)
            buf, out = guarded(M, dtype) if dtype != torch.float32 else (None, None)
            y = gemv_lora(xs[i], P, Am, M, K, lB, t, bs, out=out)
            assert buf is None or guards_intact(buf, M)
            check(y, exact[i] + d[0], s1[i], s2[0], dtype, (M, K, Rr, dtype))


@pytest.mark.parametrize("variant", [0, 1])
def test_gemv_other_ranks_both_table_layouts_and_the_bias(variant):
    hipabi.set_variant("gemv_nf4", variant)
    for M, K in FC.GEMV_VARIANT_SHAPES:
        bs = bs_of(K)
        P, Am = weight(M, K, bs)
        xs = [rand(K, dt, K) for dt in DT3]
        exact, s1 = device_products(P, Am, M, K, bs, xs)
        for i, dtype in enumerate(DT3):
            b = rand(M, dtype, M, 0.1)
            for Rr in LC.RANKS_EXTRA:
                A, lB, scale = adapter(M, K, Rr, dtype, Rr + i)
                d, s2 = adapter_terms(xs[i], A, lB, scale)
                t = down(xs[i], A, scale)
                y = gemv_lora(xs[i], P, Am, M, K, lB, t, bs)
                check(y, exact[i] + d[0], s1[i], s2[0], dtype, (variant, M, K, Rr, dtype))
                # the bias is one more rounded add on the rounded sum: T(T(sum') + bias), bit for bit
                yb = gemv_lora(xs[i], P, Am, M, K, lB, t, bs, bias=b)
                assert torch.equal(yb, (y.float() + b.float()).to(dtype)), (variant, M, K, Rr, dtype)


@pytest.mark.parametrize("M,K", FC.GEMV_GATED, ids=[f"{m}x{k}" for m, k in FC.GEMV_GATED])
def test_gemv_gated_epilogue_is_torch_silu_mul_of_the_plain_lora_rows(M, K):
    """Bit for bit T(T(silu(y[0::2])) * y[1::2]) computed by torch from the plain-epilogue LoRA output of the same interleaved weight
    and B; the residual is one more rounded add, T(t + residual), also with `residual` aliasing `out`."""
    bs = bs_of(K)
    P, Am = weight(M, K, bs)
    for dtype in DT16:
        x = rand(K, dtype, K, 2.0)
        A, lB, scale = adapter(M, K, 16, dtype, M + K)
        t = down(x, A, scale)
        r = rand(M // 2, dtype, M + 1)
        y = gemv_lora(x, P, Am, M, K, lB, t, bs)
        want = torch.nn.functional.silu(y[0::2]) * y[1::2]
        buf, out = guarded(M // 2, dtype)
        got = gemv_lora(x, P, Am, M, K, lB, t, bs, epilogue=GATED, out=out)
        assert guards_intact(buf, M // 2)
        off = int((got != want).sum())
        print(f"gated {M}x{K} {dtype}: {off} of {M // 2} elements differ from torch's silu * up")
        assert torch.equal(got, want), (M, K, dtype, off)
        got_r = gemv_lora(x, P, Am, M, K, lB, t, bs, residual=r, epilogue=GATED)
        assert torch.equal(got_r, got + r)
        h = r.clone()
        gemv_lora(x, P, Am, M, K, lB, t, bs, residual=h, epilogue=GATED, out=h)
        assert torch.equal(h, got_r)
        # plain epilogue: the same residual rule, in place as well
        rp = rand(M, dtype, M + 2)
        h = rp.clone()
        gemv_lora(x, P, Am, M, K, lB, t, bs, residual=h, out=h)
        assert torch.equal(h, y + rp) and torch.equal(gemv_lora(x, P, Am, M, K, lB, t, bs, residual=rp), y + rp)


# ---- identities ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT3, ids=str)
def test_zero_adapter_gives_the_plain_fused_ops_values(dtype):
    for M, K in ((1026, 3104), (258, 2048), (4098, 4160)):
        bs = bs_of(K)
        P, Am = weight(M, K, bs)
        Rr = 24
        A, lB, scale = adapter(M, K, Rr, dtype, 5)
        for rows in (1, 5, 33):
            if rows > 1 and (dtype == torch.float32 or K % 64):
                continue
            x = rand((rows, K), dtype, rows, 2.0)
            b = rand(M, dtype, M, 0.1)
            t = down(x, A, scale)
            zeros = (torch.zeros_like(lB), t), (lB, torch.zeros_like(t))
            for epi in (NONE, GATED):
                if epi == GATED and dtype == torch.float32:
                    continue
                r = rand((rows, M // 2 if epi == GATED else M), dtype, 9)
                for zB, zt in zeros:
                    if rows == 1:
                        want = gemv_fused(x.reshape(-1), P, Am, M, K, bs, b, r.reshape(-1), epi)
                        got = gemv_lora(x.reshape(-1), P, Am, M, K, zB, zt, bs, b, r.reshape(-1), epi)
                    else:
                        want = gemm_fused(x, P, Am, M, K, BS, b, r, epi)
                        got = gemm_lora(x, P, Am, M, K, zB, zt, BS, b, r, epi)
                    assert torch.equal(got.float(), want.float()), (M, K, rows, epi, dtype)  # value for value (-0 + 0 = +0)


def test_one_hot_adapter_adds_t_in_one_f32_add():
    """f32, one-hot rows of B: out[r] == plain[r] + t[j(r)] in one f32 add, bit for bit, at every row of tail-carrying shapes
    (one per K band count, both KSPLIT forms of the delta's path)."""
    for M, K in FC.GEMV_VARIANT_SHAPES:
        bs = bs_of(K)
        P, Am = weight(M, K, bs)
        x = rand(K, torch.float32, K)
        for Rr in (8, 40, 256):
            A, _, scale = adapter(M, K, Rr, torch.float32, Rr)
            j = (torch.arange(M, device=dev()) * 7 + 3) % Rr
            lB = torch.zeros(M, Rr, device=dev())
            lB[torch.arange(M, device=dev()), j] = 1.0
            t = down(x, A, scale)
            plain = R.gemv(x, P, Am, M, K, bs)
            got = gemv_lora(x, P, Am, M, K, lB, t, bs)
            assert torch.equal(got, plain + t[0][j]), (M, K, Rr)


# ---- 2..64 rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16, ids=str)
@pytest.mark.parametrize("M,K", FC.BATCH_SHAPES, ids=[f"{m}x{k}" for m, k in FC.BATCH_SHAPES])
def test_batched_both_epilogues_every_tile_count_and_cell(M, K, dtype):
    P, Am = weight(M, K)
    xs = rand((64, K), dtype, K + 3)
    rs = rand((64, M), dtype, M + 5)
    exact, s1 = device_products(P, Am, M, K, BS, list(xs))
    for Rr in LC.RANKS:
        A, lB, scale = adapter(M, K, Rr, dtype, Rr)
        d, s2 = adapter_terms(xs, A, lB, scale)
        for B in LC.batch_rows(K):
            x, r = xs[:B].contiguous(), rs[:B].contiguous()
            t = down(x, A, scale)
            buf, out = guarded(B * M, dtype)
            y = gemm_lora(x, P, Am, M, K, lB, t, out=out.view(B, M))
            assert guards_intact(buf, B * M)
            check(y, exact[:B] + d[:B], s1[:B], s2[:B], dtype, (M, K, Rr, B, dtype))
            # residual: one more rounded add, in place as well
            h = r.clone()
            gemm_lora(x, P, Am, M, K, lB, t, residual=h, out=h)
            assert torch.equal(h, y + r)
            # gate|up on the same rows (the bar of tests/test_gpu_nf4_fused.py's batched gated case: <= 1 ulp, >= 99.8 % identical)
            rh = rs[:B, : M // 2].contiguous()
            buf, out = guarded(B * (M // 2), dtype)
            gu = gemm_lora(x, P, Am, M, K, lB, t, epilogue=GATED, out=out.view(B, M // 2))
            assert guards_intact(buf, B * (M // 2))
            ref = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
            assert_close_ulp(gu, ref, 0.998, (M, K, Rr, B, dtype, "gated"))
            assert torch.equal(gemm_lora(x, P, Am, M, K, lB, t, residual=rh, epilogue=GATED), gu + rh)


def test_batched_bias_joins_the_f32_sum_before_the_one_rounding():
    M, K, Rr = 258, 2048, 16
    P, Am = weight(M, K)
    for dtype in DT16:
        xs = rand((40, K), dtype, 3)
        b = rand(M, dtype, M, 0.1)
        A, lB, scale = adapter(M, K, Rr, dtype, 4)
        exact, s1 = device_products(P, Am, M, K, BS, list(xs))
        d, s2 = adapter_terms(xs, A, lB, scale)
        for B in (5, 40):
            y = gemm_lora(xs[:B].contiguous(), P, Am, M, K, lB, down(xs[:B].contiguous(), A, scale), bias=b)
            check(y, exact[:B] + d[:B] + b.double(), s1[:B] + b.double().abs(), s2[:B], dtype, (B, dtype, "bias"))


# ---- refusals, determinism, capture --------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched():
    M, K = 64, 1024
    P, Am = weight(M, K)
    x = rand((4, K + 8), torch.bfloat16, 1).reshape(-1)
    lB = rand((M + 1, 264), torch.bfloat16, 2)
    t = torch.zeros(4 * 264 + 8, device=dev())
    buf, out = guarded(4 * M, torch.bfloat16)
    U, I = hipabi.ERR_UNSUPPORTED, hipabi.ERR_INVALID
    v = lambda *a, **k: gemv_lora(*a, out=out, expect_ok=False, **k)
    m = lambda *a, **k: gemm_lora(*a, out=out, expect_ok=False, B=4, **k)
    for epi in (NONE, GATED):
        for call in (v, m):
            assert call(x, P, Am, M, K, lB, t, epilogue=epi, Rr=12) == U and "not available" in hipabi.last_error()
            assert call(x, P, Am, M, K, lB, t, epilogue=epi, Rr=264) == U
            assert call(x, P, Am, M, K, lB.reshape(-1)[1:], t, epilogue=epi, Rr=8) == U   # misaligned B
            assert call(x, P, Am, M, K, lB, t[1:], epilogue=epi, Rr=8) == U               # misaligned t
            assert call(x, P, Am, M, K, lB, t, 16, epilogue=epi, Rr=8) == U               # blocksize 16
        assert v(x, P, Am, M, 1008, lB, t, 16, epilogue=epi, Rr=8) == U and "not available" in hipabi.last_error()  # K % 32 != 0
        assert m(x, P, Am, M, 992, lB, t, epilogue=epi, Rr=8) == U and "not covered" in hipabi.last_error()
        assert gemm_lora(x, P, Am, M, K, lB, t, out=out, expect_ok=False, B=65, epilogue=epi, Rr=8) == U
    for call in (v, m):
        assert call(x, P, Am, M, K, lB, t, epilogue=7, Rr=8) == I and "unknown epilogue" in hipabi.last_error()
        assert call(x, P, Am, M - 1, K, lB, t, epilogue=GATED, Rr=8) == I and "even row count" in hipabi.last_error()
    torch.cuda.synchronize()
    assert untouched(buf)


def test_repeated_calls_and_graph_replays_give_identical_bits():
    M, K, Rr = 1026, 4096, 16
    P, Am = weight(M, K)
    for dtype in DT16:
        A, lB, scale = adapter(M, K, Rr, dtype, 1)
        x, r = rand(K, dtype, 2), rand(M, dtype, 3)
        t, out = torch.empty(1, Rr, device=dev()), torch.empty(M, dtype=dtype, device=dev())
        step = lambda: (down(x, A, scale, t), gemv_lora(x, P, Am, M, K, lB, t, residual=r, out=out))
        step()
        eager = out.clone()
        step()
        assert torch.equal(out, eager)
        x8 = rand((8, K), dtype, 4)
        y8 = gemm_lora(x8, P, Am, M, K, lB, down(x8, A, scale))
        assert torch.equal(y8, gemm_lora(x8, P, Am, M, K, lB, down(x8, A, scale)))
        # the pair captured in one graph (neither allocates nor synchronises) and replayed
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
            side.synchronize()
            with torch.cuda.graph(g, stream=side):
                step()
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(3):
            out.zero_()
            t.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)


# ---- torch ops -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16, ids=str)
def test_torch_ops_equal_the_c_abi_bit_for_bit(dtype):
    import torch_bnb_fp4 as pkg

    M, K, Rr = 258, 2048, 24
    P, Am = weight(M, K)
    Bt = P.reshape(-1, 1).t()
    A, lB, scale = adapter(M, K, Rr, dtype, 1)
    b = rand(M, dtype, M, 0.1)
    for rows in (1, 5, 40):
        x = rand((rows, K), dtype, rows, 2.0)
        t = pkg.ext.lora_down(x, A, scale)
        assert t.dtype == torch.float32 and t.shape == (rows, Rr) and torch.equal(t, down(x, A, scale))
        for epi in (NONE, GATED):
            r = rand((rows, M // 2 if epi == GATED else M), dtype, 9)
            if rows == 1:
                got = pkg.ext.gemv_nf4_lora(x, Bt, Am, BS, [M, K], b, r, epi, lB, t)
                assert torch.equal(got, gemv_lora(x.reshape(-1), P, Am, M, K, lB, t, BS, b, r.reshape(-1), epi).reshape(1, -1))
            got = pkg.ext.gemm_nf4_lora(x, Bt, Am, BS, [M, K], b, r, epi, lB, t)
            assert torch.equal(got, gemm_lora(x, P, Am, M, K, lB, t, BS, b, r, epi)) and got.shape == (rows, M // 2 if epi == GATED else M)
    with pytest.raises(RuntimeError, match="not available"):
        pkg.ext.gemv_nf4_lora(x[:1].contiguous(), Bt, Am, BS, [M, K], None, None, NONE, lB[:, :12].contiguous(), t[:1, :12].contiguous())
    with pytest.raises(RuntimeError, match="not covered"):
        pkg.ext.lora_down(rand((65, K), dtype, 1), A, scale)


# ---- the layer and the surgery ---------------------------------------------------------------------------------------------------------
def _nf4_linear(M, K, dtype, seed, bias=False):
    import torch_bnb_fp4 as pkg

    torch.manual_seed(seed)
    root = nn.Sequential(nn.Linear(K, M, bias=bias).to(dtype))
    return pkg.recursively_replace_with_fp4_linear(root, as_dtype=dtype, device=dev(), quant_type="nf4")[0]


def _layer_products(layer, xs):
    qd = layer.quant_data
    return device_products(qd.A.reshape(-1), qd.absmax, int(qd.M), int(qd.N), qd.blocksize, list(xs))


@pytest.mark.parametrize("dtype", DT16, ids=str)
def test_layer_and_gate_up_against_the_oracle(dtype):
    import torch_bnb_fp4 as pkg

    K, M, r = 512, 384, 16
    lin, gate, up = (_nf4_linear(M, K, dtype, s) for s in (1, 2, 3))
    A, lB, _ = adapter(M, K, r, dtype, 1)
    layer = pkg.LoRANF4Linear.from_linear(lin, A, lB, S)
    (Ag, Bg, _), (Au, Bu, _) = adapter(M, K, r, dtype, 5), adapter(M, K, 12, dtype, 7)
    gu = pkg.LoRANF4Linear.gate_up(gate, up, (Ag, Bg, S), (Au, Bu, 0.5))
    rows_layer = pkg.LoRANF4Linear(gu.quant_data, NONE, gu.lora_A, gu.lora_B, gu.lora_scale)  # the same weight and adapter, rows as they are
    xs = rand((40, K), dtype, 9)
    res = rand((40, M), dtype, 10)
    exact, s1 = _layer_products(lin, xs)
    d, s2 = adapter_terms(xs, A, lB, torch.full((r,), S, device=dev()))
    eg, sg = _layer_products(gate, xs)
    eu, su = _layer_products(up, xs)
    dg, s2g = adapter_terms(xs, Ag, Bg, torch.full((r,), S, device=dev()))
    du, s2u = adapter_terms(xs, Au, Bu, torch.full((12,), 0.5, device=dev()))
    for rows in (1, 8, 40):
        x = xs[:rows].contiguous()
        y = layer(x)
        assert y.shape == (rows, M)
        check(y, exact[:rows] + d[:rows], s1[:rows], s2[:rows], dtype, ("layer", rows, dtype))
        assert torch.equal(layer(x, res[:rows].contiguous()), y + res[:rows])
        # gate|up: the interleaved rows against the oracle, then the gated layer against torch's silu * up of those rows
        yr = rows_layer(x)
        check(yr[:, 0::2], eg[:rows] + dg[:rows], sg[:rows], s2g[:rows], dtype, ("gate rows", rows, dtype))
        check(yr[:, 1::2], eu[:rows] + du[:rows], su[:rows], s2u[:rows], dtype, ("up rows", rows, dtype))
        assert_close_ulp(gu(x), torch.nn.functional.silu(yr[:, 0::2]) * yr[:, 1::2], 0.998, ("gate_up", rows, dtype))
    assert layer._fused_ok and layer._small_ok and layer._lora_ok and gu._fused_ok and gu._small_ok
    # 65+ rows: the adapter in torch on the parent's base.  That base is dequant + GEMM: the weights are rounded to T before the
    # product, which the exact-weight oracle does not do, so two checks.  Against the oracle, the fallback bar plus the weight
    # rounding's worst case (still a tenth of the adapter term: ulp/2 * s1 is about 0.035 in bf16 where |delta| is about 0.4).
    # That first check is a sanity bound only - alone it would pass an adapter term that is off by several percent.  The check that
    # holds the adapter is the second, and the two stay together: against the parent's own output for the base, where only the
    # adapter and the one rounding are left, at the fused ops' bar without its base term.
    x70 = rand((70, K), dtype, 11)
    e70, s70 = _layer_products(lin, x70)
    d70, s270 = adapter_terms(x70, A, lB, torch.full((r,), S, device=dev()))
    y70 = layer(x70)
    check(y70, e70 + d70, s70, s270, dtype, ("layer, 70 rows, oracle", dtype), base=e70, weights_rounded=True)
    base70 = pkg.FusedNF4Linear.from_linear(lin)(x70).double()
    check(y70, base70 + d70, torch.zeros_like(s70), s270, dtype, ("layer, 70 rows, on the parent's base", dtype))


def test_rank_4_through_the_layer_equals_rank_8_padded_by_hand():
    import torch_bnb_fp4 as pkg

    dtype, K, M = torch.bfloat16, 512, 384
    lin = _nf4_linear(M, K, dtype, 1)
    A, lB, scale = adapter(M, K, 4, dtype, 1)
    layer = pkg.LoRANF4Linear.from_linear(lin, A, lB, S)
    A8 = torch.cat([A, torch.zeros_like(A)], 0)
    B8 = torch.cat([lB, torch.zeros_like(lB)], 1).contiguous()
    s8 = torch.cat([scale, torch.zeros_like(scale)])
    qd = lin.quant_data
    P, Am = qd.A.reshape(-1), qd.absmax
    for rows in (1, 8):
        x = rand((rows, K), dtype, rows)
        t = down(x, A8, s8)
        want = gemv_lora(x.reshape(-1), P, Am, M, K, B8, t).reshape(1, M) if rows == 1 else gemm_lora(x, P, Am, M, K, B8, t)
        assert torch.equal(layer(x), want)


def test_shape_outside_the_coverage_takes_the_fallback():
    import torch_bnb_fp4 as pkg

    dtype, M, K, bs, r = torch.bfloat16, 64, 1008, 16, 8
    P, Am = weight(M, K, bs)
    A, lB, scale = adapter(M, K, r, dtype, 1)
    layer = pkg.LoRANF4Linear.from_fused(pkg.FusedNF4Linear.from_packed(P.reshape(-1, 1), Am, (M, K), bs, dtype=dtype), A, lB, S)
    x = rand((1, K), dtype, 2)
    y = layer(x)
    assert not layer._fused_ok and y.shape == (1, M)
    exact, s1 = device_products(P, Am, M, K, bs, [x])
    d, s2 = adapter_terms(x, A, lB, scale)
    check(y, exact + d, s1, s2, dtype, "K = 1008 fallback", base=exact)
    assert torch.equal(layer(x), y)


class _Attn(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.q_proj, self.o_proj = nn.Linear(H, H, bias=False), nn.Linear(H, H, bias=False)

    def forward(self, h):
        return self.o_proj(self.q_proj(h))


class _MLP(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = nn.Linear(H, I, bias=False), nn.Linear(H, I, bias=False), nn.Linear(I, H, bias=False)
        self.act_fn = nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class _Block(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.self_attn, self.mlp = _Attn(H), _MLP(H, I)

    def forward(self, h):
        h = h + self.self_attn(h)
        return h + self.mlp(h)


class _Toy(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.model = nn.Module()
        self.model.layers = nn.ModuleList([_Block(H, I), _Block(H, I)])

    def forward(self, h):
        for blk in self.model.layers:
            h = blk(h)
        return h


def _toy_and_adapter(H, I, r, dtype):
    import torch_bnb_fp4 as pkg

    torch.manual_seed(3)
    toy = pkg.recursively_replace_with_fp4_linear(_Toy(H, I).to(dtype), as_dtype=dtype, device=dev(), quant_type="nf4")
    g = torch.Generator().manual_seed(4)
    state = {}
    for i in range(2):
        for name, (M, K) in (("self_attn.q_proj", (H, H)), ("self_attn.o_proj", (H, H)), ("mlp.gate_proj", (I, H)), ("mlp.up_proj", (I, H)),
                             ("mlp.down_proj", (H, I))):
            state[f"base_model.model.model.layers.{i}.{name}.lora_A.weight"] = torch.randn(r, K, generator=g) / math.sqrt(K)
            state[f"base_model.model.model.layers.{i}.{name}.lora_B.weight"] = torch.randn(M, r, generator=g) * 0.05
    return toy, state


def _dense_reference(toy_dense, state, s, h):
    """The toy decoder in float64 with W + s B A merged into dense copies of the quantised weights."""
    def lin(i, name, x):
        layer = toy_dense[(i, name)]
        A = state[f"base_model.model.model.layers.{i}.{name}.lora_A.weight"].to(dev()).to(h.dtype).double()
        B = state[f"base_model.model.model.layers.{i}.{name}.lora_B.weight"].to(dev()).to(h.dtype).double()
        return x @ (layer + s * B @ A).t()
    h = h.double()
    for i in range(2):
        h = h + lin(i, "self_attn.o_proj", lin(i, "self_attn.q_proj", h))
        h = h + lin(i, "mlp.down_proj", torch.nn.functional.silu(lin(i, "mlp.gate_proj", h)) * lin(i, "mlp.up_proj", h))
    return h


def test_attach_lora_and_load_lora_adapter_on_a_toy_decoder(tmp_path):
    import torch_bnb_fp4 as pkg
    from oracle import torch_cpu
    from safetensors.torch import save_file

    H, I, r, alpha, dtype = 512, 768, 4, 8, torch.bfloat16
    toy, state = _toy_and_adapter(H, I, r, dtype)
    code = torch.from_numpy(R.CODE.copy()).to(dev())
    dense = {}
    for i, blk in enumerate(toy.model.layers):
        for name in ("self_attn.q_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"):
            qd = blk.get_submodule(name).quant_data
            dense[(i, name)] = torch_cpu.dequantize(qd.A.reshape(-1), qd.absmax, int(qd.M), int(qd.N), qd.blocksize, torch.float32, code).double()
    assert pkg.fuse_gated_mlps(toy, nf4=True) == 2
    assert pkg.attach_lora(toy, state, r=r, lora_alpha=alpha) == 8
    blk = toy.model.layers[0]
    assert type(blk.self_attn.q_proj) is pkg.LoRANF4Linear and type(blk.mlp.gate_up) is pkg.LoRANF4Linear and blk.mlp.gate_up.rank == 2 * r
    for rows in (1, 8):
        h = rand((rows, H), dtype, rows, 0.5)
        got = toy(h)
        want = _dense_reference(dense, state, alpha / r, h)
        rel = float((got.double() - want).abs().max() / want.abs().max())
        print(f"toy decoder with adapters, {rows} rows: max |err| / max |want| = {rel:.4f}")
        assert got.shape == (rows, H) and rel <= 2e-2  # two blocks of bf16 roundings; a missing adapter is >= 0.1
        base_only = _dense_reference(dense, {k: torch.zeros_like(v) for k, v in state.items()}, 0.0, h)
        assert float((want - base_only).abs().max() / want.abs().max()) >= 0.1
    # the same adapter from a directory in peft's layout gives the same model, bit for bit
    save_file(state, str(tmp_path / "adapter_model.safetensors"))
    (tmp_path / "adapter_config.json").write_text(json.dumps({"r": r, "lora_alpha": alpha, "peft_type": "LORA", "lora_dropout": 0.1,
                                                               "target_modules": ["q_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]}))
    toy2, _ = _toy_and_adapter(H, I, r, dtype)
    pkg.fuse_gated_mlps(toy2, nf4=True)
    assert pkg.load_lora_adapter(toy2, str(tmp_path)) == 8
    h = rand((1, H), dtype, 5, 0.5)
    assert torch.equal(toy2(h), toy(h))
    with pytest.raises(KeyError, match="no such module"):
        pkg.attach_lora(toy2, {"base_model.model.model.layers.5.self_attn.q_proj.lora_A.weight": torch.zeros(r, H),
                               "base_model.model.model.layers.5.self_attn.q_proj.lora_B.weight": torch.zeros(H, r)}, r, alpha)
