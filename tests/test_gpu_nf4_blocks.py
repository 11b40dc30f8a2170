"""The NF4 product for block sizes 128..4096 (fp4_hip_gemm_blocks_nf4, csrc/gemm_blocks_nf4.hip): 1..64 rows, one scale application per block.
Reference: the float64 product of the numpy restatement's dequantised weight (nf4_ref.dequantize_f32).  Bar: the NF4 matrix-core kernels',
|y - y*| <= 1.01 half_ulp(T) |y*| + 1e-5 sum |x_k w_rk| + 1e-30.  absmax is rand * 0.05 + 0.005, or powers of two 8x apart between neighbours:
a scale taken from the wrong block misses the bar by a wide margin."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nf4_ref as R
from gpu_util import HALF_ULP, dev, to_dev
from test_gpu_nf4_fused import rand as randn
from test_gpu_nf4_small_batch import cancellation_pairs

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
GATED = hipabi.EPILOGUE_SILU_MUL_PAIRS
SENTINEL = 0x7BCD  # a finite bit pattern in both 16-bit formats that no test output equals by accident
KBS = [(128, 128), (384, 128), (256, 128), (2304, 128), (768, 256), (1024, 512), (4096, 4096), (2048, 1024)]


def call(x, packed, absmax, out, B, M, K, bs, bias=None, residual=None, epilogue=0, dtype=None):
    f = R.lib().fp4_hip_gemm_blocks_nf4
    f.argtypes, f.restype = [ctypes.c_void_p] * 6 + [ctypes.c_int64] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p], ctypes.c_int
    return f(*map(hipabi._ptr, (x, packed, absmax, bias, residual, out)), B, M, K, bs, hipabi.DT[dtype or x.dtype], epilogue, hipabi._stream())


def blocks(x, packed, absmax, M, K, bs, bias=None, residual=None, epilogue=0, out=None):
    B = x.numel() // K
    out = torch.empty(B, M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device) if out is None else out
    rc = call(x, to_dev(packed), to_dev(absmax), out, B, M, K, bs, bias, residual, epilogue)
    assert rc == hipabi.OK, (rc, hipabi.last_error())
    return out


def weight(M, K, bs, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, M * K // 2, dtype=np.uint8), (rng.random(M * K // bs) * 0.05 + 0.005).astype(np.float32)


def exact_of(x, packed, absmax, M, K, bs, bias=None):
    """numpy float64 (x @ W^T + bias, |x| @ |W|^T) of a [B, K] device activation: the restatement."""
    w = R.dequantize_f32(packed, absmax, bs, M * K).astype(np.float64).reshape(M, K)
    x64 = x.double().cpu().numpy().reshape(-1, K)
    return x64 @ w.T + (0.0 if bias is None else bias.detach().double().cpu().numpy()), np.abs(x64) @ np.abs(w).T


def bar(exact, scale, dtype):
    return 1.01 * HALF_ULP[dtype] * np.abs(exact) + 1e-5 * scale + 1e-30


def gated_ref(e, s, dtype):
    """want = silu(g*) u* of the float64 sums and its tolerance as tests/test_gpu_nf4_fused.py's end-to-end case scales it: g, u, silu and the
    product each carry half an ulp, |d silu / dg| <= 1.1, and the bar's 1e-5 S is carried through the product."""
    g, u, Sg, Su = e[:, 0::2], e[:, 1::2], s[:, 0::2], s[:, 1::2]
    sil = g / (1.0 + np.exp(-g))
    return sil * u, HALF_ULP[dtype] * 1.02 * (3 * np.abs(sil * u) + 1.1 * np.abs(g * u)) + 1e-5 * (1.1 * np.abs(u) * Sg + np.abs(sil) * Su) + 1e-6


def within(y, exact, tol, what):
    ratio = np.abs(y.double().cpu().numpy().reshape(np.shape(exact)) - exact) / tol
    print(f"{what}: worst |err| / tol = {ratio.max():.3f}")
    assert ratio.max() <= 1.0, (what, int((ratio > 1).sum()), float(ratio.max()))


def parity_at_the_bar(dtype):
    """Units of one block (K = 128 * odd), two, one; slices of a block across waves and passes; M and B below, off and on the tiles; bias."""
    for (K, bs), M in itertools.product(KBS, (1, 17, 37, 64)):
        packed, absmax = weight(M, K, bs, K + M)
        x, bias = randn((64, K), dtype, K), randn(M, dtype, M, 0.1)
        for b in (None, bias):
            exact, scale = exact_of(x, packed, absmax, M, K, bs, b)
            for B in (1, 2, 16, 17, 33, 50, 64):
                within(blocks(x[:B], packed, absmax, M, K, bs, b), exact[:B], bar(exact[:B], scale[:B], dtype), (K, bs, M, B, b is not None))


def both_workgroup_shapes_on_the_same_input(dtype):
    for K, bs in ((2304, 128), (1024, 512)):
        packed, absmax = weight(100, K, bs, 99)
        x = randn((64, K), dtype, 5)
        exact, scale = exact_of(x, packed, absmax, 100, K, bs)
        try:
            for variant, B in itertools.product((1, 2), (17, 64)):
                hipabi.set_variant("gemm_blocks_nf4", variant)
                within(blocks(x[:B], packed, absmax, 100, K, bs), exact[:B], bar(exact[:B], scale[:B], dtype), (variant, K, B))
        finally:
            hipabi.set_variant("gemm_blocks_nf4", -1)


def every_scale_in_its_place(dtype):
    """One-hot rows around every block boundary: each output is ONE product, and neighbouring scales differ 8x or 32x (> 2^7 half-ulps)."""
    for K, bs in ((512, 128), (1024, 256), (2048, 1024)):
        M = 20
        packed = np.random.default_rng(K).integers(0, 256, M * K // 2, dtype=np.uint8)
        absmax = (2.0 ** ((np.arange(M * K // bs) * 3) % 8 - 4)).astype(np.float32)
        ks = sorted({0, 63, 64, 127, 128, bs - 1, bs, bs + 1, K - bs, K - 1})
        x = np.zeros((len(ks), K), np.float32)
        x[np.arange(len(ks)), ks] = [1.0, -1.5, 0.75, 3.0, -0.5, 2.0, -1.25, 1.0, -1.5, 0.75][:len(ks)]
        x_t = torch.from_numpy(x).to(dtype).to(dev())
        exact, scale = exact_of(x_t, packed, absmax, M, K, bs)
        assert np.array_equal(np.abs(exact), scale)  # single products
        within(blocks(x_t, packed, absmax, M, K, bs), exact, bar(exact, scale, dtype), (K, bs))


def epilogues(dtype):
    """Residual: out = T(t + r) with t = T(sum + bias) within the bar of y*, so |out - (y* + r)| <= bar + 1.01 half_ulp (|y* + r| + bar): t's own
    error, then one rounding of a sum that may be off by it.  With `residual` aliasing `out`: the same bits.  gate|up: gated_ref."""
    M, h = 38, HALF_ULP[dtype]
    bias, res, res_h = randn(M, dtype, 3, 0.1), randn((64, M), dtype, 13), randn((64, M // 2), dtype, 17)
    for (K, bs), B in itertools.product(((384, 128), (1024, 512)), (2, 17, 64)):
        packed, absmax = weight(M, K, bs, 7)
        x = randn((64, K), dtype, 11)
        exact, S = exact_of(x, packed, absmax, M, K, bs, bias)
        e, r, rh = exact[:B], res[:B].contiguous(), res_h[:B].contiguous()
        b0, er = bar(e, S[:B], dtype), e + r.double().cpu().numpy()
        got = blocks(x[:B], packed, absmax, M, K, bs, bias, r)
        within(got, er, b0 + 1.01 * h * (np.abs(er) + b0), (K, B, "residual"))
        alias = r.clone()
        assert torch.equal(blocks(x[:B], packed, absmax, M, K, bs, bias, alias, out=alias), got)
        want, tol = gated_ref(e, S[:B], dtype)
        within(blocks(x[:B], packed, absmax, M, K, bs, bias, None, GATED), want, tol, (K, B, "gate|up"))
        wr = want + rh.double().cpu().numpy()
        within(blocks(x[:B], packed, absmax, M, K, bs, bias, rh, GATED), wr, tol + 1.01 * h * (np.abs(wr) + tol), (K, B, "gate|up + residual"))


def cancellation_rows_need_both_halves_of_every_code(dtype):
    """test_gpu_nf4_small_batch.py's rows at blocksize 128: the exact sum nearly cancels, so a table without lo (or a flushed fp16 lo) misses."""
    K, bs, B = 384, 128, 64
    pairs, code, failed = cancellation_pairs(dtype), R.CODE.astype(np.float64), []
    for i0, first in itertools.product(range(0, len(pairs), 16), (0, 48)):  # the first and the last column tile
        chunk = (pairs[i0:i0 + 16] + pairs[:16])[:16]
        packed = np.repeat(np.array([(n << 4) | m for n, m, _ in chunk], np.uint8), K // 2)
        x = np.full((B, K), 0.5, np.float32)
        for i, (_, _, xm) in enumerate(chunk):
            x[first + i, 0::2], x[first + i, 1::2] = 1.0, xm
        y = blocks(torch.from_numpy(x).to(dtype).to(dev()), packed, np.ones(16 * K // bs, np.float32), 16, K, bs).double().cpu().numpy()
        for i, (n, m, xm) in enumerate(chunk):
            exact, scale = (K // 2) * (code[n] + code[m] * xm), (K // 2) * (abs(code[n]) + abs(code[m] * xm))
            if abs(y[first + i, i] - exact) > bar(exact, scale, dtype):
                failed.append((n, m))
    assert not failed, (dtype, len(failed), failed[:5])


def refusals_leave_out_untouched(dtype):
    M, K = 32, 1024
    (p_d, a_d), x = (to_dev(a) for a in weight(M, K, 64, 5)), randn((66, K), dtype, 1)
    out = torch.full((65 * M,), SENTINEL, dtype=torch.int16, device=dev())
    for kw in (dict(bs=64), dict(bs=96, K=960), dict(bs=8192), dict(K=192), dict(B=65), dict(dtype=torch.float32), dict(x=x.view(-1)[1:])):
        a = dict(dict(x=x, B=20, K=K, bs=128, dtype=dtype), **kw)
        assert call(a["x"], p_d, a_d, out.view(dtype), a["B"], M, a["K"], a["bs"], dtype=a["dtype"]) == hipabi.ERR_UNSUPPORTED, kw
        assert "fp4_hip_gemm_blocks_nf4" in hipabi.last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


def _layers(bs, K=384, M=96):
    import torch_bnb_fp4 as P

    torch.manual_seed(bs)
    mk = lambda: P.TorchFP4Linear(P.LinearNF4(K, M, bias=True, blocksize=bs).to(dev()))
    return P, nn.ModuleList([mk(), P.fused.FusedNF4Linear.gate_up(mk(), mk())])


def through_the_layers_and_a_captured_graph(dtype):
    P, model = _layers(128)
    plain, gated = model
    calls = lambda: sum(P.ext.qlinear_gemm_stats().values())  # what both routes of dequant + GEMM have served
    layer_exact = lambda qd, x: exact_of(x, qd.A.cpu().numpy().ravel(), qd.absmax.cpu().numpy(), qd.M, qd.N, qd.blocksize, qd.bias)
    xs = [randn((rows, 384), dtype, rows) for rows in (2, 17, 64)]
    assert P.set_small_batch_fused(model, True, nf4_blocks=True) == 2 and plain.quant_data.blocks_batch_fused_nf4
    before = calls()
    for x in xs:
        y, yg = plain(x), gated(x)  # the first call casts the bias to the compute dtype: the reference reads it afterwards
        e, s = layer_exact(plain.quant_data, x)
        within(y, e, bar(e, s, dtype), ("layer", len(x)))
        within(yg, *gated_ref(*layer_exact(gated.quant_data, x), dtype), ("gate|up layer", len(x)))
    with pytest.raises(RuntimeError, match="not covered"):  # a refusal by the library, as the layers' fallback expects it
        P.ext.gemm_nf4_blocks(xs[0].float(), plain.quant_data.A.t(), plain.quant_data.absmax, 128, [96, 384], None, None, 0)
    # one captured step at 8 rows replays bit-identically to eager
    x8, stream = randn((8, 384), dtype, 21), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        plain(x8)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y8 = plain(x8)
    for i in range(3):
        x8.copy_(randn((8, 384), dtype, 30 + i))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y8, plain(x8)), i
    assert calls() == before  # neither route of dequant + GEMM has served a call so far
    # the new switch off, the two older ones on: a blocksize-128 weight is back on dequant + GEMM
    assert P.set_small_batch_fused(model, False, nf4_blocks=True) == 2 and P.set_small_batch_fused(model, True, nf4=True, nf4_wide=True) == 1
    for x in xs:
        plain(x), gated(x)
    assert calls() == before + 2 * len(xs)
    # a blocksize-64 layer with only the new switch set: dequant + GEMM
    P, model64 = _layers(64)
    P.set_small_batch_fused(model64, True, nf4_blocks=True)
    model64[0](xs[1])
    assert calls() == before + 2 * len(xs) + 1


CHECKS = [parity_at_the_bar, both_workgroup_shapes_on_the_same_input, every_scale_in_its_place, epilogues,
          cancellation_rows_need_both_halves_of_every_code, refusals_leave_out_untouched, through_the_layers_and_a_captured_graph]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_blocks_kernel_from_the_c_abi_to_the_layers(dtype):
    """One item per dtype (about a second): each check prints its worst |err| / tol and names the case it fails on."""
    for check in CHECKS:
        check(dtype)
