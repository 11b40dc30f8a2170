"""The dense GEMM behind the batch > 1 path (`qlinear*` = dequant + GEMM, reference csrc/torch_fp4.cpp:64-103): called on hipBLASLt directly with
cached plans (csrc/torch_ext.cpp, lt_linear) instead of through at::linear, whose ~18 us of host time per call made an eager small-batch
FP4 layer slower than the dense layer it replaces.  Same maths, so: both routes against the float64 product of the dequantised weight (rounded
to the activation dtype first, as the reference's dequant does), against each other, for every dtype / bias / rank / odd size, under HIP-graph
capture (first call of a process arriving under capture included), with activations and bias past 16-byte alignment, and the host-side
saving itself.  The NF4 ops (qlinear_nf4[_bias]) run the same GEMM after the NF4 dequant and are held to the same bars."""
import time

import numpy as np
import pytest
import torch

import nf4_ref as R
from gpu_util import case, dev
from oracle import fp4_oracle as o
from qlinear_constructed import routed

pytestmark = pytest.mark.gpu
BS = 64
COUNTER = {"hipblaslt": "direct", "aten": "aten"}  # set_qlinear_gemm's name of a route -> its counter in qlinear_gemm_stats()
TOL = {torch.float32: (2e-5, 2e-5), torch.float16: (2e-3, 2e-3), torch.bfloat16: (1.6e-2, 1.6e-2)}


def pkg():
    import torch_bnb_fp4

    return torch_bnb_fp4


@pytest.fixture(autouse=True)
def _default_route():
    yield
    pkg().ext.set_qlinear_gemm("hipblaslt")


def _want(c, x_t, bias_t, dtype, table):
    """float64 x @ W_T^T + b with W_T = the dequantised weight rounded to the activation dtype (what both routes multiply)."""
    w = o.dequantize(c.packed, c.am, BS, c.M * c.K, {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}[dtype], table)
    if dtype == torch.float32:
        w64 = w.astype(np.float64)
    elif dtype == torch.float16:
        w64 = w.view(np.float16).astype(np.float64)
    else:
        w64 = o.bf16_bits_to_f32(w).astype(np.float64)
    want = x_t.double().cpu().numpy().reshape(-1, c.K) @ w64.reshape(c.M, c.K).T
    if bias_t is not None:
        want = want + bias_t.double().cpu().numpy()
    return want


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,K,shape", [(2048, 768, (2, 768)), (64, 2048, (6, 2048)), (4096, 4096, (3, 5, 4096)), (300, 1000, (7, 1000)),
                                      (1024, 4096, (300, 4096))])
def test_both_gemm_routes_against_float64(dtype, M, K, shape):
    P = pkg()
    c = case(M, K, seed=5)
    g = torch.Generator(device=dev()).manual_seed(M + K)
    x = torch.randn(*shape, device=dev(), generator=g).to(dtype)
    bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
    code = P.ext.code_table("codebook").to(dev())
    A = c.P.view(-1, 1)
    rtol, atol = TOL[dtype]
    for table, ops in (("codebook", (lambda: P.ext.qlinear_codebook(x, A, c.A, code, M, K, BS), lambda: P.ext.qlinear_codebook_bias(x, A, c.A, code, M, K, BS, bias))),
                       ("tree", (lambda: P.ext.qlinear(x, A, c.A, M, K, BS), lambda: P.ext.qlinear_bias(x, A, c.A, M, K, BS, bias)))):
        for op, b in zip(ops, (None, bias)):
            want = _want(c, x, b, dtype, table)
            scale = np.abs(want).max()
            outs = {}
            for route in ("hipblaslt", "aten"):
                P.ext.set_qlinear_gemm(route)
                with routed(P.ext, COUNTER[route], calls=1):  # the route named is the route that ran
                    y = op()
                assert y.shape == (*shape[:-1], M) and y.dtype == dtype
                outs[route] = y.double().cpu().numpy().reshape(-1, M)
                err = np.abs(outs[route] - want).max()
                assert err <= rtol * scale + atol, (route, table, b is not None, err, scale)
            assert np.abs(outs["hipblaslt"] - outs["aten"]).max() <= rtol * scale + atol


def _round_weight(w32, dtype):
    """f32 weight values -> float64 values of their RNE rounding to dtype (what the dequant writes and both routes multiply)."""
    return torch.from_numpy(np.ascontiguousarray(w32)).to(dtype).double().numpy()


def _want_nf4(c, x_t, bias_t, dtype):
    """float64 x @ W_T^T + b, W_T = the NF4 reading of the case's bytes and scales (code[nibble] * absmax) rounded to dtype."""
    w64 = _round_weight(R.dequantize_f32(c.packed, c.am, BS, c.M * c.K), dtype).reshape(c.M, c.K)
    want = x_t.double().cpu().numpy().reshape(-1, c.K) @ w64.T
    if bias_t is not None:
        want = want + bias_t.double().cpu().numpy()
    return want


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,K,shape", [(2048, 768, (2, 768)), (64, 2048, (6, 2048)), (4096, 4096, (3, 5, 4096)), (300, 1000, (7, 1000)),
                                      (1024, 4096, (300, 4096))])
def test_nf4_both_gemm_routes_against_float64(dtype, M, K, shape):
    """qlinear_nf4[_bias] = NF4 dequant (KEEP_CACHED) + the same GEMM: every NF4 call with more than one token, prefill included.
    The case's packed bytes read as NF4 (any byte is a valid pair of codes) with its positive scales."""
    P = pkg()
    c = case(M, K, seed=5)
    g = torch.Generator(device=dev()).manual_seed(M + K + 1)
    x = torch.randn(*shape, device=dev(), generator=g).to(dtype)
    bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
    A = c.P.view(-1, 1)
    rtol, atol = TOL[dtype]
    for op, b in ((lambda: P.ext.qlinear_nf4(x, A, c.A, M, K, BS), None), (lambda: P.ext.qlinear_nf4_bias(x, A, c.A, M, K, BS, bias), bias)):
        want = _want_nf4(c, x, b, dtype)
        scale = np.abs(want).max()
        outs = {}
        for route in ("hipblaslt", "aten"):
            P.ext.set_qlinear_gemm(route)
            with routed(P.ext, COUNTER[route], calls=1):
                y = op()
            assert y.shape == (*shape[:-1], M) and y.dtype == dtype
            outs[route] = y.double().cpu().numpy().reshape(-1, M)
            err = np.abs(outs[route] - want).max()
            assert err <= rtol * scale + atol, (route, b is not None, err, scale)
        assert np.abs(outs["hipblaslt"] - outs["aten"]).max() <= rtol * scale + atol


def test_nf4_graph_capture_and_replay_of_the_direct_gemm():
    """qlinear_nf4 / qlinear_nf4_bias captured (one shape planned during capture) and replayed: bit-identical to eager."""
    P = pkg()
    M, K = 768, 1536
    c = case(M, K, seed=3)
    A = c.P.view(-1, 1)
    x = torch.randn(5, K, device=dev()).to(torch.bfloat16)
    bias = torch.randn(M, device=dev()).to(torch.bfloat16)
    P.ext.qlinear_nf4(torch.randn(2, K, device=dev()).to(torch.bfloat16), A, c.A, M, K, BS)  # the device's handle exists before capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            y = P.ext.qlinear_nf4_bias(x, A, c.A, M, K, BS, bias)
            y0 = P.ext.qlinear_nf4(x, A, c.A, M, K, BS)
        torch.cuda.synchronize()
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        got, got0 = y.clone(), y0.clone()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(got, P.ext.qlinear_nf4_bias(x, A, c.A, M, K, BS, bias))
    assert torch.equal(got0, P.ext.qlinear_nf4(x, A, c.A, M, K, BS))
    want = _want_nf4(c, x, bias, torch.bfloat16)
    assert np.abs(got.double().cpu().numpy() - want).max() <= TOL[torch.bfloat16][0] * np.abs(want).max() + TOL[torch.bfloat16][1]


def _past_alignment(t, byte_off):
    """A contiguous copy of ``t`` whose data pointer lies ``byte_off`` bytes past a 16-byte boundary (a view at an element offset into
    a larger buffer, with room behind it)."""
    k = byte_off // t.element_size()
    buf = torch.zeros(t.numel() + 32, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == byte_off
    return v


@pytest.mark.parametrize("fmt", ["fp4", "nf4"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_activations_and_bias_past_16_byte_alignment(fmt, dtype):
    """Contiguous activations and a bias whose data pointers are 2, 4 or 8 bytes past 16-byte alignment (views at an element offset):
    the plan cache key has no alignment field, so the direct route must still be right there - and so must at::linear."""
    P = pkg()
    rtol, atol = TOL[dtype]
    for M, K, shape in ((2048, 768, (2, 768)), (300, 1000, (7, 1000)), (1024, 4096, (300, 4096))):
        c = case(M, K, seed=5)
        A = c.P.view(-1, 1)
        g = torch.Generator(device=dev()).manual_seed(M + K + 2)
        x = torch.randn(*shape, device=dev(), generator=g).to(dtype)
        bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
        if fmt == "fp4":
            ops = (lambda xx, bb: P.ext.qlinear(xx, A, c.A, M, K, BS)), (lambda xx, bb: P.ext.qlinear_bias(xx, A, c.A, M, K, BS, bb))
            wants = _want(c, x, None, dtype, "tree"), _want(c, x, bias, dtype, "tree")
        else:
            ops = (lambda xx, bb: P.ext.qlinear_nf4(xx, A, c.A, M, K, BS)), (lambda xx, bb: P.ext.qlinear_nf4_bias(xx, A, c.A, M, K, BS, bb))
            wants = _want_nf4(c, x, None, dtype), _want_nf4(c, x, bias, dtype)
        for off in (2, 4, 8):
            if off % x.element_size():
                continue
            for moved in ("x", "bias", "both"):
                xo = _past_alignment(x, off) if moved in ("x", "both") else x
                bo = _past_alignment(bias, off) if moved in ("bias", "both") else bias
                for route in ("hipblaslt", "aten"):
                    P.ext.set_qlinear_gemm(route)
                    for op, want, with_bias in zip(ops, wants, (False, True)):
                        if moved == "bias" and not with_bias:
                            continue
                        y = op(xo, bo)
                        torch.cuda.synchronize()
                        assert y.shape == (*shape[:-1], M)
                        err = np.abs(y.double().cpu().numpy().reshape(-1, M) - want).max()
                        scale = np.abs(want).max()
                        assert err <= rtol * scale + atol, (M, K, off, moved, route, with_bias, err, scale)


def test_non_contiguous_activations_and_foreign_bias_dtype_still_work():
    P = pkg()
    M, K = 512, 1024
    c = case(M, K, seed=9)
    A = c.P.view(-1, 1)
    x = torch.randn(K, 4, device=dev()).to(torch.bfloat16).t()  # [4, K], not contiguous
    assert not x.is_contiguous()
    y = P.ext.qlinear(x, A, c.A, M, K, BS)
    P.ext.set_qlinear_gemm("aten")
    assert torch.allclose(y.float(), P.ext.qlinear(x, A, c.A, M, K, BS).float(), rtol=2e-2, atol=2e-2)
    P.ext.set_qlinear_gemm("hipblaslt")
    # a bias of another dtype is not the library path's business: at::linear decides (and raises, like the reference's F.linear would)
    with pytest.raises(RuntimeError):
        P.ext.qlinear_bias(x.contiguous(), A, c.A, M, K, BS, torch.zeros(M, device=dev(), dtype=torch.float32))
    with pytest.raises(RuntimeError):
        P.ext.set_qlinear_gemm("cublas")


def test_graph_capture_and_replay_of_the_direct_gemm():
    """A shape never seen before is planned (heuristic query, host only) during capture; replays reproduce the eager result bit for bit."""
    P = pkg()
    M, K = 768, 1536
    c = case(M, K, seed=2)
    A = c.P.view(-1, 1)
    x = torch.randn(5, K, device=dev()).to(torch.float16)
    bias = torch.randn(M, device=dev()).to(torch.float16)
    P.ext.qlinear(torch.randn(2, K, device=dev()).to(torch.float16), A, c.A, M, K, BS)  # the device's handle exists before capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            y = P.ext.qlinear_bias(x, A, c.A, M, K, BS, bias)
        torch.cuda.synchronize()
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        got = y.clone()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(got, P.ext.qlinear_bias(x, A, c.A, M, K, BS, bias))


def test_the_direct_gemm_saves_host_time_in_the_layer_call():
    """What the change is for: the eager batch-2 call of an FP4 layer (dequant + GEMM) next to a dense nn.Linear of the same shape.
    The at::linear route costs a dense call plus the dequant op (measured 29.6 us against 21.5 dense on the round-5 box); the direct route
    must come out below the dense call (18.7 us there) and well below the at::linear route."""
    P = pkg()
    lin = torch.nn.Linear(2048, 2048).to(dev()).to(torch.bfloat16)
    fp4 = P.recursively_replace_with_fp4_linear(torch.nn.Linear(2048, 2048).to(torch.bfloat16), as_dtype=torch.bfloat16, device=dev())
    x = torch.randn(2, 2048, device=dev(), dtype=torch.bfloat16)

    def us(fn, n=1500):
        for _ in range(200):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    with torch.inference_mode():
        dense = us(lambda: lin(x))
        direct = us(lambda: fp4(x))
        P.ext.set_qlinear_gemm("aten")
        aten = us(lambda: fp4(x))
    assert direct < dense and direct < 0.8 * aten, (dense, direct, aten)
