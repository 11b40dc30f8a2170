"""The dequant + GEMM path (`qlinear*`: every call with more than one token that no fused kernel takes) on constructed operands whose
result is known BIT FOR BIT (tests/qlinear_constructed.py, proved on the CPU by tests/test_qlinear_constructed_host.py), on both GEMM
routes - hipBLASLt through the cached plan ('direct') and at::linear ('aten') - with the route that ran ASSERTED through the
extension's counters (qlinear_gemm_stats); a per-element bar on the direct route's accumulation; and the two things at::linear means
beyond a product, which the direct route must step aside for: autograd (gradient to the activation and to a bias) and autocast.

Comparisons are of bit patterns, the sign of an exact zero aside (see qlinear_constructed)."""
import threading
import time

import numpy as np
import pytest
import torch

import qlinear_constructed as Q
from gpu_util import assert_within_bar, bits as tbits, case, dev

pytestmark = pytest.mark.gpu
BS = Q.BS
TD = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
OPS = ["tree", "codebook", "nf4", "nested"]  # qlinear[_bias], qlinear_codebook[_bias], qlinear_nf4[_bias], qlinear_nf4_nested
ROUTES = (("hipblaslt", "direct"), ("aten", "aten"))
OP_SHAPES = [(op, M, K) for op in OPS for (M, K) in (Q.NESTED_SHAPES if op == "nested" else Q.WEIGHT_SHAPES)]
_CACHE = {}


def pkg():
    import torch_bnb_fp4

    return torch_bnb_fp4


@pytest.fixture(autouse=True)
def _default_route():
    yield
    pkg().ext.set_qlinear_gemm("hipblaslt")


def fmt_of(op):
    return "nf4" if op == "nested" else op


class Weight:
    """One constructed weight on the device (made once per session; the ops only read it) with the oracle's T values of it."""

    def __init__(self, kind, M, K, fmt):
        self.M, self.K, self.fmt = M, K, fmt
        self.packed, self.am = {"cycle": lambda: (Q.byte_cycle_weight(M, K), Q.flat_scales(M, K)), "zero": lambda: Q.zero_code_weight(M, K, fmt),
                                "sums": lambda: Q.exact_sum_weight(M, K, fmt)}[kind]()
        self.A = torch.from_numpy(self.packed).to(dev()).view(-1, 1)
        self.absmax = torch.from_numpy(self.am).to(dev())
        self._nested = None
        self._wT = {}

    def nested(self):
        if self._nested is None:
            q, nested, code, off = Q.tabled_statistics(self.am)
            self._nested = (torch.from_numpy(q).to(dev()), torch.from_numpy(nested).to(dev()), torch.from_numpy(code).to(dev()), off)
        return self._nested

    def w_T(self, dtype):
        if dtype not in self._wT:
            self._wT[dtype] = Q.weight_T(self.packed, self.am, self.M, self.K, self.fmt, dtype)
        return self._wT[dtype]


def weight(kind, M, K, fmt) -> Weight:
    key = (kind, M, K, fmt)
    if key not in _CACHE:
        _CACHE[key] = Weight(kind, M, K, fmt)
    return _CACHE[key]


def call(op, x, W: Weight, bias=None):
    e, M, K = pkg().ext, W.M, W.K
    if op == "tree":
        return e.qlinear(x, W.A, W.absmax, M, K, BS) if bias is None else e.qlinear_bias(x, W.A, W.absmax, M, K, BS, bias)
    if op == "codebook":
        code = _CACHE.setdefault("code", e.code_table("codebook").to(dev()))
        return e.qlinear_codebook(x, W.A, W.absmax, code, M, K, BS) if bias is None else e.qlinear_codebook_bias(x, W.A, W.absmax, code, M, K, BS, bias)
    if op == "nf4":
        return e.qlinear_nf4(x, W.A, W.absmax, M, K, BS) if bias is None else e.qlinear_nf4_bias(x, W.A, W.absmax, M, K, BS, bias)
    q, nested, code, off = W.nested()
    return e.qlinear_nf4_nested(x, W.A, q, nested, code, off, 256, M, K, BS, bias)


def t_of(values, dtype):
    """float64 T values -> device tensor of T."""
    return torch.from_numpy(np.ascontiguousarray(values, np.float64)).to(TD[dtype]).to(dev())


def got_bits(y):
    y = y.detach()
    return tbits(torch.where(y == 0, torch.zeros_like(y), y))


def same_bits(y, want, dtype, shape, what):
    """y has ``shape`` and dtype T, and the bits of the float64 expectation ``want`` [rows, M] (zeros of either sign alike)."""
    assert tuple(y.shape) == tuple(shape) and y.dtype == TD[dtype], (what, tuple(y.shape), y.dtype)
    g, w = got_bits(y).reshape(-1), Q.bits(want, dtype).reshape(-1)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.size} outputs differ; first at flat index {i} (row {i // want.shape[-1]}, column "
                             f"{i % want.shape[-1]}): got bits {g[i]:#x}, want {w[i]:#x} ({np.asarray(want).reshape(-1)[i]!r})")


def past_alignment(t, byte_off):
    """A contiguous copy of ``t`` whose data pointer lies ``byte_off`` bytes past a 16-byte boundary."""
    k = byte_off // t.element_size()
    buf = torch.zeros(t.numel() + 32, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == byte_off
    return v


def out_shape(shape, M):
    return tuple(shape[:-1]) + (M,)


# ---- 1. one-hot rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", Q.DTYPES)
@pytest.mark.parametrize("op,M,K", OP_SHAPES)
def test_one_hot_rows_on_both_routes(op, M, K, dtype):
    """y[b][r] = T(fl32(W_T[r][k_b] * v)): over the byte cycle every byte value, nibble, block scale and row is told apart."""
    e = pkg().ext
    W = weight("cycle", M, K, fmt_of(op))
    w = W.w_T(dtype)
    for shape in Q.row_shapes(K):
        rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        for p, v in zip(*Q.one_hot_batches(K, rows)):
            x = t_of(Q.one_hot_rows(p, v, K).reshape(shape), dtype)
            want = Q.one_hot_expected(w, p, v, dtype)
            for setting, route in ROUTES:
                e.set_qlinear_gemm(setting)
                with Q.routed(e, route, calls=1):
                    y = call(op, x, W)
                same_bits(y, want, dtype, out_shape(shape, M), (op, M, K, dtype, shape, route))
    for setting, _ in ROUTES:  # no rows: only shape and dtype, and the library is not asked for an empty product
        e.set_qlinear_gemm(setting)
        with Q.routed(e, "aten", calls=1):
            y = call(op, torch.zeros(0, K, dtype=TD[dtype], device=dev()), W)
        assert tuple(y.shape) == (0, M) and y.dtype == TD[dtype]


# ---- 2. bias alone and exact sums ------------------------------------------------------------------------------------------------------
def _placements(x, bias):
    """(label, activation, bias) with either or both 2, 4 and 8 bytes past 16-byte alignment, and the activation as a transposed view."""
    yield "plain", x, bias
    for off in (2, 4, 8):
        if off % x.element_size():
            continue
        for moved in ("x", "bias", "both"):
            if bias is None and moved != "x":
                continue
            yield f"{moved}+{off}", (past_alignment(x, off) if moved != "bias" else x), (past_alignment(bias, off) if moved != "x" else bias)
    if x.dim() == 2:
        xt = x.t().contiguous().t()
        assert not xt.is_contiguous() or x.shape[0] == 1
        yield "transposed view", xt, bias


@pytest.mark.parametrize("dtype", Q.DTYPES)
@pytest.mark.parametrize("op,M,K", OP_SHAPES)
def test_bias_alone_and_exact_sums_on_both_routes(op, M, K, dtype):
    """Over the zero-code weight the output IS the bias (a bias rounded on its own, taken from a neighbouring column or added in fewer
    bits shows); the exact sums have one answer in every summation order, so a block read under its neighbour's scale, a wrong
    nibble or a term dropped shows as a wrong integer."""
    e = pkg().ext
    fmt = fmt_of(op)
    Wz, Ws = weight("zero", M, K, fmt), weight("sums", M, K, fmt)
    bias_z, bias_s = Q.full_precision_bias(M, dtype), Q.exact_sum_bias(M)
    bz, bs_ = t_of(bias_z, dtype), t_of(bias_s, dtype)
    for shape in Q.row_shapes(K):
        rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        xa = t_of(Q.arbitrary_rows(shape, dtype, seed=rows), dtype)
        xs_np = Q.exact_sum_rows(shape)
        xs = t_of(xs_np, dtype)
        cases = [("bias alone", Wz, xa, bz, np.broadcast_to(bias_z, (rows, M))),
                 ("exact sums", Ws, xs, None, Q.product(Ws.w_T(dtype), xs_np)),
                 ("exact sums + bias", Ws, xs, bs_, Q.product(Ws.w_T(dtype), xs_np, bias_s))]
        for name, W, x, b, want in cases:
            for label, xp, bp in _placements(x, b):
                for setting, route in ROUTES:
                    e.set_qlinear_gemm(setting)
                    with Q.routed(e, route, calls=1):
                        y = call(op, xp, W, bp)
                    same_bits(y, want, dtype, out_shape(shape, M), (name, op, M, K, dtype, shape, label, route))


# ---- 3. the bias pointer of a cached, shared descriptor ---------------------------------------------------------------------------------
def _alternate(op, W, x, biases, dtype, out):
    try:
        e = pkg().ext
        for _ in range(3):
            for b_np, b in biases:
                with_bits = call(op, x, W, b)
                same_bits(with_bits, np.broadcast_to(b_np, (x.shape[0], W.M)), dtype, (x.shape[0], W.M), ("alternating biases", op, dtype))
        out.append(dict(e.qlinear_gemm_stats()))
    except BaseException as exc:  # noqa: BLE001 - handed to the test's thread
        out.append(exc)


@pytest.mark.parametrize("dtype", Q.DTYPES)
@pytest.mark.parametrize("op", ["tree", "nf4"])
def test_each_call_uses_its_own_bias_on_one_cached_plan(op, dtype):
    """The bias pointer is a mutable attribute of the plan's descriptor: two biases alternated on ONE (rows, M, K) key, in this thread
    and in a second one (plans are per thread), then a captured graph with bias 1 replayed after an eager call with bias 2."""
    e = pkg().ext
    M, K = Q.WEIGHT_SHAPES[0]
    W = weight("zero", M, K, fmt_of(op))
    b1_np = Q.full_precision_bias(M, dtype)
    b2_np = -2.0 * b1_np[::-1]
    biases = [(b1_np, t_of(b1_np, dtype)), (b2_np, t_of(b2_np, dtype))]
    x = t_of(Q.arbitrary_rows((5, K), dtype, seed=1), dtype)
    before = dict(e.qlinear_gemm_stats())
    for runner in ("this thread", "a second thread"):
        out = []
        if runner == "this thread":
            _alternate(op, W, x, biases, dtype, out)
        else:
            t = threading.Thread(target=_alternate, args=(op, W, x, biases, dtype, out))
            t.start()
            t.join()
        assert len(out) == 1
        if isinstance(out[0], BaseException):
            raise out[0]
    after = dict(e.qlinear_gemm_stats())
    assert after["direct"] - before["direct"] == 12 and after["aten"] == before["aten"]
    # capture with bias 1 (the device's handle exists: the calls above), run eagerly with bias 2 on the same key, replay
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with Q.routed(e, "direct", calls=1):
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                y1 = call(op, x, W, biases[0][1])
        torch.cuda.synchronize()
        with Q.routed(e, "direct", calls=1):
            y2 = call(op, x, W, biases[1][1])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got1, got2 = y1.clone(), y2.clone()
    torch.cuda.current_stream().wait_stream(s)
    same_bits(got1, np.broadcast_to(b1_np, (5, M)), dtype, (5, M), ("replay keeps the captured bias", op, dtype))
    same_bits(got2, np.broadcast_to(b2_np, (5, M)), dtype, (5, M), ("eager call between capture and replay", op, dtype))


# ---- 4. plan cache turnover -------------------------------------------------------------------------------------------------------------
def test_the_plan_cache_empties_itself_and_rebuilds():
    """4100 distinct (rows, M, K) keys in one thread: the map of plans is cleared at 4096 entries (csrc/torch_ext.cpp, lt_plan); exact
    sums before, at and after the turn, and rows 1 and 2 again afterwards on rebuilt plans - all on the direct route."""
    e = pkg().ext
    M, K, dtype, last = 16, 64, "bfloat16", 4100
    W = weight("sums", M, K, "tree")
    x_np, bias_np = Q.exact_sum_rows((last, K)), Q.exact_sum_bias(M)
    x, bias = t_of(x_np, dtype), t_of(bias_np, dtype)
    want = Q.product(W.w_T(dtype), x_np, bias_np)
    assert Q.exact_sum_bound(W.w_T(dtype), x_np, bias_np) < 256
    checked = (1, 2, 4095, 4096, 4097, last)
    t0 = time.perf_counter()
    with Q.routed(e, "direct", calls=last + 2):
        for rows in range(1, last + 1):
            y = call("tree", x[:rows], W, bias)
            if rows in checked:
                same_bits(y, want[:rows], dtype, (rows, M), ("plan cache turnover", rows))
        for rows in (1, 2):
            same_bits(call("tree", x[:rows], W, bias), want[:rows], dtype, (rows, M), ("after the turnover", rows))
    torch.cuda.synchronize()
    print(f"plan cache turnover: {last + 2} calls in {time.perf_counter() - t0:.2f} s")


# ---- 5. accumulation precision of the direct route --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", Q.DTYPES)
@pytest.mark.parametrize("M,K,rows", [(1024, 4096, 7), (300, 1000, 65)])
def test_direct_route_meets_the_gemv_bar_per_element(M, K, rows, dtype):
    """What csrc/torch_ext.cpp claims for the direct route - f32 accumulation, the bias in the epilogue, ONE rounding to T - is the
    project's GEMV bar per element: 1.01 half-ulps of T plus 1e-5 sum |x w| against the float64 product of the T-rounded oracle
    weight (+ bias).  Exact sums cannot show this (they are exact in bf16 too): N(0, 1) activations over a quantised N(0, 0.02)."""
    e = pkg().ext
    c = case(M, K, seed=5)
    x, b, _, _ = c.rows(rows, 11, TD[dtype], bias=True)
    xv, bv = x.double().cpu().numpy(), b.double().cpu().numpy()
    A = c.P.view(-1, 1)
    code = e.code_table("codebook").to(dev())
    ops = {"tree": (lambda: e.qlinear(x, A, c.A, M, K, BS), lambda: e.qlinear_bias(x, A, c.A, M, K, BS, b)),
           "codebook": (lambda: e.qlinear_codebook(x, A, c.A, code, M, K, BS), lambda: e.qlinear_codebook_bias(x, A, c.A, code, M, K, BS, b)),
           "nf4": (lambda: e.qlinear_nf4(x, A, c.A, M, K, BS), lambda: e.qlinear_nf4_bias(x, A, c.A, M, K, BS, b))}
    for fmt, (plain, with_bias) in ops.items():
        w = Q.weight_T(c.packed, c.am, M, K, fmt, dtype)
        scale = np.abs(xv) @ np.abs(w).T
        for op, exact, sc in ((plain, xv @ w.T, scale), (with_bias, xv @ w.T + bv, scale + np.abs(bv))):
            with Q.routed(e, "direct", calls=1):
                y = op()
            err = assert_within_bar(y, exact, sc, TD[dtype])
            tol = {"float32": 0.0, "float16": 2.0**-11, "bfloat16": 2.0**-8}[dtype] * 1.01 * np.abs(exact) + 1e-5 * sc + 1e-30
            print(f"direct route {fmt} {dtype} {M}x{K} x {rows} rows, bias={op is with_bias}: worst error / bar = {float((err / tol).max()):.4f}")


# ---- 6. gradients -----------------------------------------------------------------------------------------------------------------------
def _grad_rows(rows, M, dtype):
    """g [rows, M] with one non-zero v per row at column r_b = (37 b + 5) % M."""
    cols = (37 * np.arange(rows) + 5) % M
    vals = np.array([Q.ONE_HOT_VALUES[b % 4] for b in range(rows)], np.float64)
    g = np.zeros((rows, M))
    g[np.arange(rows), cols] = vals
    return cols, vals, g


@pytest.mark.parametrize("setting", ["hipblaslt", "aten"])
@pytest.mark.parametrize("dtype", Q.DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_gradient_reaches_the_activation_and_the_bias(op, dtype, setting):
    """The reference's batch > 1 path is F.linear over the dequantised weight, not under no_grad: gradient flows to the activation
    and to a bias that requires grad.  x.grad[b] = T(fl32(W_T[r_b] * v)) for a one-hot g; bias.grad = the column sums of g."""
    e = pkg().ext
    e.set_qlinear_gemm(setting)
    fmt = fmt_of(op)
    for M, K, rows in ((320, 192, 5), (300, 1000, 2)):
        if op == "nested" and (M, K) not in Q.NESTED_SHAPES:
            continue
        cols, vals, g_np = _grad_rows(rows, M, dtype)
        g = t_of(g_np, dtype)
        # the byte-cycle weight: every code and scale in the gradient
        W = weight("cycle", M, K, fmt)
        x = t_of(Q.arbitrary_rows((rows, K), dtype, seed=3), dtype).requires_grad_()
        with Q.routed(e, "aten", calls=1):
            y = call(op, x, W)
        assert y.grad_fn is not None and y.requires_grad
        y.backward(g)
        same_bits(x.grad, Q.one_hot_expected(W.w_T(dtype).T, cols, vals, dtype), dtype, (rows, K), ("x.grad", op, M, K, dtype, setting))
        # exact sums with a bias that requires grad: the forward bits, x.grad and bias.grad
        W = weight("sums", M, K, fmt)
        x_np, bias_np = Q.exact_sum_rows((rows, K)), Q.exact_sum_bias(M)
        for x_grad, b_grad in ((True, True), (False, True), (True, False)):
            x, bias = t_of(x_np, dtype).requires_grad_(x_grad), t_of(bias_np, dtype).requires_grad_(b_grad)
            with Q.routed(e, "aten", calls=1):
                y = call(op, x, W, bias)
            assert y.grad_fn is not None
            same_bits(y, Q.product(W.w_T(dtype), x_np, bias_np), dtype, (rows, M), ("forward under autograd", op, M, K, dtype, setting))
            y.backward(g)
            if x_grad:
                same_bits(x.grad, Q.one_hot_expected(W.w_T(dtype).T, cols, vals, dtype), dtype, (rows, K), ("x.grad, exact sums", op, dtype, setting))
            if b_grad:
                same_bits(bias.grad, g_np.sum(axis=0)[None, :], dtype, (M,), ("bias.grad", op, M, K, dtype, setting))
        # inference keeps the GEMM it was given: no_grad, inference_mode and inputs that do not require grad
        route = "direct" if setting == "hipblaslt" else "aten"
        x, bias = t_of(x_np, dtype).requires_grad_(), t_of(bias_np, dtype).requires_grad_()
        want = Q.product(W.w_T(dtype), x_np, bias_np)
        with Q.routed(e, route, calls=3):
            with torch.no_grad():
                y1 = call(op, x, W, bias)
            with torch.inference_mode():
                y2 = call(op, x, W, bias)
            y3 = call(op, x.detach(), W, bias.detach())
        for y in (y1, y2, y3):
            assert y.grad_fn is None and not y.requires_grad
            same_bits(y, want, dtype, (rows, M), ("inference", op, M, K, dtype, setting))


@pytest.mark.parametrize("dtype", Q.DTYPES)
def test_gradient_through_the_modules(dtype):
    """An FP4 layer, an NF4 layer and a resident nested NF4 layer over the SAME weight values (+-1.0 and 0 are codes of both formats)
    with a [4, K] activation that requires grad: one x.grad, bit for bit, and the one the dequantised weight gives."""
    P = pkg()
    M, K = Q.NESTED_SHAPES[0]
    Wf, Wn = weight("sums", M, K, "codebook"), weight("sums", M, K, "nf4")
    assert np.array_equal(Wf.w_T(dtype), Wn.w_T(dtype))
    bias_np = Q.exact_sum_bias(M)
    q, nested, code256, off = Wn.nested()
    layers = {
        "fp4": P.serialization.plain_linear(Wf.A, Wf.absmax, P.ext.code_table("codebook").to(dev()), (M, K), BS, TD[dtype], "fp4", t_of(bias_np, dtype)),
        "nf4": P.serialization.plain_linear(Wn.A, Wn.absmax, P.ext.code_table("nf4").to(dev()), (M, K), BS, TD[dtype], "nf4", t_of(bias_np, dtype)),
        "nested nf4": P.nested.NestedNF4Linear(Wn.A, q, nested, code256, off, (M, K), BS, bias=t_of(bias_np, dtype), dtype=TD[dtype]),
    }
    cols, vals, g_np = _grad_rows(4, M, dtype)
    x_np = Q.exact_sum_rows((4, K))
    want_y, want_g = Q.product(Wf.w_T(dtype), x_np, bias_np), Q.one_hot_expected(Wf.w_T(dtype).T, cols, vals, dtype)
    grads = {}
    for name, layer in layers.items():
        x = t_of(x_np, dtype).requires_grad_()
        with Q.routed(P.ext, "aten", calls=1):
            y = layer(x)
        assert y.grad_fn is not None, name
        same_bits(y, want_y, dtype, (4, M), ("module forward", name, dtype))
        y.backward(t_of(g_np, dtype))
        same_bits(x.grad, want_g, dtype, (4, K), ("module x.grad", name, dtype))
        grads[name] = got_bits(x.grad)
        with Q.routed(P.ext, "direct", calls=1), torch.inference_mode():
            same_bits(layer(t_of(x_np, dtype)), want_y, dtype, (4, M), ("module inference", name, dtype))
    assert np.array_equal(grads["fp4"], grads["nf4"]) and np.array_equal(grads["nf4"], grads["nested nf4"])


# ---- 7. autocast ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low", ["bfloat16", "float16"])
@pytest.mark.parametrize("op", OPS)
def test_autocast_applies_its_cast_policy(op, low):
    """Under torch.autocast an f32 activation gives what at::linear gives there: the lower-precision dtype (the reference's F.linear
    is on autocast's cast list).  Exact sums, so the bits are known in either dtype.  Outside the context: direct and f32 again."""
    e = pkg().ext
    M, K = Q.WEIGHT_SHAPES[0]
    W = weight("sums", M, K, fmt_of(op))
    x_np, bias_np = Q.exact_sum_rows((5, K)), Q.exact_sum_bias(M)
    x, bias = t_of(x_np, "float32"), t_of(bias_np, "float32")
    for b, want in ((None, Q.product(W.w_T("float32"), x_np)), (bias, Q.product(W.w_T("float32"), x_np, bias_np))):
        with torch.autocast("cuda", dtype=TD[low]):
            with Q.routed(e, "aten", calls=2):
                y = call(op, x, W, b)
                e.set_qlinear_gemm("aten")
                y_aten = call(op, x, W, b)
                e.set_qlinear_gemm("hipblaslt")
        assert y.dtype == y_aten.dtype == TD[low] and torch.equal(y, y_aten)
        same_bits(y, want, low, (5, M), ("under autocast", op, low, b is not None))
        with Q.routed(e, "direct", calls=1):
            y = call(op, x, W, b)
        same_bits(y, want, "float32", (5, M), ("outside autocast", op, low, b is not None))
