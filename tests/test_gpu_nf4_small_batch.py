"""The fused NF4 small-batch product (fp4_hip_gemm_small_nf4, csrc/gemm_small_nf4.hip): 1..16 activation rows on the matrix cores.

Checker and bar are the NF4 GEMV's (tests/test_gpu_nf4_gemv.py): y* = the float64 product of the exact f32 weights
code[nibble] * absmax (+ bias), formed on the device by the pure-torch oracle and tied to the numpy restatement
(nf4_ref.gemv_exact) on sampled rows;  |y - y*| <= 1.01 * ulp_T(y*)/2 + 1e-5 * sum |x_k w_rk|, no element outside it.

The NF4 codes are exact in neither bf16 nor fp16, so the kernel feeds every weight to the matrix cores as hi = T(code) and
lo = T(code - hi).  Random data hides a build that drops lo in fp16 (its typical error stays below the half-ulp term), so
test_cancellation_rows_need_both_halves_of_every_code constructs rows whose exact sum nearly cancels: there the code's
representation error is all that is left, and a hi-only table misses the bar by up to 237x (bf16) / 29x (fp16)."""
import ctypes

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st
from torch import nn

import hipabi
import nf4_ref as R
from gpu_util import HALF_ULP, dev, to_dev
from test_gpu_nf4_gemv import check_bar, device_products, tie_to_restatement

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
BS = 64
SENTINEL = 0x7BCD  # a finite bit pattern in both 16-bit formats that no test output equals by accident
COMMON = dict(deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)


def _lib():
    l = R.lib()
    if not getattr(l, "_nf4_small_bound", False):
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        l.fp4_hip_gemm_small_nf4.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]
        l.fp4_hip_gemm_small_nf4.restype = i32
        l._nf4_small_bound = True
    return l


def call(x, packed, absmax, out, B, M, K, bs=BS, bias=None, dtype=None):
    return _lib().fp4_hip_gemm_small_nf4(hipabi._ptr(x), hipabi._ptr(packed), hipabi._ptr(absmax), hipabi._ptr(bias), hipabi._ptr(out), B, M, K,
                                         bs, hipabi.DT[dtype or x.dtype], hipabi._stream())


def gemm(x, packed, absmax, M, K, bias=None):
    B = x.numel() // K
    out = torch.empty(B, M, dtype=x.dtype, device=x.device)
    rc = call(x, packed, absmax, out, B, M, K, bias=bias)
    assert rc == hipabi.OK, (rc, hipabi.last_error())
    return out


def bits_t(t):
    return t.contiguous().view(torch.int16)


def _random_nf4(n_elems, seed):
    g = torch.Generator(device=dev()).manual_seed(seed)
    packed = torch.randint(0, 256, (n_elems // 2,), dtype=torch.uint8, device=dev(), generator=g)
    absmax = torch.rand(n_elems // BS, device=dev(), generator=g) * 0.05 + 0.005
    return packed, absmax


def _host_exact(x, packed, absmax, M, K):
    """numpy float64 (x @ W^T, |x| @ |W|^T) for a [B, K] activation: the restatement itself, for the small constructed cases."""
    w = R.dequantize_f32(packed, absmax, BS, M * K).astype(np.float64).reshape(M, K)
    x64 = x.double().cpu().numpy().reshape(-1, K)
    with np.errstate(invalid="ignore", over="ignore"):
        return x64 @ w.T, np.abs(x64) @ np.abs(w).T


def _within_bar(y, exact, scale, dtype, what, mask=None):
    tol = 1.01 * HALF_ULP[dtype] * np.abs(exact) + 1e-5 * scale + 1e-30
    err = np.abs(y.double().cpu().numpy().reshape(exact.shape) - exact)
    bad = err > tol
    if mask is not None:
        bad &= mask
    assert not bad.any(), (what, dtype, int(bad.sum()), float(np.nanmax(np.where(bad, err / tol, 0.0))))


# ---- 1. parity at the bar ------------------------------------------------------------------------------------------------------------
SHAPES = [(4096, 4096), (1024, 4096), (33, 512), (7, 1024), (257, 1536), (300, 8192), (40, 14336), (66, 2560), (16, 32768)]
ROWS = [1, 2, 3, 4, 5, 8, 9, 13, 16]


@pytest.mark.parametrize("M,K", SHAPES, ids=[f"{m}x{k}" for m, k in SHAPES])
def test_parity_at_the_bar_every_row_count_and_split(M, K):
    """K / 512 = 1, 2, 3, 5, 8, 16, 28, 64: every blocks-per-wave split of the dispatcher (1, 2, 4), one and many passes, M below
    and off the 16-row tile; 1..16 rows crossing the x-image sizes (<= 4, <= 8, direct); with and without the bias."""
    packed_d, absmax_d = _random_nf4(M * K, 31 * M + K)
    g = torch.Generator().manual_seed(K + M)
    x32 = torch.randn(16, K, generator=g)
    b32 = torch.randn(M, generator=g) * 0.1
    for dtype in DTYPES:
        x = x32.to(dtype).to(dev())
        bias = b32.to(dtype).to(dev())
        exact_d, scale_d = device_products(packed_d, absmax_d, M, K, BS, list(x))
        tie_to_restatement(packed_d, absmax_d, M, K, BS, [x[0]], exact_d[:1], np.random.default_rng(M), n_rows=2)
        with_bias = exact_d + bias.double()
        for B in ROWS:
            y = gemm(x[:B].contiguous(), packed_d, absmax_d, M, K)
            check_bar(y, exact_d[:B].reshape(-1), scale_d[:B].reshape(-1), dtype, (M, K, B, "plain"))
            yb = gemm(x[:B].contiguous(), packed_d, absmax_d, M, K, bias=bias)
            check_bar(yb, with_bias[:B].reshape(-1), scale_d[:B].reshape(-1), dtype, (M, K, B, "bias"))


# ---- 2. the split matters --------------------------------------------------------------------------------------------------------------
def cancellation_pairs(dtype):
    """Every ordered pair of non-zero codes (n, m), n != m, with x_m = T(-code[n] / code[m]) and |x_m| <= 4."""
    code = R.CODE.astype(np.float64)
    pairs = []
    for n in range(16):
        for m in range(16):
            if n == m or n == 7 or m == 7:
                continue
            xm = float(torch.tensor(-code[n] / code[m], dtype=torch.float64).to(torch.float32).to(dtype).double())
            if abs(xm) <= 4:
                pairs.append((n, m, xm))
    return pairs


@pytest.mark.parametrize("dtype", DTYPES)
def test_cancellation_rows_need_both_halves_of_every_code(dtype):
    """One weight row of K = 512 per pair: even elements nibble n, odd elements nibble m, absmax 1; activations +1 on even k and x_m
    on odd k.  y* = 256 (code[n] + code[m] x_m) nearly cancels, scale = 256 (|code[n]| + |code[m] x_m|) does not.  16 pairs per
    launch (weight row i and activation row i belong to pair i; only the diagonal is checked).  With hi + lo the code term reaches
    at most 0.44 (bf16) / 0.01 (fp16) of the tolerance; with T(code) alone 181 / 167 of the 185 pairs fail."""
    K = 512
    pairs = cancellation_pairs(dtype)
    assert len(pairs) == 185
    code = R.CODE.astype(np.float64)
    absmax = torch.ones(16 * K // BS, device=dev())
    worst, failed = 0.0, []
    for i0 in range(0, len(pairs), 16):
        chunk = pairs[i0:i0 + 16]
        chunk = chunk + [chunk[0]] * (16 - len(chunk))
        packed = np.repeat(np.array([(n << 4) | m for n, m, _ in chunk], np.uint8), K // 2)
        x = np.ones((16, K), np.float32)
        for i, (_, _, xm) in enumerate(chunk):
            x[i, 1::2] = xm
        x_t = torch.from_numpy(x).to(dtype).to(dev())
        assert torch.equal(x_t.float().cpu(), torch.from_numpy(x))  # every activation is exact in T
        y = gemm(x_t, to_dev(packed), absmax, 16, K).double().cpu().numpy()
        for i, (n, m, xm) in enumerate(chunk):
            exact = 256.0 * (code[n] + code[m] * xm)
            scale = 256.0 * (abs(code[n]) + abs(code[m] * xm))
            tol = 1.01 * HALF_ULP[dtype] * abs(exact) + 1e-5 * scale + 1e-30
            ratio = abs(y[i, i] - exact) / tol
            worst = max(worst, ratio)
            if ratio > 1:
                failed.append((n, m, ratio))
    print(f"cancellation rows {dtype}: worst |err| / tol = {worst:.3f}, {len(failed)} of {len(pairs)} pairs outside the bar")
    assert not failed, (dtype, len(failed), max(f[2] for f in failed), failed[:5])


# ---- 3. every code in the right place ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [512, 1024, 2048])
def test_every_code_reaches_the_matrix_cores_in_the_right_place(dtype, K):
    """Row r < 16 is all nibble r; rows 16.. repeat one byte whose two nibbles differ (0x0F, 0xF0, 0x7E, 0x1C).  One-hot
    activations at the first and last k, around the 64-weight block and the 512-weight wave boundary, even and odd k: the output is
    T(code[nibble(r, k)] * x_k) - a swapped nibble, a k order that differs between the A and the B side or a wrong table entry shows."""
    row_bytes = [n * 17 for n in range(16)] + [0x0F, 0xF0, 0x7E, 0x1C]
    M = len(row_bytes)
    packed = np.repeat(np.array(row_bytes, np.uint8), K // 2)
    absmax = np.ones(M * K // BS, np.float32)
    ks = sorted({0, 1, 2, 7, 8, 15, 16, 63, 64, 65, 127, 128, 511 % K, 512 % K, K - 2, K - 1})
    vals = [1.0, -1.5, 0.75, 3.0]
    for B in (16, 8, 4):  # the direct, the <= 8-row and the <= 4-row x paths (the images only where K / 512 is a multiple of 4)
        for k0 in range(0, len(ks), B):
            sel = ks[k0:k0 + B]
            x = np.zeros((len(sel), K), np.float32)
            for b, k in enumerate(sel):
                x[b, k] = vals[(b + k) % 4]
            x_t = torch.from_numpy(x).to(dtype).to(dev())
            y = gemm(x_t, to_dev(packed), to_dev(absmax), M, K)
            exact, scale = _host_exact(x_t, packed, absmax, M, K)
            want = np.array([[R.CODE[(row_bytes[r] >> 4) if k % 2 == 0 else (row_bytes[r] & 15)].astype(np.float64) * x[b, k]
                              for r in range(M)] for b, k in enumerate(sel)])
            assert np.array_equal(exact, want)  # the restatement agrees with the sentence above
            _within_bar(y, exact, scale, dtype, (K, B, sel))


# ---- 4. scales -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_scales_powers_of_two_zero_and_inf(dtype):
    M, K, B = 20, 2048, 5
    rng = np.random.default_rng(11)
    packed = rng.integers(0, 256, M * K // 2, dtype=np.uint8)
    x_t = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)).to(dtype).to(dev())
    nb = M * K // BS
    absmax = (2.0 ** ((np.arange(nb) * 7) % 31 - 20)).astype(np.float32)  # 2^-20 .. 2^10 within every row (32 blocks per row)
    assert absmax.min() == 2.0**-20 and absmax.max() == 2.0**10
    y = gemm(x_t, to_dev(packed), to_dev(absmax), M, K)
    exact, scale = _host_exact(x_t, packed, absmax, M, K)
    _within_bar(y, exact, scale, dtype, "powers of two")
    zeroed = absmax.copy()
    zeroed[::3] = 0.0
    zeroed[K // BS * 4: K // BS * 5] = 0.0  # all of row 4
    y = gemm(x_t, to_dev(packed), to_dev(zeroed), M, K)
    exact, scale = _host_exact(x_t, packed, zeroed, M, K)
    _within_bar(y, exact, scale, dtype, "zero scales")
    assert (y[:, 4] == 0).all()
    one_inf = absmax.copy()
    one_inf[K // BS * 5 + 3] = np.inf  # one block of row 5
    y = gemm(x_t, to_dev(packed), to_dev(one_inf), M, K)
    assert not torch.isfinite(y[:, 5]).any()
    others = np.ones((B, M), bool)
    others[:, 5] = False
    exact, scale = _host_exact(x_t, packed, absmax, M, K)
    _within_bar(y, exact, scale, dtype, "inf scale: the other rows", mask=others)
    assert torch.isfinite(y[:, [r for r in range(M) if r != 5]]).all()


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,M,K", [(3, 33, 512), (7, 7, 1024), (16, 257, 2048), (2, 1, 4096)])
def test_guards_offset_views_and_determinism(dtype, B, M, K):
    """Nothing is stored past row B or weight row M (sentinel guard regions around out); x, packed, absmax and bias as views at
    16-byte-aligned non-zero offsets inside larger buffers; two runs are bit-identical."""
    G = 4096
    g = torch.Generator(device=dev()).manual_seed(B * M + K)
    big_x = torch.randn(8 + B * K + 8, device=dev(), generator=g).to(dtype)
    big_p = torch.randint(0, 256, (16 + M * K // 2 + 16,), dtype=torch.uint8, device=dev(), generator=g)
    big_a = torch.rand(4 + M * K // BS + 4, device=dev(), generator=g) * 0.05 + 0.005
    big_b = (torch.randn(8 + M + 8, device=dev(), generator=g) * 0.1).to(dtype)
    x, packed, absmax, bias = big_x[8:8 + B * K], big_p[16:16 + M * K // 2], big_a[4:4 + M * K // BS], big_b[8:8 + M]
    assert all(t.data_ptr() % 16 == 0 and t.data_ptr() != s.data_ptr() for t, s in ((x, big_x), (packed, big_p), (bias, big_b)))
    buf = torch.full((G + B * M + G,), SENTINEL, dtype=torch.int16, device=dev())
    out = buf[G:G + B * M].view(dtype)
    assert call(x, packed, absmax, out, B, M, K, bias=bias) == hipabi.OK, hipabi.last_error()
    assert (buf[:G] == SENTINEL).all() and (buf[G + B * M:] == SENTINEL).all()
    first = out.clone()
    exact, scale = _host_exact(x.view(B, K), packed.cpu().numpy(), absmax.cpu().numpy(), M, K)
    _within_bar(first, exact + bias.double().cpu().numpy(), scale, dtype, (B, M, K))
    out.view(torch.int16).fill_(SENTINEL)
    assert call(x, packed, absmax, out, B, M, K, bias=bias) == hipabi.OK
    assert torch.equal(bits_t(out), bits_t(first))
    # the same operands from fresh, unshifted allocations: the same bits
    again = gemm(x.clone().view(B, K), packed.clone(), absmax.clone(), M, K, bias=bias.clone())
    assert torch.equal(bits_t(again).reshape(-1), bits_t(first))


def test_empty_and_refused_calls_leave_out_untouched():
    M, K = 32, 1152  # big enough for every shape asked for below
    packed, absmax = _random_nf4(M * K, 5)
    bad = [dict(K=576), dict(bs=128), dict(dtype=torch.float32), dict(B=17), dict(K=1024 + 64), dict(K=256)]
    for dtype in DTYPES:
        x = torch.randn(17, K, device=dev()).to(dtype)
        out = torch.full((17 * M,), SENTINEL, dtype=torch.int16, device=dev())
        for kw in ({"M": 0}, {"B": 0}):
            a = dict(B=2, M=M, K=1024)
            a.update(kw)
            assert call(x, packed, absmax, out.view(dtype), a["B"], a["M"], a["K"]) == hipabi.OK
        for kw in bad:
            a = dict(B=2, M=M, K=1024, bs=BS, dtype=dtype)
            a.update(kw)
            rc = call(x, packed, absmax, out.view(dtype), a["B"], a["M"], a["K"], bs=a["bs"], dtype=a["dtype"])
            assert rc == hipabi.ERR_UNSUPPORTED, (kw, rc)
            assert "gemm_small_nf4" in hipabi.last_error()
        # operands off the 16-byte alignment the kernel's loads need: refused, not misread
        assert call(x.view(-1)[1:], packed, absmax, out.view(dtype), 2, M, 1024) == hipabi.ERR_UNSUPPORTED
        assert call(x, packed[1:], absmax, out.view(dtype), 2, M, 1024) == hipabi.ERR_UNSUPPORTED
        assert call(x, packed, absmax, out.view(dtype), -1, M, 1024) == hipabi.ERR_INVALID
        assert call(None, packed, absmax, out.view(dtype), 2, M, 1024, dtype=dtype) == hipabi.ERR_INVALID
        torch.cuda.synchronize()
        assert (out == SENTINEL).all()


# ---- 6. torch op and module ------------------------------------------------------------------------------------------------------------
def _pkg():
    import torch_bnb_fp4 as pkg

    return pkg


@pytest.mark.parametrize("dtype", DTYPES)
def test_torch_op_equals_the_c_abi_bit_for_bit(dtype):
    P = _pkg()
    M, K = 300, 2048
    packed, absmax = _random_nf4(M * K, 77)
    g = torch.Generator(device=dev()).manual_seed(3)
    bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
    for shape in [(2, K), (16, K), (2, 4, K), (1, K), (K,)]:
        x = torch.randn(*shape, device=dev(), generator=g).to(dtype)
        for b in (None, bias):
            y = P.ext.gemm_small_nf4(x, packed.view(-1, 1).t(), absmax, BS, [M, K], b)
            assert tuple(y.shape) == tuple(shape[:-1]) + (M,) and y.dtype == dtype
            assert torch.equal(bits_t(y).reshape(-1), bits_t(gemm(x, packed, absmax, M, K, bias=b)).reshape(-1)), (shape, b is None)
    with pytest.raises(RuntimeError):
        P.ext.gemm_small_nf4(torch.randn(17, K, device=dev()).to(dtype), packed.view(-1, 1).t(), absmax, BS, [M, K], None)
    with pytest.raises(RuntimeError):
        P.ext.gemm_small_nf4(torch.randn(2, K, device=dev()), packed.view(-1, 1).t(), absmax, BS, [M, K], None)  # f32
    with pytest.raises(RuntimeError):
        P.ext.gemm_small_nf4(torch.randn(2, 576, device=dev()).to(dtype), packed.view(-1, 1).t(), absmax, BS, [64, 576], None)


def _nf4_layer(K, M, seed=0, bias=True):
    P = _pkg()
    torch.manual_seed(seed)
    return P.TorchFP4Linear(P.LinearNF4(K, M, bias=bias).to(dev()))


def _restated(layer, x):
    qd = layer.quant_data
    exact, scale = _host_exact(x, qd.A.cpu().numpy().ravel(), qd.absmax.cpu().numpy(), qd.M, qd.N)
    if layer.bias is not None:
        exact = exact + layer.bias.detach().double().cpu().numpy()
    return exact, scale


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_switch_routes_2_to_16_rows_and_nothing_else(dtype):
    P = _pkg()
    root = nn.Sequential(_nf4_layer(1024, 512, seed=1))
    layer = root[0]
    assert P.set_small_batch_fused(root, True) == 0 and not layer.quant_data.small_batch_fused_nf4
    g = torch.Generator(device=dev()).manual_seed(9)
    xs = {rows: torch.randn(rows, 1024, device=dev(), generator=g).to(dtype) for rows in (1, 2, 8, 16, 17, 200)}
    xs["3d"] = torch.randn(2, 4, 1024, device=dev(), generator=g).to(dtype)
    off = {k: layer(x) for k, x in xs.items()}
    assert P.set_small_batch_fused(root, True, nf4=True) == 1 and layer.quant_data.small_batch_fused_nf4
    for k, x in xs.items():
        y = layer(x)
        if k in (1, 17, 200):
            assert torch.equal(bits_t(y), bits_t(off[k])), k
            continue
        exact, scale = _restated(layer, x)
        _within_bar(y, exact, scale, dtype, ("module", k))
        # through the switch the layer is exactly the op on its own operands
        qd = layer.quant_data
        assert torch.equal(bits_t(y), bits_t(P.ext.gemm_small_nf4(x, qd.A.t(), qd.absmax, 64, [512, 1024], qd.bias)))
        assert tuple(y.shape) == tuple(x.shape[:-1]) + (512,)
    assert P.set_small_batch_fused(root, False, nf4=True) == 1 and not layer.quant_data.small_batch_fused_nf4
    assert torch.equal(bits_t(layer(xs[8])), bits_t(off[8]))
    # K % 512 != 0: the switch changes nothing
    odd = _nf4_layer(576, 128, seed=4)
    x = torch.randn(4, 576, device=dev(), generator=g).to(dtype)
    y_off = odd(x)
    odd.quant_data.small_batch_fused_nf4 = True
    assert torch.equal(bits_t(odd(x)), bits_t(y_off))


# ---- 7. graph capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_capture_replays_bit_identical_to_eager(dtype):
    P = _pkg()
    M, K, B = 1024, 4096, 8
    packed, absmax = _random_nf4(M * K, 13)
    g = torch.Generator(device=dev()).manual_seed(21)
    bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
    x = torch.randn(B, K, device=dev(), generator=g).to(dtype)
    Bt = packed.view(-1, 1).t()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        P.ext.gemm_small_nf4(x, Bt, absmax, BS, [M, K], bias)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = P.ext.gemm_small_nf4(x, Bt, absmax, BS, [M, K], bias)
    for i in range(3):
        x.copy_(torch.randn(B, K, device=dev(), generator=g).to(dtype))
        graph.replay()
        torch.cuda.synchronize()
        eager = P.ext.gemm_small_nf4(x, Bt, absmax, BS, [M, K], bias)
        assert torch.equal(bits_t(y), bits_t(eager)), i


# ---- 8. hypothesis ---------------------------------------------------------------------------------------------------------------------
_POOL = {}


def _pool():
    if not _POOL:
        _POOL["w"] = _random_nf4(3000 * 512 * 40, 1234)
        g = torch.Generator(device=dev()).manual_seed(4321)
        _POOL["x"] = torch.randn(16, 512 * 40 + 64, device=dev(), generator=g)
        _POOL["b"] = torch.randn(3000, device=dev(), generator=g) * 0.1
    return _POOL


@settings(max_examples=100, **COMMON)
@given(B=st.integers(1, 16), M=st.integers(1, 3000), u=st.integers(1, 40), dtype=st.sampled_from(DTYPES), with_bias=st.booleans(),
       shift=st.integers(0, 63))
def test_hypothesis_draws(B, M, u, dtype, with_bias, shift):
    """Element e of the flat weight is code[nib(e)] * absmax[e // 64] whatever (M, K) is: every draw reads a window of one pool."""
    K = 512 * u
    pool = _pool()
    off = shift * 512  # whole quant blocks, 16-byte aligned
    packed, absmax = pool["w"][0][off // 2:], pool["w"][1][off // BS:]
    if packed.numel() < M * K // 2:
        packed, absmax = pool["w"]
    x = pool["x"][:B, shift:shift + K].to(dtype).contiguous()
    bias = pool["b"][:M].to(dtype) if with_bias else None
    exact_d, scale_d = device_products(packed, absmax, M, K, BS, list(x))
    if with_bias:
        exact_d = exact_d + bias.double()
    y = gemm(x, packed, absmax, M, K, bias=bias)
    check_bar(y, exact_d.reshape(-1), scale_d.reshape(-1), dtype, (B, M, K, with_bias))


# ---- 9. the single-round rule of the x image -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 16], ids=["16cus", "16cus+16"])
def test_the_8_row_x_image_switches_off_past_one_round_of_workgroups(extra):
    """dispatch_nf4_mfma_shape stages x for 5..8 rows only while the grid is a single round (B <= 8 && blocks <= cus): M = 16 cus is
    the last shape with the image, 16 cus + 16 the first without, and no other small-batch shape here is taller than 4096.  5 and 8
    rows, both dtypes, through fp4_hip_gemm_small_nf4 and through fp4_hip_gemm_fused_nf4: the plain result at this file's bar against
    the restatement (and the same bits from both entry points); the gate|up epilogue within 1 ulp of torch's silu(g) * u on that
    result, >= 99.8 % identical (the batched rule of tests/test_gpu_nf4_fused.py)."""
    l = _lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    l.fp4_hip_gemm_fused_nf4.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp]
    l.fp4_hip_gemm_fused_nf4.restype = i32
    M, K = 16 * torch.cuda.get_device_properties(dev()).multi_processor_count + extra, 2048
    packed_d, absmax_d = _random_nf4(M * K, 31 * M + K)
    g = torch.Generator().manual_seed(K + M)
    x32 = torch.randn(8, K, generator=g)
    b32 = torch.randn(M, generator=g) * 0.1
    for dtype in DTYPES:
        x, bias = x32.to(dtype).to(dev()), b32.to(dtype).to(dev())
        exact_d, scale_d = device_products(packed_d, absmax_d, M, K, BS, list(x))
        tie_to_restatement(packed_d, absmax_d, M, K, BS, [x[0], x[7]], exact_d[[0, 7]], np.random.default_rng(M), n_rows=14)
        with_bias = exact_d + bias.double()
        for B in (5, 8):
            xb = x[:B].contiguous()
            y = gemm(xb, packed_d, absmax_d, M, K)
            check_bar(y, exact_d[:B].reshape(-1), scale_d[:B].reshape(-1), dtype, (M, K, B, "plain"))
            yb = gemm(xb, packed_d, absmax_d, M, K, bias=bias)
            check_bar(yb, with_bias[:B].reshape(-1), scale_d[:B].reshape(-1), dtype, (M, K, B, "bias"))
            outs = {}
            for epi in (hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS):
                out = torch.empty(B, M // 2 if epi else M, dtype=dtype, device=dev())
                rc = l.fp4_hip_gemm_fused_nf4(hipabi._ptr(xb), hipabi._ptr(packed_d), hipabi._ptr(absmax_d), hipabi._ptr(bias), None,
                                              hipabi._ptr(out), B, M, K, BS, hipabi.DT[dtype], epi, hipabi._stream())
                assert rc == hipabi.OK, (rc, hipabi.last_error())
                outs[epi] = out
            assert torch.equal(bits_t(outs[hipabi.EPILOGUE_NONE]), bits_t(yb))
            ref = torch.nn.functional.silu(yb[:, 0::2]) * yb[:, 1::2]
            line = lambda t: torch.where((bits_t(t).int() & 0xFFFF) >= 0x8000, 0x8000 - (bits_t(t).int() & 0xFFFF), bits_t(t).int() & 0xFFFF)
            d = (line(outs[hipabi.EPILOGUE_SILU_MUL_PAIRS]) - line(ref)).abs()
            assert int(d.max()) <= 1 and float((d == 0).float().mean()) >= 0.998, (M, B, dtype, int(d.max()))
