"""The one-pass NF4 product for up to 128 activation rows (fp4_hip_gemm_wide_nf4, csrc/gemm_wide_nf4.hip).

Checker and bar are the NF4 GEMV's (tests/test_gpu_nf4_gemv.py): y* = the float64 product of the exact f32 weights
code[nibble] * absmax (+ bias), formed on the device by the pure-torch oracle and tied to the numpy restatement
(nf4_ref.gemv_exact) on sampled rows;  |y - y*| <= 1.01 * ulp_T(y*)/2 + 1e-5 * sum |x_k w_rk|, no element outside it.
The (shape, rows) cases are tests/nf4_wide_cases.py's; tests/test_nf4_wide_batch_host.py shows they reach every dispatcher cell."""
import ctypes

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st
from torch import nn

import hipabi
import nf4_ref as R
import nf4_wide_cases as C
from gpu_util import HALF_ULP, dev, to_dev
from test_gpu_nf4_gemv import check_bar, device_products, tie_to_restatement
from test_gpu_nf4_small_batch import cancellation_pairs, gemm as gemm_small

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
BS = 64
SENTINEL = 0x7BCD  # a finite bit pattern in both 16-bit formats that no test output equals by accident
COMMON = dict(deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)


def _lib():
    l = R.lib()
    if not getattr(l, "_nf4_wide_bound", False):
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        l.fp4_hip_gemm_wide_nf4.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]
        l.fp4_hip_gemm_wide_nf4.restype = i32
        l._nf4_wide_bound = True
    return l


def call(x, packed, absmax, out, B, M, K, bs=BS, bias=None, dtype=None):
    return _lib().fp4_hip_gemm_wide_nf4(hipabi._ptr(x), hipabi._ptr(packed), hipabi._ptr(absmax), hipabi._ptr(bias), hipabi._ptr(out), B, M, K,
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
@pytest.mark.parametrize("M,K", C.SHAPES, ids=[f"{m}x{k}" for m, k in C.SHAPES])
def test_parity_at_the_bar_every_tile_count_chunking_and_cell(M, K):
    """17..128 rows across every column-tile count and the two-chunk split; 1, 2, 5, 16 rows where K % 512 != 0 (the one-tile form);
    both workgroup shapes, both blocks-per-wave, ragged last passes, M below and off the tile; with and without the bias."""
    packed_d, absmax_d = _random_nf4(M * K, 31 * M + K)
    g = torch.Generator().manual_seed(K + M)
    x32 = torch.randn(128, K, generator=g)
    b32 = torch.randn(M, generator=g) * 0.1
    for dtype in DTYPES:
        x = x32.to(dtype).to(dev())
        bias = b32.to(dtype).to(dev())
        exact_d, scale_d = device_products(packed_d, absmax_d, M, K, BS, list(x))
        tie_to_restatement(packed_d, absmax_d, M, K, BS, [x[0], x[127]], exact_d[[0, 127]], np.random.default_rng(M), n_rows=2)
        with_bias = exact_d + bias.double()
        for B in C.rows_for(K):
            y = gemm(x[:B].contiguous(), packed_d, absmax_d, M, K)
            check_bar(y, exact_d[:B].reshape(-1), scale_d[:B].reshape(-1), dtype, (M, K, B, "plain"))
            yb = gemm(x[:B].contiguous(), packed_d, absmax_d, M, K, bias=bias)
            check_bar(yb, with_bias[:B].reshape(-1), scale_d[:B].reshape(-1), dtype, (M, K, B, "bias"))


@pytest.mark.parametrize("variant", [1, 2])
def test_both_workgroup_shapes_on_the_same_input(variant):
    """fp4_hip_set_variant("gemm_wide_nf4", 1 / 2) forces 16 / 32 weight rows per workgroup whatever M is; both hold the bar."""
    M, K = 1000, 2304
    packed_d, absmax_d = _random_nf4(M * K, 99)
    try:
        hipabi.set_variant("gemm_wide_nf4", variant)
        for dtype in DTYPES:
            x = torch.randn(128, K, device=dev(), generator=torch.Generator(device=dev()).manual_seed(5)).to(dtype)
            exact_d, scale_d = device_products(packed_d, absmax_d, M, K, BS, list(x))
            for B in (17, 50, 64, 128):
                check_bar(gemm(x[:B].contiguous(), packed_d, absmax_d, M, K), exact_d[:B].reshape(-1), scale_d[:B].reshape(-1), dtype,
                          (variant, B))
    finally:
        hipabi.set_variant("gemm_wide_nf4", -1)


# ---- 2. the split matters --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,first", [(64, 0), (64, 16), (64, 48), (50, 34), (128, 112), (128, 64)])
def test_cancellation_rows_need_both_halves_of_every_code(dtype, B, first):
    """The rows of tests/test_gpu_nf4_small_batch.py's cancellation test, 16 pairs per launch in activation rows first..first + 15 of
    B (the first, a middle and the last column tile, and both chunks of a 128-row call): weight row i and activation row first + i
    belong to pair i, even elements nibble n, odd elements nibble m; the exact sum nearly cancels, so a table without lo (or, in
    fp16, a flushed lo) misses the bar.  K = 576 keeps 16-row calls off the forwarded kernel as well."""
    K = 576
    pairs = cancellation_pairs(dtype)
    assert len(pairs) == 185
    code = R.CODE.astype(np.float64)
    absmax = torch.ones(16 * K // BS, device=dev())
    worst, failed = 0.0, []
    for i0 in range(0, len(pairs), 16):
        chunk = pairs[i0:i0 + 16]
        chunk = chunk + [chunk[0]] * (16 - len(chunk))
        packed = np.repeat(np.array([(n << 4) | m for n, m, _ in chunk], np.uint8), K // 2)
        x = np.full((B, K), 0.5, np.float32)
        for i, (_, _, xm) in enumerate(chunk):
            x[first + i, 0::2] = 1.0
            x[first + i, 1::2] = xm
        x_t = torch.from_numpy(x).to(dtype).to(dev())
        assert torch.equal(x_t.float().cpu(), torch.from_numpy(x))  # every activation is exact in T
        y = gemm(x_t, to_dev(packed), absmax, 16, K).double().cpu().numpy()
        for i, (n, m, xm) in enumerate(chunk):
            exact = (K // 2) * (code[n] + code[m] * xm)
            scale = (K // 2) * (abs(code[n]) + abs(code[m] * xm))
            tol = 1.01 * HALF_ULP[dtype] * abs(exact) + 1e-5 * scale + 1e-30
            ratio = abs(y[first + i, i] - exact) / tol
            worst = max(worst, ratio)
            if ratio > 1:
                failed.append((n, m, ratio))
    print(f"cancellation rows {dtype} B={B} first={first}: worst |err| / tol = {worst:.3f}, {len(failed)} of {len(pairs)} pairs outside")
    assert not failed, (dtype, len(failed), max(f[2] for f in failed), failed[:5])


# ---- 3. every code in the right place ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [576, 1024, 2304])
def test_every_code_and_every_column_tile_in_the_right_place(dtype, K):
    """Row r < 16 is all nibble r; rows 16.. repeat one byte whose two nibbles differ (0x0F, 0xF0, 0x7E, 0x1C).  Activation row b is
    one-hot at k = ks[b % len(ks)] with a value that depends on b: the first and last k, around the 64-weight block, the 256-weight
    unit and the 8-unit pass boundaries, even and odd k.  out[b][r] = T(code[nibble(r, k_b)] * x_b): a swapped nibble, a k order that
    differs between the operands, a wrong table entry or a column tile stored to another tile's rows shows."""
    row_bytes = [n * 17 for n in range(16)] + [0x0F, 0xF0, 0x7E, 0x1C]
    M = len(row_bytes)
    packed = np.repeat(np.array(row_bytes, np.uint8), K // 2)
    absmax = np.ones(M * K // BS, np.float32)
    ks = sorted({0, 1, 2, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512 % K, K - 65, K - 64, K - 2, K - 1})
    vals = [1.0, -1.5, 0.75, 3.0, -0.5, 2.0, -1.25]
    for B in (128, 64, 49, 17):
        for shift in (0, 11):
            x = np.zeros((B, K), np.float32)
            kb = [ks[(b + shift) % len(ks)] for b in range(B)]
            for b in range(B):
                x[b, kb[b]] = vals[b % 7] * (1 + b // 7 % 2)
            x_t = torch.from_numpy(x).to(dtype).to(dev())
            y = gemm(x_t, to_dev(packed), to_dev(absmax), M, K)
            exact, scale = _host_exact(x_t, packed, absmax, M, K)
            want = np.array([[R.CODE[(row_bytes[r] >> 4) if kb[b] % 2 == 0 else (row_bytes[r] & 15)].astype(np.float64) * x[b, kb[b]]
                              for r in range(M)] for b in range(B)])
            assert np.array_equal(exact, want)  # the restatement agrees with the sentence above
            _within_bar(y, exact, scale, dtype, (K, B, shift))


# ---- 4. scales -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [37, 100])
def test_scales_powers_of_two_zero_and_inf(dtype, B):
    M, K = 20, 2048
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
@pytest.mark.parametrize("B,M,K", [(17, 33, 512), (40, 7, 1024), (64, 257, 2048), (65, 1, 4096), (128, 50, 576), (3, 21, 320)])
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
    bad = [dict(K=544), dict(bs=128), dict(bs=32), dict(dtype=torch.float32), dict(B=129), dict(B=1000), dict(K=1024 + 32)]
    for dtype in DTYPES:
        x = torch.randn(129, K, device=dev()).to(dtype)
        out = torch.full((129 * M,), SENTINEL, dtype=torch.int16, device=dev())
        for kw in ({"M": 0}, {"B": 0}):
            a = dict(B=20, M=M, K=1024)
            a.update(kw)
            assert call(x, packed, absmax, out.view(dtype), a["B"], a["M"], a["K"]) == hipabi.OK
        for kw in bad:
            a = dict(B=20, M=M, K=1024, bs=BS, dtype=dtype)
            a.update(kw)
            rc = call(x, packed, absmax, out.view(dtype), a["B"], a["M"], a["K"], bs=a["bs"], dtype=a["dtype"])
            assert rc == hipabi.ERR_UNSUPPORTED, (kw, rc)
            assert "fp4_hip_gemm_wide_nf4" in hipabi.last_error()
        # operands off the 16-byte alignment the kernel's loads need: refused, not misread
        assert call(x.view(-1)[1:], packed, absmax, out.view(dtype), 20, M, 1024) == hipabi.ERR_UNSUPPORTED
        assert call(x, packed[1:], absmax, out.view(dtype), 20, M, 1024) == hipabi.ERR_UNSUPPORTED
        assert call(x, packed, absmax, out.view(dtype), -1, M, 1024) == hipabi.ERR_INVALID
        assert "fp4_hip_gemm_wide_nf4" in hipabi.last_error()
        assert call(None, packed, absmax, out.view(dtype), 20, M, 1024, dtype=dtype) == hipabi.ERR_INVALID
        assert "fp4_hip_gemm_wide_nf4" in hipabi.last_error()
        torch.cuda.synchronize()
        assert (out == SENTINEL).all()


# ---- 6. the forwarded rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_1_to_16_rows_on_k_512_equal_the_small_batch_entry_point_bit_for_bit(dtype):
    g = torch.Generator(device=dev()).manual_seed(17)
    for M, K in [(300, 2048), (33, 512), (1024, 4096)]:
        packed, absmax = _random_nf4(M * K, M + K)
        bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
        x = torch.randn(16, K, device=dev(), generator=g).to(dtype)
        for B in (1, 2, 5, 9, 16):
            for b in (None, bias):
                assert torch.equal(bits_t(gemm(x[:B].contiguous(), packed, absmax, M, K, bias=b)),
                                   bits_t(gemm_small(x[:B].contiguous(), packed, absmax, M, K, bias=b))), (M, K, B, b is None)


# ---- 7. torch op and module ------------------------------------------------------------------------------------------------------------
def _pkg():
    import torch_bnb_fp4 as pkg

    return pkg


@pytest.mark.parametrize("dtype", DTYPES)
def test_torch_op_equals_the_c_abi_bit_for_bit(dtype):
    P = _pkg()
    M, K = 300, 2304
    packed, absmax = _random_nf4(M * K, 77)
    g = torch.Generator(device=dev()).manual_seed(3)
    bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
    for shape in [(17, K), (64, K), (128, K), (5, 20, K), (2, K), (1, K), (K,)]:
        x = torch.randn(*shape, device=dev(), generator=g).to(dtype)
        for b in (None, bias):
            y = P.ext.gemm_wide_nf4(x, packed.view(-1, 1).t(), absmax, BS, [M, K], b)
            assert tuple(y.shape) == tuple(shape[:-1]) + (M,) and y.dtype == dtype
            assert torch.equal(bits_t(y).reshape(-1), bits_t(gemm(x, packed, absmax, M, K, bias=b)).reshape(-1)), (shape, b is None)
    with pytest.raises(RuntimeError):
        P.ext.gemm_wide_nf4(torch.randn(129, K, device=dev()).to(dtype), packed.view(-1, 1).t(), absmax, BS, [M, K], None)
    with pytest.raises(RuntimeError):
        P.ext.gemm_wide_nf4(torch.randn(20, K, device=dev()), packed.view(-1, 1).t(), absmax, BS, [M, K], None)  # f32
    with pytest.raises(RuntimeError):
        P.ext.gemm_wide_nf4(torch.randn(20, 544, device=dev()).to(dtype), packed.view(-1, 1).t(), absmax, BS, [64, 544], None)


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
def test_module_switch_routes_as_specified(dtype):
    P = _pkg()
    root = nn.Sequential(_nf4_layer(1024, 512, seed=1))
    layer, qd = root[0], root[0].quant_data
    assert qd.wide_batch_fused_nf4 is False
    g = torch.Generator(device=dev()).manual_seed(9)
    xs = {rows: torch.randn(rows, 1024, device=dev(), generator=g).to(dtype) for rows in (1, 2, 16, 17, 33, 64, 65, 128, 129, 200)}
    xs["3d"] = torch.randn(5, 8, 1024, device=dev(), generator=g).to(dtype)
    off = {k: layer(x) for k, x in xs.items()}
    # the old switch alone: 17 and 200 rows (and everything above 16) are today's bits
    assert P.set_small_batch_fused(root, True, nf4=True) == 1 and qd.small_batch_fused_nf4 and not qd.wide_batch_fused_nf4
    for k in (17, 64, 128, 200, "3d"):
        assert torch.equal(bits_t(layer(xs[k])), bits_t(off[k])), k
    assert P.set_small_batch_fused(root, False, nf4=True) == 1
    # the new switch alone
    assert P.set_small_batch_fused(root, True, nf4_wide=True) == 1 and qd.wide_batch_fused_nf4 and not qd.small_batch_fused_nf4
    for k, x in xs.items():
        y = layer(x)
        if k in (1, 2, 16, 65, 128, 129, 200):  # one row: the GEMV; 2..16 rows on K % 512 == 0: the other switch; > 64: dequant + GEMM
            assert torch.equal(bits_t(y), bits_t(off[k])), k
            continue
        exact, scale = _restated(layer, x)
        _within_bar(y, exact, scale, dtype, ("module", k))
        assert torch.equal(bits_t(y), bits_t(P.ext.gemm_wide_nf4(x, qd.A.t(), qd.absmax, 64, [512, 1024], qd.bias)))
        assert tuple(y.shape) == tuple(x.shape[:-1]) + (512,)
    assert P.set_small_batch_fused(root, False, nf4_wide=True) == 1 and not qd.wide_batch_fused_nf4
    assert torch.equal(bits_t(layer(xs[64])), bits_t(off[64]))
    # K % 512 != 0: 2..16 rows go to the wide kernel's one-tile form as well
    odd = _nf4_layer(576, 128, seed=4)
    x = torch.randn(4, 576, device=dev(), generator=g).to(dtype)
    y_off = odd(x)
    odd.quant_data.small_batch_fused_nf4 = True
    assert torch.equal(bits_t(odd(x)), bits_t(y_off))
    odd.quant_data.wide_batch_fused_nf4 = True
    oq = odd.quant_data
    assert torch.equal(bits_t(odd(x)), bits_t(P.ext.gemm_wide_nf4(x, oq.A.t(), oq.absmax, 64, [128, 576], oq.bias)))
    exact, scale = _restated(odd, x)
    _within_bar(odd(x), exact, scale, dtype, "module, K = 576")


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [48, 128])
def test_graph_capture_replays_bit_identical_to_eager(dtype, B):
    P = _pkg()
    M, K = 1024, 4096
    packed, absmax = _random_nf4(M * K, 13)
    g = torch.Generator(device=dev()).manual_seed(21)
    bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
    x = torch.randn(B, K, device=dev(), generator=g).to(dtype)
    Bt = packed.view(-1, 1).t()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        P.ext.gemm_wide_nf4(x, Bt, absmax, BS, [M, K], bias)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = P.ext.gemm_wide_nf4(x, Bt, absmax, BS, [M, K], bias)
    for i in range(3):
        x.copy_(torch.randn(B, K, device=dev(), generator=g).to(dtype))
        graph.replay()
        torch.cuda.synchronize()
        eager = P.ext.gemm_wide_nf4(x, Bt, absmax, BS, [M, K], bias)
        assert torch.equal(bits_t(y), bits_t(eager)), i


# ---- 8. hypothesis ---------------------------------------------------------------------------------------------------------------------
_POOL = {}


def _pool():
    if not _POOL:
        _POOL["w"] = _random_nf4(3000 * 64 * 320, 1234)
        g = torch.Generator(device=dev()).manual_seed(4321)
        _POOL["x"] = torch.randn(128, 64 * 320 + 64, device=dev(), generator=g)
        _POOL["b"] = torch.randn(3000, device=dev(), generator=g) * 0.1
    return _POOL


@settings(max_examples=100, **COMMON)
@given(B=st.integers(1, 128), M=st.integers(1, 3000), u=st.integers(1, 320), dtype=st.sampled_from(DTYPES), with_bias=st.booleans(),
       shift=st.integers(0, 63))
def test_hypothesis_draws(B, M, u, dtype, with_bias, shift):
    """Element e of the flat weight is code[nib(e)] * absmax[e // 64] whatever (M, K) is: every draw reads a window of one pool."""
    K = 64 * u
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
