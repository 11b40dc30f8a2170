"""The batch-1 NF4 GEMV (fp4_hip_gemv_nf4, csrc/gemv_nf4.hip) over the whole range its dispatcher decides on.

* every dispatch cell: dispatch_nf4 picks (ks, G, iters) from (M, K) - the rule is restated in tests/nf4_ref.py (gemv_cell) and
  R.GEMV_CELL_CASES reach each of the 12 cells twice, once with M a multiple of the rows per workgroup and once with a row tail
  (tests/test_nf4_host.py checks that on the host), in f16 / bf16 / f32 and both LDS table layouts, with and without the bias;
* every row length K = 32 .. 32768 on a few rows, block sizes 32 and 64; block sizes 256 .. 4096 on the fast path;
* the generic kernel: K % 32 != 0, x or the packed bytes at an element offset, and M = 0 / K = 0;
* hypothesis draws of M up to 40 000 and K up to 32 768.

Checker: the float64 product of the exact f32 weights, code[nibble] * absmax.  For the large shapes it is formed ON THE DEVICE by
the pure-torch oracle (oracle/torch_cpu.py: table lookup x scale in f32, then a float64 GEMV) with the NF4 code as its table, and
that evaluation is tied to the numpy restatement (nf4_ref.gemv_exact) on sampled rows, first and last included.  The bar is the GEMV
bar of tests/test_gpu_gemv.py: |y - y*| <= ulp_T(y*)/2 * 1.01 + 1e-5 * sum |x_k w_rk|.  NF4 has no sign bit, so the |W| |x| term is
taken from |W| itself (the FP4 helpers clear the sign bits of the packed bytes instead)."""
import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

import hipabi
import nf4_ref as R
from gpu_util import HALF_ULP, assert_within_bar, dev, torch_values
from oracle import torch_cpu

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
COMMON = dict(deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)


@pytest.fixture(autouse=True)
def _nf4_variant():
    """The table layout is a process-wide switch that conftest.py does not reset: every test starts and ends on the default."""
    hipabi.set_variant("gemv_nf4", -1)
    yield
    hipabi.set_variant("gemv_nf4", -1)


def _bits_t(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _random_nf4(n_elems, bs, seed):
    """Random packed bytes + positive scales on the device: every byte is a valid pair of NF4 codes."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    packed = torch.randint(0, 256, (n_elems // 2,), dtype=torch.uint8, device=dev(), generator=g)
    absmax = torch.rand(-(-n_elems // bs), device=dev(), generator=g) * 0.05 + 0.005
    return packed, absmax


_CODE_D = {}


def _code_d():
    if "c" not in _CODE_D:
        _CODE_D["c"] = torch.from_numpy(R.CODE.copy()).to(dev())
    return _CODE_D["c"]


def device_products(packed_d, absmax_d, M, K, bs, xs):
    """float64 (x @ W^T, |x| @ |W|^T) for each device vector of ``xs`` at once, W = code[nibble] * absmax formed by the pure-torch
    oracle on the device in row chunks of <= 32 Mi weights.  Returns two [len(xs), M] float64 device tensors."""
    X = torch.stack([x.double().reshape(-1) for x in xs], 1)
    Xa = X.abs()
    exact = torch.empty(M, len(xs), dtype=torch.float64, device=dev())
    scale = torch.empty_like(exact)
    step = max(1, (1 << 25) // K)
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        w = torch_cpu.dequantize(packed_d[r0 * K // 2:r1 * K // 2], absmax_d[r0 * K // bs:r1 * K // bs], r1 - r0, K, bs, torch.float32,
                                 _code_d()).double()
        exact[r0:r1] = w @ X
        scale[r0:r1] = w.abs() @ Xa  # absmax > 0: |code * absmax| = |code| * absmax exactly
    return exact.t().contiguous(), scale.t().contiguous()


def tie_to_restatement(packed_d, absmax_d, M, K, bs, xs, exact_d, rng, n_rows=14):
    """The device-side product against nf4_ref.gemv_exact (numpy, float64) on the first, last and some random rows."""
    rows = np.unique(np.concatenate([[0, M - 1], rng.integers(0, M, n_rows)]))
    p_rows = packed_d.view(M, K // 2)[torch.from_numpy(rows).to(dev())].cpu().numpy().reshape(-1)
    a_rows = absmax_d.view(M, K // bs)[torch.from_numpy(rows).to(dev())].cpu().numpy().reshape(-1)
    got = exact_d[:, torch.from_numpy(rows).to(dev())].cpu().numpy()
    for i, x in enumerate(xs):
        want, _ = R.gemv_exact(x.double().cpu().numpy(), p_rows, a_rows, len(rows), K, bs)
        assert np.allclose(got[i], want, rtol=1e-11, atol=1e-13), (M, K, i)


def check_bar(y, exact_d, scale_d, dtype, what):
    tol = HALF_ULP[dtype] * 1.01 * exact_d.abs() + 1e-5 * scale_d + 1e-30
    err = (y.double().reshape(-1) - exact_d).abs()
    bad = int((err > tol).sum().item())
    assert bad == 0, (what, dtype, bad, float((err / tol).max().item()), int((err / tol).argmax().item()))


# ---- every dispatch cell ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", R.GEMV_CELL_CASES, ids=[f"{m}x{k}-cell{''.join(map(str, R.gemv_cell(m, k)))}" for m, k in R.GEMV_CELL_CASES])
def test_every_dispatch_cell_rows_tails_dtypes_and_table_layouts(M, K):
    bs = 64 if K % 64 == 0 else 32
    packed_d, absmax_d = _random_nf4(M * K, bs, 7919 * M + K)
    g = torch.Generator().manual_seed(K + 3)
    x32 = torch.randn(K, generator=g)
    b32 = torch.randn(M, generator=g) * 0.1
    xs = [x32.to(dt).to(dev()) for dt in DTYPES]
    exact_d, scale_d = device_products(packed_d, absmax_d, M, K, bs, xs)
    tie_to_restatement(packed_d, absmax_d, M, K, bs, xs, exact_d, np.random.default_rng(M))
    for i, dtype in enumerate(DTYPES):
        bias = b32.to(dtype).to(dev())
        outs = []
        for variant in (0, 1):
            hipabi.set_variant("gemv_nf4", variant)
            y = R.gemv(xs[i], packed_d, absmax_d, M, K, bs)
            check_bar(y, exact_d[i], scale_d[i], dtype, (M, K, R.gemv_cell(M, K), variant))
            # the fused bias: one more rounded add on top of the plain result, T(T(sum) + bias), bit for bit
            fused = R.gemv(xs[i], packed_d, absmax_d, M, K, bs, bias=bias)
            assert torch.equal(_bits_t(fused), _bits_t((y.float() + bias.float()).to(dtype))), (M, K, dtype, variant)
            outs.append(y)
        # the two layouts hold the same f32 code values and sum in the same order
        assert torch.equal(_bits_t(outs[0]), _bits_t(outs[1])), (M, K, dtype)


# ---- every row length --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_row_length_up_to_32768(dtype):
    """K = 32, 64, ..., 32768 on 6 rows, blocksize 32 and (where it divides K) 64: all launches first, one synchronisation, then the
    checker.  Element e of the flat weight is code[nib(e)] * absmax[e // bs] whatever K is, so each K's weight is a prefix of one flat
    restated array."""
    M, K_MAX = 6, 32768
    packed_d, absmax_d = _random_nf4(M * K_MAX, 32, 31)
    g = torch.Generator().manual_seed(32)
    x_all = torch.randn(K_MAX, generator=g).to(dtype)
    x_d = x_all.to(dev())
    xv_all = x_all.float().numpy().astype(np.float64)
    packed = packed_d.cpu().numpy()
    runs = []
    for bs in (32, 64):
        absmax = absmax_d[: M * K_MAX // bs]
        for K in range(32, K_MAX + 1, 32):
            if K % bs:
                continue
            out = torch.empty(M, dtype=dtype, device=dev())
            rc = R.lib().fp4_hip_gemv_nf4(hipabi._ptr(x_d), hipabi._ptr(packed_d), hipabi._ptr(absmax), None, hipabi._ptr(out), M, K, bs,
                                          hipabi.DT[dtype], hipabi._stream())
            assert rc == hipabi.OK, (K, bs, rc, hipabi.last_error())
            runs.append((bs, K, out))
    got_all = torch.stack([o for _, _, o in runs]).double().cpu().numpy()
    flat = {bs: R.dequantize_f32(packed, absmax_d[: M * K_MAX // bs].cpu().numpy(), bs, M * K_MAX).astype(np.float64) for bs in (32, 64)}
    worst = 0.0
    for i, (bs, K, _) in enumerate(runs):
        w = flat[bs][: M * K].reshape(M, K)
        xv = xv_all[:K]
        exact, scale = w @ xv, np.abs(w) @ np.abs(xv)
        tol = HALF_ULP[dtype] * 1.01 * np.abs(exact) + 1e-5 * scale + 1e-30
        err = np.abs(got_all[i] - exact)
        assert (err <= tol).all(), (K, bs, got_all[i], exact, err / tol)
        worst = max(worst, float((err / tol).max()))
    assert len(runs) == 1024 + 512 and worst <= 1.0


# ---- block sizes above 128 on the fast path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [256, 512, 1024, 2048, 4096])
def test_large_block_sizes_on_the_fast_path(bs):
    rng = np.random.default_rng(bs)
    for M, K in ((33, bs), (257, 4096), (130, 12288), (64, 32768)):
        if K % bs:
            continue
        packed, absmax = R.quantize((rng.standard_normal(M * K) * 0.02).astype(np.float32), bs)
        p, a = torch.from_numpy(packed).to(dev()), torch.from_numpy(absmax).to(dev())
        x32 = rng.standard_normal(K).astype(np.float32)
        for dtype in DTYPES:
            x = torch_values(x32, dtype)
            exact, scale = R.gemv_exact(x.float().cpu().numpy(), packed, absmax, M, K, bs)
            assert_within_bar(R.gemv(x, p, a, M, K, bs), exact, scale, dtype)


# ---- the generic kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_generic_path_odd_k_and_offset_operands(dtype):
    rng = np.random.default_rng(17)
    # K % 32 != 0 with block sizes that do and do not divide K
    for M, K, bs in ((70, 4000, 32), (9, 4098, 2), (300, 1000, 40), (5, 30, 64), (129, 8194, 8194)):
        packed, absmax = R.quantize((rng.standard_normal(M * K) * 0.05).astype(np.float32), bs)
        x = torch_values(rng.standard_normal(K), dtype)
        exact, scale = R.gemv_exact(x.float().cpu().numpy(), packed, absmax, M, K, bs)
        assert_within_bar(R.gemv(x, torch.from_numpy(packed).to(dev()), torch.from_numpy(absmax).to(dev()), M, K, bs), exact, scale, dtype)
    # a fast-path shape whose x or packed bytes start 1..3 elements past a 16-byte boundary: routed to the generic kernel, same bar,
    # same fused-bias rule
    M, K, bs = 300, 4096, 64
    packed, absmax = R.quantize((rng.standard_normal(M * K) * 0.05).astype(np.float32), bs)
    a = torch.from_numpy(absmax).to(dev())
    x32 = rng.standard_normal(K)
    bias = torch_values(rng.standard_normal(M) * 0.1, dtype)
    for x_off, p_off in ((0, 0), (1, 0), (0, 1), (3, 5), (2, 8)):
        x_buf = torch.zeros(K + 16, dtype=dtype, device=dev())
        x_buf[x_off:x_off + K] = torch_values(x32, dtype)
        x = x_buf[x_off:x_off + K]
        p_buf = torch.zeros(packed.size + 16, dtype=torch.uint8, device=dev())
        p_buf[p_off:p_off + packed.size] = torch.from_numpy(packed).to(dev())
        p = p_buf[p_off:p_off + packed.size]
        assert (x.data_ptr() % 16 != 0) == (x_off % (16 // x.element_size()) != 0) and (p.data_ptr() % 16 != 0) == (p_off % 16 != 0)
        exact, scale = R.gemv_exact(x.float().cpu().numpy(), packed, absmax, M, K, bs)
        y = R.gemv(x, p, a, M, K, bs)
        assert_within_bar(y, exact, scale, dtype)
        fused = R.gemv(x, p, a, M, K, bs, bias=bias)
        assert torch.equal(_bits_t(fused), _bits_t((y.float() + bias.float()).to(dtype))), (x_off, p_off)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_shapes(dtype):
    """M = 0 writes nothing; K = 0 is an empty sum: zeros, or the bias when there is one."""
    x = torch.randn(64, device=dev()).to(dtype)
    p = torch.zeros(64, dtype=torch.uint8, device=dev())
    a = torch.ones(4, device=dev())
    out = torch.full((4,), float("nan"), dtype=dtype, device=dev())
    R.gemv(x, p, a, 0, 64, 64, out=out)
    torch.cuda.synchronize()
    assert bool(out.isnan().all())  # nothing written
    for M in (1, 5, 300):
        out = torch.full((M,), float("nan"), dtype=dtype, device=dev())
        y = R.gemv(x, p, a, M, 0, 64, out=out)
        assert torch.equal(_bits_t(y), _bits_t(torch.zeros(M, dtype=dtype, device=dev()))), M
        bias = torch.randn(M, device=dev()).to(dtype)
        out = torch.full((M,), float("nan"), dtype=dtype, device=dev())
        yb = R.gemv(x, p, a, M, 0, 64, bias=bias, out=out)
        assert torch.equal(_bits_t(yb), _bits_t(bias)), M


# ---- hypothesis --------------------------------------------------------------------------------------------------------------------
@settings(max_examples=100, **COMMON)
@given(M=st.integers(1, 40000), kc=st.integers(1, 1024), bs_log=st.integers(5, 12), dt=st.sampled_from(DTYPES), bias=st.booleans(),
       variant=st.sampled_from([-1, 0, 1]), seed=st.integers(0, 2**31))
def test_gemv_any_large_shape(M, kc, bs_log, dt, bias, variant, seed):
    """M up to 40 000 and K up to 32 768 (up to 1.3 G weights), a block size that divides K, either table layout: EVERY row against
    the device-side float64 product, tied to the restatement on 16 sampled rows; the fused bias bit for bit."""
    K = kc * 32
    bs = 1 << bs_log
    while K % bs:
        bs >>= 1
    packed_d, absmax_d = _random_nf4(M * K, bs, seed)
    rng = np.random.default_rng(seed)
    x_t = torch_values(rng.standard_normal(K), dt)
    hipabi.set_variant("gemv_nf4", variant)
    y = R.gemv(x_t, packed_d, absmax_d, M, K, bs)
    if bias:
        b_t = torch_values(rng.standard_normal(M) * 0.1, dt)
        fused = R.gemv(x_t, packed_d, absmax_d, M, K, bs, bias=b_t)
        assert torch.equal(_bits_t(fused), _bits_t((y.float() + b_t.float()).to(dt)))
    hipabi.set_variant("gemv_nf4", -1)
    exact_d, scale_d = device_products(packed_d, absmax_d, M, K, bs, [x_t])
    tie_to_restatement(packed_d, absmax_d, M, K, bs, [x_t], exact_d, rng)
    check_bar(y, exact_d[0], scale_d[0], dt, (M, K, bs, variant))
