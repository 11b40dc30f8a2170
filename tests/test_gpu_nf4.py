"""NF4 on the MI355X: dequant and quantiser bit-exact to the numpy restatement (tests/nf4_ref.py), the batch-1 GEMV within the
GEMV bar against float64, and the module level (dispatch table, state_dict, device moves, safetensors round trip)."""
import threading

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nf4_ref as R
import torch_bnb_fp4 as pkg
from gpu_util import HALF_ULP, assert_within_bar, bits, dev, to_dev

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def _round_to(v32: np.ndarray, dtype) -> np.ndarray:
    """f32 values -> bit patterns of their RNE rounding to dtype (torch's CPU conversion)."""
    return bits(torch.from_numpy(np.ascontiguousarray(v32)).to(dtype))


def _same_f32(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit equality with every NaN equal to every NaN (the absmax of a block holding a NaN)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all())


# ---- dequant ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_dequant_bit_exact_all_bytes_blocksizes_flags(dtype):
    rng = np.random.default_rng(3)
    for bs in (32, 64, 128, 256, 512, 1024, 2048, 4096):
        for n in (1 << 16, (1 << 16) + 2 * bs - 6, 4 * bs + 14, 37):
            packed = np.tile(np.arange(256, dtype=np.uint8), -(-((n + 1) // 2) // 256))[: (n + 1) // 2]
            rng.shuffle(packed)
            absmax = (rng.standard_normal(-(-n // bs)) * 3).astype(np.float32)
            absmax[0] = 0.0
            want = _round_to(R.dequantize_f32(packed, absmax, bs, n), dtype)
            p, a = to_dev(packed), to_dev(absmax)
            for flags in (hipabi.AUTO, hipabi.KEEP_CACHED, hipabi.STREAM):
                got = hipabi.dequantize(p, a, bs, n, dtype, table=R.TABLE_NF4, flags=flags)
                assert (bits(got) == want).all(), (bs, n, flags)


def test_dequant_past_2_31_elements():
    n = (1 << 31) + 4096 + 10
    bs = 64
    torch.manual_seed(0)
    packed = torch.randint(0, 256, ((n + 1) // 2,), dtype=torch.uint8, device=dev())
    absmax = torch.rand(-(-n // bs), device=dev()) + 0.5
    out = hipabi.dequantize(packed, absmax, bs, n, torch.bfloat16, table=R.TABLE_NF4)
    torch.cuda.synchronize()
    for lo in (0, (1 << 31) - 4096, n - 8192):
        hi = min(n, lo + 8192)
        p = packed[lo // 2: (hi + 1) // 2].cpu().numpy()
        a = absmax.cpu().numpy()[lo // bs: -(-hi // bs)]
        want = _round_to(R.dequantize_f32(p, np.repeat(a, bs)[lo % bs:], 1, hi - lo), torch.bfloat16)
        assert (bits(out[lo:hi]) == want).all(), lo
    del out, packed


_FULL = {}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", [-1, 1, 2, 4, 8, 16, 8 | 256, 2 | 256])
def test_full_size_4096x4096_bit_exact_every_variant(dtype, variant):
    """Every dequant geometry (LOADS | NT << 8) that the FP4 test runs, with the NF4 table (dequant_tiles_nf4_kernel<DT, LOADS, NT>)."""
    n = 4096 * 4096
    if "in" not in _FULL:
        rng = np.random.default_rng(101)
        packed = rng.integers(0, 256, n // 2, dtype=np.uint8)
        am = (rng.random(n // 64, dtype=np.float32) * 0.1 + 0.01).astype(np.float32)
        am[::97] = 0.0
        _FULL["in"] = (packed, am, to_dev(packed), to_dev(am))
    packed, am, P, A = _FULL["in"]
    if dtype not in _FULL:
        _FULL[dtype] = _round_to(R.dequantize_f32(packed, am, 64, n), dtype)
    hipabi.set_variant("dequant", variant)
    out = torch.empty(n, dtype=dtype, device=dev())
    if dtype != torch.float32 and variant in (16, 8 | 256):  # not built for 16-bit output: refused, never computed
        rc = hipabi.lib().fp4_hip_dequantize_blockwise(P.data_ptr(), A.data_ptr(), out.data_ptr(), 64, n, hipabi.DT[dtype], R.TABLE_NF4, 0, None)
        assert rc == hipabi.ERR_INVALID and "unknown kernel variant" in hipabi.last_error()
        return
    hipabi.dequantize(P, A, 64, n, dtype, table=R.TABLE_NF4, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), _FULL[dtype])


# ---- quantiser -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("bs", [32, 64, 4096])
def test_quantize_every_16bit_pattern(dtype, bs):
    pat = np.arange(1 << 16, dtype=np.uint16)
    rng = np.random.default_rng(bs)
    for order in (pat, rng.permutation(pat)):  # natural order: blocks of neighbouring patterns (subnormal, inf, NaN blocks)
        w = torch.from_numpy(order.view(np.int16).copy()).view(dtype)
        want_p, want_a = R.quantize(w.float().numpy(), bs)
        p, a = R.quantize_dev(w.to(dev()), bs)
        assert (p.cpu().numpy() == want_p).all()
        assert _same_f32(a.cpu().numpy(), want_a)


@pytest.mark.parametrize("bs", [32, 64, 128, 512, 1024, 4096])
def test_quantize_f32_random_thresholds_and_special_blocks(bs):
    rng = np.random.default_rng(bs)
    n = 1 << 16
    w = (rng.standard_normal(n) * 0.02).astype(np.float32)
    # values exactly on each threshold and one ulp either side, in blocks whose absmax is exactly 1.0
    edge = np.concatenate([R.THRESHOLDS, np.nextafter(R.THRESHOLDS, np.float32(2)), np.nextafter(R.THRESHOLDS, np.float32(-2)), [1.0]])
    w[: edge.size] = edge
    w[bs: bs + edge.size] = -edge
    w[bs + edge.size: 2 * bs] = 0.0
    w[2 * bs: 3 * bs] = 0.0                      # all-zero block
    w[3 * bs: 4 * bs] = np.inf                   # inf block
    w[4 * bs + 3] = -np.inf
    w[5 * bs + 1] = np.nan                       # NaN block
    w[6 * bs: 7 * bs] = 1e-40                    # subnormal absmax
    w[6 * bs + 5] = -3e-41
    for ragged in (n, n - 6, n - bs - 2):
        want_p, want_a = R.quantize(w[:ragged], bs)
        p, a = R.quantize_dev(to_dev(w[:ragged]), bs)
        assert (p.cpu().numpy() == want_p).all(), ragged
        assert _same_f32(a.cpu().numpy(), want_a), ragged
    assert (want_p[bs: 3 * bs // 2] == 0).all()  # the all-zero block: 0x00 bytes


def _tail_lengths(bs):
    return sorted({1, 3, 7, 9, bs - 1, bs + 1, 4095, 4097, 3 * 4096 - 1, 3 * 4096 + 1, 4096 + bs + 3, 3 * 4096 + bs + 3})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [32, 64, 128, 256, 512, 1024, 2048, 4096])
def test_quantize_odd_and_ragged_lengths(dtype, bs):
    """Odd n leaves a spare low nibble in the last byte: the kernel ranks the zero it pads the last block with, as bitsandbytes does
    (7 under a finite non-zero or an infinite scale, 0 under a zero or NaN one - tests/nf4_ref.py), and writes exactly ceil(n/2)
    bytes.  Ragged lengths around the 4096-element tile, the last block plain, all zero, holding an inf, or holding a NaN."""
    rng = np.random.default_rng(bs)
    for n in _tail_lengths(bs):
        last = (n - 1) // bs * bs
        for tail in ("plain", "zero", "inf", "nan"):
            w32 = (rng.standard_normal(n) * 0.05).astype(np.float32)
            if tail == "zero":
                w32[last:] = 0.0
            elif tail == "inf":
                w32[last + (n - last) // 2] = -np.inf
            elif tail == "nan":
                w32[n - 1] = np.nan
            w = torch.from_numpy(w32).to(dtype)
            want_p, want_a = R.quantize(w.float().numpy(), bs)
            # packed with a guard region behind it: nothing past byte ceil(n/2) - 1 may be written
            buf = torch.full((want_p.size + 64,), 0xA5, dtype=torch.uint8, device=dev())
            absmax = torch.empty(want_a.size, dtype=torch.float32, device=dev())
            rc = R.lib().fp4_hip_quantize_blockwise_nf4(hipabi._ptr(w.to(dev())), hipabi.DT[dtype], hipabi._ptr(buf), hipabi._ptr(absmax), n,
                                                      bs, hipabi._stream())
            assert rc == hipabi.OK, (rc, hipabi.last_error())
            got = buf.cpu().numpy()
            assert (got[: want_p.size] == want_p).all(), (n, tail, got[want_p.size - 2: want_p.size].tolist(), want_p[-2:].tolist())
            assert (got[want_p.size:] == 0xA5).all(), (n, tail)
            assert _same_f32(absmax.cpu().numpy(), want_a), (n, tail)
            if n % 2:
                pad = {"plain": 7, "zero": 0, "inf": 7, "nan": 0}[tail]  # scale finite, 0, inf, NaN
                assert got[want_p.size - 1] & 15 == pad, (n, tail)


def test_quantize_odd_length_first_case_and_the_torch_op():
    """[0.5, 0.1, 0.3] at bs = 32 is F9 D7 (the pad ranks as 0.0 -> 7); the torch op returns [ceil(n/2), 1] bytes for an odd n and
    its n dequantised values are the restatement's, bit for bit."""
    for dtype in DTYPES:
        p, a = R.quantize_dev(torch.tensor([0.5, 0.1, 0.3], dtype=dtype, device=dev()), 32)
        assert p.cpu().numpy().tobytes() == bytes([0xF9, 0xD7]) and a.cpu().tolist() == [0.5], dtype
    rng = np.random.default_rng(8)
    for n in (1, 3, 4097, 65 * 64 + 1):
        for dtype in DTYPES:
            w = torch.from_numpy((rng.standard_normal(n) * 0.05).astype(np.float32)).to(dtype)
            packed, absmax = pkg.quantize_nf4(w.to(dev()), 64)
            assert tuple(packed.shape) == ((n + 1) // 2, 1) and packed.dtype == torch.uint8 and tuple(absmax.shape) == (-(-n // 64),)
            want_p, want_a = R.quantize(w.float().numpy(), 64)
            assert (packed.cpu().numpy().reshape(-1) == want_p).all() and _same_f32(absmax.cpu().numpy(), want_a), (n, dtype)
            d = pkg.dequantize_nf4(packed, absmax, 64, 1, n, dtype)
            assert tuple(d.shape) == (1, n)
            assert (bits(d).reshape(-1) == _round_to(R.dequantize_f32(want_p, want_a, 64, n), dtype)).all(), (n, dtype)


def test_quantize_dequant_quantize_is_a_fixed_point():
    torch.manual_seed(1)
    for dtype in DTYPES:
        w = (torch.randn(1 << 20, device=dev()) * 0.02).to(dtype)
        p1, a1 = R.quantize_dev(w, 64)
        d = hipabi.dequantize(p1, a1, 64, w.numel(), dtype, table=R.TABLE_NF4)
        p2, a2 = R.quantize_dev(d, 64)
        assert torch.equal(p1, p2) and torch.equal(a1, a2), dtype


# ---- GEMV ------------------------------------------------------------------------------------------------------------------------
def _weight(M, K, bs, seed=0, on_gpu=True):
    rng = np.random.default_rng(seed)
    if on_gpu and bs >= 32 and (bs & (bs - 1)) == 0 and M * K >= (1 << 20):
        w = torch.randn(M * K, generator=torch.Generator().manual_seed(seed)).mul_(0.02).to(dev())
        p, a = R.quantize_dev(w, bs)
        del w
        return p, a, p.cpu().numpy(), a.cpu().numpy()
    packed, absmax = R.quantize((rng.standard_normal(M * K) * 0.02).astype(np.float32), bs)
    return to_dev(packed), to_dev(absmax), packed, absmax


def _check_gemv(M, K, bs, dtypes=DTYPES, seed=0):
    p, a, p_np, a_np = _weight(M, K, bs, seed)
    rng = np.random.default_rng(seed + 1)
    x32 = rng.standard_normal(K).astype(np.float32)
    for dtype in dtypes:
        x = torch.from_numpy(x32).to(dtype).to(dev())
        exact, scale = R.gemv_exact(x.float().cpu().numpy(), p_np, a_np, M, K, bs)
        y = R.gemv(x, p, a, M, K, bs)
        assert_within_bar(y, exact, scale, dtype)


@pytest.mark.parametrize("M,K", [(4096, 4096), (14336, 4096), (4096, 14336), (1024, 11008), (512, 32768)])
def test_gemv_decode_shapes(M, K):
    _check_gemv(M, K, 64)


def test_gemv_every_k():
    for K in (32, 64, 96, 128, 160, 256, 480, 1024, 2048, 2080, 4096, 8192, 8224, 16384, 32768):
        for bs in (32, 64, 128):
            if K % bs == 0:
                _check_gemv(64 + K % 7, K, bs, seed=K)


@pytest.mark.parametrize("M,K,bs", [(37, 250, 50), (33, 1000, 40), (17, 4098, 2), (64, 4096, 48), (5, 96, 64)])
def test_gemv_generic_path(M, K, bs):
    _check_gemv(M, K, bs)


@pytest.mark.parametrize("variant", [0, 1])
def test_gemv_table_variants_agree(variant):
    p, a, _, _ = _weight(2048, 4096, 64)
    x = torch.randn(4096, device=dev(), dtype=torch.bfloat16)
    try:
        hipabi.set_variant("gemv_nf4", -1)
        ref = R.gemv(x, p, a, 2048, 4096, 64)
        hipabi.set_variant("gemv_nf4", variant)
        assert torch.equal(R.gemv(x, p, a, 2048, 4096, 64), ref)
    finally:
        hipabi.set_variant("gemv_nf4", -1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_fused_bias_is_bit_identical_to_the_separate_add(dtype):
    M, K, bs = 4096, 4096, 64
    p, a, _, _ = _weight(M, K, bs)
    x = torch.randn(K, device=dev()).to(dtype)
    bias = (torch.randn(M, device=dev()) * 0.1).to(dtype)
    plain = R.gemv(x, p, a, M, K, bs)
    fused = R.gemv(x, p, a, M, K, bs, bias=bias)
    assert torch.equal(bits_t(fused), bits_t((plain.float() + bias.float()).to(dtype)))
    for (m, k, b) in ((37, 250, 50),):  # generic path
        pg, ag, _, _ = _weight(m, k, b)
        xg = torch.randn(k, device=dev()).to(dtype)
        bg = torch.randn(m, device=dev()).to(dtype)
        assert torch.equal(bits_t(R.gemv(xg, pg, ag, m, k, b, bias=bg)), bits_t((R.gemv(xg, pg, ag, m, k, b).float() + bg.float()).to(dtype)))


def bits_t(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_gemv_op_3d_input_graph_capture_and_threads():
    M, K, bs = 4096, 4096, 64
    p, a, _, _ = _weight(M, K, bs)
    B = p.reshape(-1, 1).t()
    x = torch.randn(1, 1, K, device=dev(), dtype=torch.bfloat16)
    q = pkg.ScalarType.bfloat16.value
    y3 = pkg.ext.gemv_nf4(x, B, a, bs, q, [M, K])
    assert tuple(y3.shape) == (1, 1, M)
    y2 = pkg.gemv_nf4(x.view(1, K), B, a, bs, torch.bfloat16, [M, K])
    assert torch.equal(y3.view(1, M), y2)
    assert torch.equal(y2.view(-1), R.gemv(x.view(-1), p, a, M, K, bs))
    # HIP graph capture and replay
    xs = x.view(1, K).clone()
    out = {}
    g = torch.cuda.CUDAGraph()
    pkg.ext.gemv_nf4(xs, B, a, bs, q, [M, K])
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        out["y"] = pkg.ext.gemv_nf4(xs, B, a, bs, q, [M, K])
    for _ in range(3):
        xs.copy_(torch.randn(1, K, device=dev(), dtype=torch.bfloat16))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["y"], pkg.ext.gemv_nf4(xs, B, a, bs, q, [M, K]))
    # two threads launching at once, each on its own stream
    want = pkg.ext.gemv_nf4(xs, B, a, bs, q, [M, K])
    torch.cuda.synchronize()
    errors = []

    def worker():
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(200):
                    y = pkg.ext.gemv_nf4(xs, B, a, bs, q, [M, K])
                s.synchronize()
                if not torch.equal(y, want):
                    errors.append("mismatch")
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker) for _ in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors


# ---- module level --------------------------------------------------------------------------------------------------------------
def _nf4_layer(K=1024, M=512, bias=True, seed=0, dtype=torch.bfloat16):
    torch.manual_seed(seed)
    lin = pkg.LinearNF4(K, M, bias=bias).to(dev())
    return pkg.TorchFP4Linear(lin), lin


def _restated(layer, x):
    qd = layer.quant_data
    w = R.dequantize_f32(qd.A.cpu().numpy().ravel(), qd.absmax.cpu().numpy(), qd.blocksize, qd.M * qd.N).reshape(qd.M, qd.N)
    y = x.double().cpu().numpy() @ w.T.astype(np.float64)
    if layer.bias is not None:
        y = y + layer.bias.detach().double().cpu().numpy()
    return y, np.abs(x.double().cpu().numpy()) @ np.abs(w.T.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_nf4_every_dispatch_row(dtype):
    layer, lin = _nf4_layer()
    assert layer.quant_data.nf4 and torch.equal(layer.code.cpu(), torch.from_numpy(R.CODE))
    K, M = 1024, 512
    h = HALF_ULP[dtype]  # batch > 1 runs dequant (weights rounded to T) + GEMM: allow one rounding per weight and one of the result
    for shape in [(1, K), (1, 1, K), (4, K), (2, 3, K), (1, 2, K), (K,), (200, K)]:
        x = torch.randn(*shape, device=dev()).to(dtype)
        with torch.no_grad():  # the wrapped layer's bias is a Parameter that requires grad: outside no_grad the batch > 1 rows carry
            y = layer(x)       # a grad_fn, as the reference's F.linear does (tests/test_gpu_qlinear_exact.py); this test is inference
        exact, scale = _restated(layer, x.float())
        assert tuple(y.shape) == tuple(shape[:-1]) + (M,)
        err = np.abs(y.double().cpu().numpy() - exact)
        assert (err <= 2.02 * h * (np.abs(exact) + scale) + 1e-5 * scale + 1e-6).all(), shape
    y0 = layer(torch.empty(0, K, device=dev(), dtype=dtype))
    assert tuple(y0.shape) == (0, M)


def test_nf4_state_dict_and_device_moves():
    layer, _ = _nf4_layer()
    x = torch.randn(1, 1024, device=dev(), dtype=torch.bfloat16)
    y = layer(x)
    sd = {k: v.clone() for k, v in layer.state_dict().items()}
    layer.to("cpu")
    assert layer.qweight.device.type == "cpu"
    layer.to(dev())
    assert torch.equal(layer(x), y)
    other, _ = _nf4_layer(seed=5)
    other(x)
    other.load_state_dict(sd)
    assert torch.equal(other(x), y)


def test_nf4_safetensors_round_trip(tmp_path):
    torch.manual_seed(2)
    model = nn.Sequential(nn.Linear(512, 1024), nn.ReLU(), nn.Linear(1024, 256, bias=False))
    model = pkg.recursively_replace_with_fp4_linear(model, as_dtype=torch.bfloat16, device=dev(), quant_type="nf4")
    assert all(m.quant_data.nf4 for m in model.modules() if isinstance(m, pkg.TorchFP4Linear))
    x = torch.randn(3, 512, device=dev(), dtype=torch.bfloat16)
    y = model(x)
    path = str(tmp_path / "nf4.safetensors")
    pkg.save_fp4_model(model, path)
    fresh = nn.Sequential(nn.Linear(512, 1024), nn.ReLU(), nn.Linear(1024, 256, bias=False))
    loaded = pkg.load_fp4_layers(fresh, path, device=dev())
    for a, b in zip([m for m in model.modules() if isinstance(m, pkg.TorchFP4Linear)],
                    [m for m in loaded.modules() if isinstance(m, pkg.TorchFP4Linear)]):
        assert b.quant_data.nf4 and torch.equal(a.qweight, b.qweight) and torch.equal(a.absmax, b.absmax)
    assert torch.equal(loaded(x), y)
    assert torch.equal(loaded(x[:1]), model(x[:1]))


def test_nf4_linear4bit_is_not_decoded_as_fp4():
    """A bitsandbytes-style NF4 Linear4bit (packed NF4 bytes, NF4 quant_map, quant_type "nf4") must compute with the NF4 code;
    before NF4 support the quant_type was never read and the nibbles were decoded with the FP4 table."""
    M, K, bs = 256, 512, 64
    rng = np.random.default_rng(7)
    packed, absmax = R.quantize((rng.standard_normal(M * K) * 0.05).astype(np.float32), bs)
    state = pkg.QuantState(to_dev(absmax), (M, K), to_dev(R.CODE.copy()), bs, torch.float16, quant_type="nf4")
    shell = pkg.LinearFP4(K, M, bias=False, device="meta")
    shell._parameters["weight"] = pkg.Params4bit(to_dev(packed).reshape(-1, 1), False, state, bs, "nf4")
    layer = pkg.TorchFP4Linear(shell)
    for rows in (1, 4):
        x = torch.randn(rows, K, device=dev(), dtype=torch.float32)
        exact, scale = _restated(layer, x)
        err = np.abs(layer(x).double().cpu().numpy() - exact)
        assert (err <= 1e-5 * scale + 1e-5).all(), rows


def test_fp4_only_paths_leave_nf4_alone():
    g, _ = _nf4_layer(K=256, M=512)
    u, _ = _nf4_layer(K=256, M=512, seed=1)
    with pytest.raises(ValueError, match="NF4"):
        pkg.TorchFP4Linear.fuse([g, u])
    with pytest.raises(ValueError, match="NF4"):
        pkg.FusedFP4Linear.from_linear(g)
    mlp = nn.Module()
    mlp.gate_proj, mlp.up_proj, mlp.down_proj, mlp.act_fn = g, u, nn.Identity(), nn.SiLU()
    root = nn.Module()
    root.mlp = mlp
    assert pkg.fuse_gated_mlps(root) == 0 and root.mlp is mlp
    assert pkg.set_small_batch_fused(root) == 0 and not g.quant_data.small_batch_fused


@pytest.mark.parametrize("dtype", DTYPES)
def test_nf4_unfused_bias_is_bit_identical_to_the_fused_call(dtype):
    """fuse_bias=False (GEMV, then out += bias) against the default fused epilogue: T(T(sum) + bias) both ways, 2-D and 3-D tokens."""
    fused, _ = _nf4_layer(K=4096, M=1024, seed=3)
    x = torch.randn(1, 4096, device=dev()).to(dtype)
    y_fused, y3_fused = fused(x), fused(x.view(1, 1, 4096))
    fused.quant_data.fuse_bias = False
    try:
        assert torch.equal(bits_t(fused(x)), bits_t(y_fused))
        assert torch.equal(bits_t(fused(x.view(1, 1, 4096))), bits_t(y3_fused))
    finally:
        fused.quant_data.fuse_bias = True
    exact, scale = _restated(fused, x.float())
    err = np.abs(y_fused.double().cpu().numpy() - exact)
    assert (err <= 2.02 * HALF_ULP[dtype] * (np.abs(exact) + scale) + 1e-5 * scale + 1e-6).all()


def test_nf4_single_token_with_k_not_a_multiple_of_the_blocksize_takes_qlinear_nf4(monkeypatch):
    """One token whose K is not a multiple of the blocksize is not a GEMV row (quant_data.forward): it must run qlinear_nf4[_bias],
    and give exactly what that op gives."""
    from torch_bnb_fp4 import quant_data as qd_mod

    calls = []

    class Recording:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(pkg.ext, name)

    for bias in (True, False):
        layer, _ = _nf4_layer(K=96, M=256, bias=bias, seed=4)
        qd = layer.quant_data
        assert qd.blocksize == 64 and 96 % qd.blocksize
        x = torch.randn(1, 96, device=dev(), dtype=torch.bfloat16)
        layer(x)  # compute dtype set on the first call
        calls.clear()
        monkeypatch.setattr(qd_mod, "ext", Recording())
        with torch.no_grad():  # inference: the bias Parameter requires grad, and outside no_grad qlinear_nf4_bias returns a grad_fn
            y = layer(x)
        monkeypatch.undo()
        assert calls == ["qlinear_nf4_bias" if bias else "qlinear_nf4"], calls
        with torch.no_grad():
            direct = (pkg.ext.qlinear_nf4_bias(x, qd.A, qd.absmax, qd.M, qd.N, qd.blocksize, qd.bias) if bias else
                      pkg.ext.qlinear_nf4(x, qd.A, qd.absmax, qd.M, qd.N, qd.blocksize))
        assert torch.equal(y, direct)
        exact, scale = _restated(layer, x.float())
        err = np.abs(y.double().cpu().numpy() - exact)
        assert (err <= 2.02 * HALF_ULP[torch.bfloat16] * (np.abs(exact) + scale) + 1e-5 * scale + 1e-6).all()
