"""Double-quantised (nested) absmax on the GPU: fp4_hip_absmax_unnest / fp4_hip_absmax_nest against the numpy oracle of
tests/nested_ref.py, fp4_hip_gemv_nested_nf4 against fp4_hip_gemv_fused_nf4 on the ORACLE-expanded absmax, then the torch ops and
the modules.

Bars.  Unnest: bit-exact (two f32 roundings; the fixture is shown, on the CPU, to tell them from a fused multiply-add).  Nest:
nested_absmax bit-exact, codes equal except where the oracle finds the two nearest table entries equidistant.  Round trip:
|unnest(nest(a)) - a| <= 1/2 * (largest gap of the table) * nested_absmax[group] + 2 ulp, the ulp taken at the largest of |a|,
|offset| and the group's scale (the subtraction, the decode's multiply and its add each round once at that magnitude or below).
GEMV: EQUAL BITS in every cell, dtype, table layout and epilogue - the kernel differs from the fused one only in how it obtains
the scale, so no tolerance applies."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nested_ref as N
import nf4_ref as R
from gpu_util import dev, to_dev
from test_gpu_nf4_fused import DT16, GATED, GUARD, NONE, bs_of, gemv_fused, guarded, guards_intact, rand, untouched

pytestmark = pytest.mark.gpu
F32_SENTINEL = 0x7BCD7BCD  # two 16-bit sentinels: the f32 guards use the same pattern


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@functools.lru_cache(maxsize=1)
def table():
    return N.dynamic_map()


@functools.lru_cache(maxsize=1)
def table_dev():
    return to_dev(table())


def unnest(q, nested, code, offset, g, nb=None, out=None, expect_ok=True):
    nb = q.numel() if nb is None else nb
    if out is None:
        out = torch.empty(nb, dtype=torch.float32, device=q.device)
    rc = N.lib().fp4_hip_absmax_unnest(hipabi._ptr(q), hipabi._ptr(nested), hipabi._ptr(code), offset, g, nb, hipabi._ptr(out), hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def nest(a, offset, code, g, q=None, nested=None):
    nb = a.numel()
    q = torch.empty(nb, dtype=torch.uint8, device=a.device) if q is None else q
    nested = torch.empty(-(-nb // g), dtype=torch.float32, device=a.device) if nested is None else nested
    rc = N.lib().fp4_hip_absmax_nest(hipabi._ptr(a), nb, offset, hipabi._ptr(code), g, hipabi._ptr(q), hipabi._ptr(nested), hipabi._stream())
    assert rc == hipabi.OK, (rc, hipabi.last_error())
    return q, nested


def gemv_nested(x, P, q, nested, code, offset, M, K, bs, bias=None, residual=None, epilogue=NONE, out=None, g=256, expect_ok=True, dtype=None):
    if out is None:
        out = torch.empty(M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = N.lib().fp4_hip_gemv_nested_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(q), hipabi._ptr(nested), hipabi._ptr(code), offset, g,
                                         hipabi._ptr(bias), hipabi._ptr(residual), hipabi._ptr(out), M, K, bs, hipabi.DT[dtype or x.dtype],
                                         epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def guarded_f32(n):
    buf = torch.full((n + 2 * GUARD,), F32_SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[GUARD:GUARD + n]


def f32_guards_intact(buf, n):
    return bool((buf[:GUARD] == F32_SENTINEL).all()) and bool((buf[GUARD + n:] == F32_SENTINEL).all())


# ---- unnest --------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_tells_two_roundings_from_an_fma_and_the_kernel_rounds_twice():
    """1000 blocks of 64 draws of 0.05 * N(0, 1), seed 0, absmax nested by the oracle: computed here on the CPU, with the FMA emulated
    in float64, at least 1 % of the expanded values differ between multiply-then-add and a fused multiply-add."""
    a = N.recipe_absmax()
    offset = float(np.float32(a.mean()))
    for g in (64, 256, 4096):
        q, nested, _ = N.nest(a, offset, table(), g)
        two, fma = N.unnest(q, nested, table(), offset, g), N.unnest_fma(q, nested, table(), offset, g)
        differ = int((_bits(two) != _bits(fma)).sum())
        print(f"g = {g}: {differ} of {a.size} expanded values differ between two roundings and an FMA")
        assert differ >= a.size // 100
        got = unnest(to_dev(q), to_dev(nested), table_dev(), offset, g).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(two)), (g, int((_bits(got) != _bits(two)).sum()), int((_bits(got) != _bits(fma)).sum()))


@pytest.mark.parametrize("g", [64, 256, 4096])
@pytest.mark.parametrize("nb", [1, 255, 256, 257, 1000, 262144])
def test_unnest_is_bit_exact(nb, g):
    rng = np.random.default_rng(nb * 7 + g)
    q = rng.integers(0, 256, nb).astype(np.uint8)
    if nb >= 256:
        q[rng.permutation(nb)[:256]] = np.arange(256, dtype=np.uint8)  # every code occurs
        assert len(set(q.tolist())) == 256
    ng = -(-nb // g)
    nested = (rng.random(ng) * 0.05 + 0.01).astype(np.float32)  # a scale of its own per group
    if ng > 2:
        nested[1] = 0.0  # a group that expands to exactly the offset
    qd, nd = to_dev(q), to_dev(nested)
    for offset in (0.0, -0.0173, 0.031):
        want = N.unnest(q, nested, table(), offset, g)
        buf, out = guarded_f32(nb)
        got = unnest(qd, nd, table_dev(), offset, g, out=out)
        assert f32_guards_intact(buf, nb)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (nb, g, offset)
        assert torch.equal(unnest(qd, nd, table_dev(), offset, g), got)  # twice: the same bits
        if ng > 2:
            assert bool((got[g:2 * g] == np.float32(offset)).all())
    # operands that are not aligned for the 4-wide path take the element-wise one: the same bits
    shifted_q = torch.empty(nb + 1, dtype=torch.uint8, device=dev())
    shifted_q[1:] = qd
    buf, out = guarded_f32(nb + 1)
    got = unnest(shifted_q[1:], nd, table_dev(), 0.031, g, out=out[1:])
    assert f32_guards_intact(buf, nb + 1) and int(buf[GUARD]) == F32_SENTINEL
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(N.unnest(q, nested, table(), 0.031, g)))


def test_unnest_captures_in_a_graph_and_refusals_touch_nothing():
    a = N.recipe_absmax()
    q, nested, _ = N.nest(a, 0.02, table(), 256)
    qd, nd = to_dev(q), to_dev(nested)
    out = torch.zeros(a.size, device=dev())
    unnest(qd, nd, table_dev(), 0.02, 256, out=out)  # warm-up: the code object is loaded before the capture
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            unnest(qd, nd, table_dev(), 0.02, 256, out=out)  # the offset is a kernel argument: nothing is read from the host on replay
    torch.cuda.current_stream().wait_stream(side)
    assert bool((out == 0).all())  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(N.unnest(q, nested, table(), 0.02, 256)))
    buf, guarded_out = guarded_f32(a.size)
    for g in (32, 100, 8192):
        assert unnest(qd, nd, table_dev(), 0.02, g, out=guarded_out, expect_ok=False) == hipabi.ERR_UNSUPPORTED
    assert unnest(qd, None, table_dev(), 0.02, 256, out=guarded_out, expect_ok=False) == hipabi.ERR_INVALID
    assert unnest(qd, nd, table_dev(), 0.02, 256, nb=0, out=guarded_out) is guarded_out
    torch.cuda.synchronize()
    assert bool((buf == F32_SENTINEL).all())


# ---- nest ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [64, 256, 4096])
def test_nest_matches_the_oracle_and_round_trips(g):
    a = N.recipe_absmax()  # 1000 blocks: the last group is partial for every g
    t = table()
    for offset in (float(np.float32(a.mean())), 0.0, -0.01):
        wq, wn, ties = N.nest(a, offset, t, g)
        assert int(ties.sum()) == 0  # the smallest gap between the two nearest entries is 3.8e-7 on this fixture: no tie, no excuse
        nb, ng = a.size, -(-a.size // g)
        qbuf = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev())
        nbuf, nview = guarded_f32(ng)
        q, nested = nest(to_dev(a), offset, table_dev(), g, q=qbuf[GUARD:GUARD + nb], nested=nview)
        assert f32_guards_intact(nbuf, ng) and bool((qbuf[:GUARD] == 0xA5).all()) and bool((qbuf[GUARD + nb:] == 0xA5).all())
        assert np.array_equal(_bits(nested.cpu().numpy()), _bits(wn)), (g, offset)
        mismatch = int(((q.cpu().numpy() != wq) & ~ties).sum())
        print(f"g = {g}, offset = {offset}: {mismatch} codes differ from the oracle outside ties")
        assert mismatch == 0
        q2, n2 = nest(to_dev(a), offset, table_dev(), g)
        assert torch.equal(q2, q) and torch.equal(n2, nested)
        # round trip through the device's own expander
        back = unnest(q.contiguous(), nested.contiguous(), table_dev(), offset, g).cpu().numpy().astype(np.float64)
        scale = wn[np.arange(nb) // g].astype(np.float64)
        half_gap = float(np.diff(t.astype(np.float64)).max()) / 2
        ulp = np.spacing(np.maximum(np.maximum(np.abs(a), np.float32(abs(offset))), wn[np.arange(nb) // g]).astype(np.float32)).astype(np.float64)
        err = np.abs(back - a.astype(np.float64))
        bound = half_gap * scale + 2 * ulp
        print(f"  round trip: worst |err| / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all()


def test_nest_all_equal_groups():
    t = table()
    zero_index = int(np.argmin(np.abs(t)))
    assert t[zero_index] == 0.0 and zero_index == 127
    a = np.full(700, 0.0421, np.float32)
    a[512:] = 0.07  # the partial last group of g = 256 differs from the offset
    ad = to_dev(a)
    # offset == the value: m == 0, every code the table's 0.0, and the group expands to exactly the offset
    q, nested = nest(ad, float(np.float32(0.0421)), table_dev(), 256)
    wq, wn, _ = N.nest(a, float(np.float32(0.0421)), t, 256)
    assert np.array_equal(q.cpu().numpy(), wq) and np.array_equal(_bits(nested.cpu().numpy()), _bits(wn))
    assert bool((q[:512] == zero_index).all()) and bool((nested[:2] == 0).all()) and float(nested[2]) > 0
    back = unnest(q, nested, table_dev(), float(np.float32(0.0421)), 256)
    assert bool((back[:512] == np.float32(0.0421)).all())
    # offset 0: every |n| is exactly 1, the last entry of the table
    q, nested = nest(ad, 0.0, table_dev(), 256)
    assert bool((q == 255).all()) and np.array_equal(_bits(nested.cpu().numpy()), _bits(np.array([0.0421, 0.0421, 0.07], np.float32)))
    assert np.array_equal(_bits(unnest(q, nested, table_dev(), 0.0, 256).cpu().numpy()), _bits(a))


# ---- GEMV ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def nested_weight(M, K, bs):
    """Random NF4 bytes with double-quantised statistics whose group scales and codes differ everywhere, and the ORACLE's expansion
    of them (numpy, on the CPU) as the f32 absmax the fused entry point is given."""
    g = torch.Generator(device=dev()).manual_seed(29 * M + K)
    packed = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev(), generator=g)
    nb = M * K // bs
    rng = np.random.default_rng(M * 3 + K)
    q = rng.integers(0, 256, nb).astype(np.uint8)
    nested = (rng.random(-(-nb // 256)) * 0.03 + 0.01).astype(np.float32)
    offset = float(np.float32(0.0237 + (M % 7) * 0.001))
    expanded = N.unnest(q, nested, table(), offset, 256)
    return packed, to_dev(q), to_dev(nested), offset, to_dev(expanded)


@pytest.mark.parametrize("M,K", R.GEMV_CELL_CASES, ids=[f"{m}x{k}" for m, k in R.GEMV_CELL_CASES])
def test_gemv_nested_equals_the_fused_gemv_on_the_expanded_absmax(M, K):
    """Every cell of the dispatcher (tests/nf4_ref.py), both table layouts, three dtypes.  At K = 1024 a group of 256 blocks spans 16
    rows, at K = 32768 a row spans two groups, and 1023 x 992 / 4097 x 800 (blocksize 32) have a block count that is no multiple of
    256: a group index taken from the row, the chunk or a rounded-up count shows."""
    bs = bs_of(K)
    P, q, nested, offset, A = nested_weight(M, K, bs)
    code = table_dev()
    try:
        for variant in (0, 1):
            hipabi.set_variant("gemv_nf4", variant)
            for dtype in DT16 + [torch.float32]:
                x, b, r = rand(K, dtype, K), rand(M, dtype, M, 0.1), rand(M, dtype, M + 1)
                for bias, res in ((None, None), (b, r), (b, None), (None, r)):
                    want = gemv_fused(x, P, A, M, K, bs, bias, res)
                    if dtype == torch.float32:
                        got = gemv_nested(x, P, q, nested, code, offset, M, K, bs, bias, res)
                    else:
                        buf, out = guarded(M, dtype)
                        got = gemv_nested(x, P, q, nested, code, offset, M, K, bs, bias, res, out=out)
                        assert guards_intact(buf, M)
                    assert torch.equal(got, want), (variant, dtype, bias is not None, res is not None, int((got != want).sum()))
                h = r.clone()  # in place: the residual aliases out
                gemv_nested(x, P, q, nested, code, offset, M, K, bs, b, h, out=h)
                assert torch.equal(h, gemv_fused(x, P, A, M, K, bs, b, r))
                if M % 2 == 0 and dtype != torch.float32:
                    rh = r[: M // 2].contiguous()
                    for bias, res in ((None, None), (b, rh)):
                        buf, out = guarded(M // 2, dtype)
                        got = gemv_nested(x, P, q, nested, code, offset, M, K, bs, bias, res, GATED, out=out)
                        assert guards_intact(buf, M // 2)
                        assert torch.equal(got, gemv_fused(x, P, A, M, K, bs, bias, res, GATED)), (variant, dtype, "gated")
                    h = rh.clone()
                    gemv_nested(x, P, q, nested, code, offset, M, K, bs, b, h, GATED, out=h)
                    assert torch.equal(h, gemv_fused(x, P, A, M, K, bs, b, rh, GATED))
    finally:
        hipabi.set_variant("gemv_nf4", -1)


def test_gemv_nested_on_statistics_nested_by_the_device():
    """The whole chain on the device: quantise, nest, then the nested GEMV against the fused one on the device's own expansion."""
    M, K = 1024, 4096
    w = rand(M * K, torch.bfloat16, 3, 0.05)
    P, absmax = R.quantize_dev(w, 64)
    offset = float(absmax.mean())
    q, nested = nest(absmax, offset, table_dev(), 256)
    expanded = unnest(q, nested, table_dev(), offset, 256)
    half_gap = float(np.diff(table().astype(np.float64)).max()) / 2  # the round-trip bound of the nest test, at the largest group scale
    assert float((expanded - absmax).abs().max()) <= half_gap * float(nested.max()) + 2 * float(np.spacing(np.float32(absmax.max().item())))
    x = rand(K, torch.bfloat16, 5)
    assert torch.equal(gemv_nested(x, P, q, nested, table_dev(), offset, M, K, 64), gemv_fused(x, P, expanded, M, K, 64))


def test_gemv_nested_refusals_leave_out_untouched():
    M, K = 64, 1024
    P, q, nested, offset, A = nested_weight(M, K, 64)
    code = table_dev()
    x16 = rand(K + 8, torch.bfloat16, 1)
    buf, out = guarded(M, torch.bfloat16)
    call = lambda x, m, k, bs, epi, **kw: gemv_nested(x, P, q, nested, code, offset, m, k, bs, None, None, epi, out=out, expect_ok=False, **kw)
    for epi in (NONE, GATED):
        for g in (64, 128, 512, 4096):
            assert call(x16[:K], M, K, 64, epi, g=g) == hipabi.ERR_UNSUPPORTED and "nested_blocksize" in hipabi.last_error()
        assert call(x16[:1008], M, 1008, 16, epi) == hipabi.ERR_UNSUPPORTED and "not available" in hipabi.last_error()
        assert call(x16[1:K + 1], M, K, 64, epi) == hipabi.ERR_UNSUPPORTED
    out32 = torch.full((M,), 123.0, device=dev())
    assert gemv_nested(rand(K, torch.float32, 1), P, q, nested, code, offset, M, K, 64, None, None, GATED, out=out32,
                       expect_ok=False) == hipabi.ERR_UNSUPPORTED
    assert call(x16[:K], M - 1, K, 64, GATED) == hipabi.ERR_INVALID and "even row count" in hipabi.last_error()
    assert call(x16[:K], M, K, 64, 7) == hipabi.ERR_INVALID
    assert call(x16[:K], M, K, 64, NONE, g=0) == hipabi.ERR_INVALID
    assert call(x16[:K], 0, K, 64, NONE) == hipabi.OK
    torch.cuda.synchronize()
    assert untouched(buf) and bool((out32 == 123.0).all())


# ---- torch ops -----------------------------------------------------------------------------------------------------------------------
def test_torch_ops_equal_the_c_abi_bit_for_bit():
    import torch_bnb_fp4 as pkg

    a = N.recipe_absmax()
    ad = to_dev(a)
    q, nested = pkg.ext.absmax_nest(ad, 0.02, table_dev(), 256)
    cq, cn = nest(ad, 0.02, table_dev(), 256)
    assert torch.equal(q, cq) and torch.equal(nested, cn) and q.dtype == torch.uint8 and nested.shape == (4,)
    assert torch.equal(pkg.ext.absmax_unnest(q, nested, table_dev(), 0.02, 256), unnest(cq, cn, table_dev(), 0.02, 256))
    with pytest.raises(RuntimeError, match="nested_blocksize"):
        pkg.ext.absmax_unnest(q, torch.cat([nested] * 3), table_dev(), 0.02, 100)  # enough scales for groups of 100: the C ABI refuses
    for M, K in ((1026, 3104), (258, 2048)):
        bs = bs_of(K)
        P, q, nested, offset, A = nested_weight(M, K, bs)
        Bt = P.reshape(-1, 1).t()
        for dtype in DT16 + [torch.float32]:
            b = rand(M, dtype, M, 0.1)
            x = rand((1, K), dtype, 1, 2.0)
            for epi in (NONE, GATED) if dtype != torch.float32 else (NONE,):
                r = rand((1, M // 2 if epi == GATED else M), dtype, 9)
                got = pkg.ext.gemv_nf4_nested(x, Bt, q, nested, table_dev(), offset, 256, bs, [M, K], b, r, epi)
                want = gemv_nested(x.reshape(-1), P, q, nested, table_dev(), offset, M, K, bs, b, r.reshape(-1), epi).reshape(1, -1)
                assert torch.equal(got, want) and got.shape == (1, M // 2 if epi == GATED else M)
            assert pkg.ext.gemv_nf4_nested(x.view(1, 1, K), Bt, q, nested, table_dev(), offset, 256, bs, [M, K], None, None, NONE).shape == (1, 1, M)
            for rows in (8, 64):
                xb = rand((rows, K), dtype, rows)
                for bias in (None, b):
                    got = pkg.ext.qlinear_nf4_nested(xb, P.reshape(-1, 1), q, nested, table_dev(), offset, 256, M, K, bs, bias)
                    want = pkg.ext.qlinear_nf4(xb, P.reshape(-1, 1), A, M, K, bs) if bias is None else pkg.ext.qlinear_nf4_bias(
                        xb, P.reshape(-1, 1), A, M, K, bs, bias)
                    assert torch.equal(got, want)
    P, q, nested, offset, A = nested_weight(258, 2048, 64)
    with pytest.raises(RuntimeError, match="nested_blocksize"):
        pkg.ext.gemv_nf4_nested(rand((1, 2048), torch.bfloat16, 1), P.reshape(-1, 1).t(), q, torch.cat([nested] * 4), table_dev(), offset, 64, 64,
                                [258, 2048], None, None, NONE)


# ---- modules -------------------------------------------------------------------------------------------------------------------------
class _MLP(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = nn.Linear(H, I, bias=False), nn.Linear(H, I, bias=False), nn.Linear(I, H)
        self.act_fn = nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class _Net(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.mlp = _MLP(H, I)
        self.odd = nn.Linear(48, 32, bias=False)  # in_features % 32 != 0: outside the nested GEMV, expanded in resident mode

    def forward(self, x):
        return self.mlp(x)


@pytest.fixture(scope="module")
def nested_file(tmp_path_factory):
    """A double-quantised NF4 checkpoint written by save_fp4_model(nested=True) from a freshly quantised model."""
    import torch_bnb_fp4 as pkg

    H, I = 512, 768
    torch.manual_seed(5)
    net = pkg.recursively_replace_with_fp4_linear(_Net(H, I).to(torch.bfloat16), as_dtype=torch.bfloat16, device=dev(), quant_type="nf4")
    path = str(tmp_path_factory.mktemp("nested") / "model.safetensors")
    pkg.save_fp4_model(net, path, nested=True)
    return path, H, I, net


def test_nested_save_is_lossy_within_the_round_trip_bound_and_modules_agree(nested_file):
    import torch_bnb_fp4 as pkg
    from safetensors.torch import load_file

    path, H, I, net = nested_file
    state = load_file(path)
    assert state["mlp.gate_proj.weight.absmax"].dtype == torch.uint8 and "mlp.gate_proj.weight.nested_quant_map" in state
    resident = pkg.load_fp4_layers(_Net(H, I).to(torch.bfloat16), path, device=dev(), nested="resident")
    expanded = pkg.load_fp4_layers(_Net(H, I).to(torch.bfloat16), path, device=dev())
    assert resident.fp4_nested_expanded == ["odd"] and expanded.fp4_nested_expanded == []
    assert type(resident.odd) is pkg.TorchFP4Linear
    half_gap = float(np.diff(table().astype(np.float64)).max()) / 2
    for name in ("gate_proj", "up_proj", "down_proj"):
        res, exp, orig = getattr(resident.mlp, name), getattr(expanded.mlp, name), getattr(net.mlp, name)
        assert type(res) is pkg.NestedNF4Linear and type(exp) is pkg.TorchFP4Linear
        assert torch.equal(res.expanded_absmax(), exp.absmax) and torch.equal(res.qweight, exp.qweight)
        # lossy in the scales, by no more than the round-trip bound (2 ulp of the scales' magnitude is below 1e-8 here)
        assert float((exp.absmax - orig.absmax).abs().max()) <= half_gap * float(res.nested_absmax.max()) + 1e-8
        assert float((exp.absmax - orig.absmax).abs().max()) > 0
        # device bytes of the statistics: a quarter and a bit
        stat_res = res.absmax_u8.numel() + 4 * res.nested_absmax.numel() + 4 * res.nested_code.numel()
        assert stat_res < 0.3 * 4 * exp.absmax.numel()
        for rows in (1, 2, 24):
            x = rand((rows, res.in_features), torch.bfloat16, rows, 0.5)
            assert torch.equal(res(x), exp(x)), (name, rows)
        x3 = rand((1, 1, res.in_features), torch.bfloat16, 3, 0.5)
        assert torch.equal(res(x3), exp(x3)) and res(x3).shape == (1, 1, res.out_features)
        r = rand((1, res.out_features), torch.bfloat16, 4)
        assert torch.equal(res(x3.view(1, -1), r), exp(x3.view(1, -1)) + r)
        r24 = rand((24, res.out_features), torch.bfloat16, 6)
        x24 = rand((24, res.in_features), torch.bfloat16, 24, 0.5)
        assert torch.equal(res(x24, r24), exp(x24) + r24)
        assert torch.equal(res.dequantize(torch.bfloat16), exp.quant_data.dequantize())
        assert type(res.expand()) is pkg.TorchFP4Linear and torch.equal(res.expand()(x24), exp(x24))
    h = rand((1, H), torch.bfloat16, 8, 0.5)
    assert torch.equal(resident(h), expanded(h))
    # a GraphedStep replay equals eager
    step = pkg.GraphedStep(lambda t: resident.mlp.down_proj(resident.mlp.gate_proj(t)), h)
    for scale in (1.0, -0.5):
        assert torch.equal(step(h * scale), resident.mlp.down_proj(resident.mlp.gate_proj(h * scale)))
    # device moves keep the module whole
    moved = resident.mlp.gate_proj.to("cpu")
    assert moved.absmax_u8.device.type == "cpu" and moved.nested_code.device.type == "cpu"
    moved.to(dev())
    assert torch.equal(moved(h), expanded.mlp.gate_proj(h))


def test_a_resident_model_saved_nested_loads_back_bit_identical(nested_file, tmp_path):
    import torch_bnb_fp4 as pkg
    from safetensors.torch import load_file

    path, H, I, _ = nested_file
    resident = pkg.load_fp4_layers(_Net(H, I).to(torch.bfloat16), path, device=dev(), nested="resident")
    resident.odd = nn.Identity()  # (an expanded layer would be nested again on the way out: lossy, not this test's subject)
    again = str(tmp_path / "again.safetensors")
    pkg.save_fp4_model(resident, again, nested=True)
    a, b = load_file(path), load_file(again)
    keys = [k for k in a if k.startswith("mlp.")]
    assert sorted(keys) == sorted(b) and all(torch.equal(a[k], b[k]) for k in keys)
    back = pkg.load_fp4_layers(_Net(H, I).to(torch.bfloat16), again, device=dev(), nested="resident", strict=False)
    for name in ("gate_proj", "up_proj", "down_proj"):
        one, two = getattr(resident.mlp, name), getattr(back.mlp, name)
        assert type(two) is pkg.NestedNF4Linear and one.offset == two.offset
        for buf in ("qweight", "absmax_u8", "nested_absmax", "nested_code", "code"):
            assert torch.equal(getattr(one, buf), getattr(two, buf))
        assert (one.bias is None) == (two.bias is None) and (one.bias is None or torch.equal(one.bias, two.bias))
    h = rand((1, H), torch.bfloat16, 8, 0.5)
    assert torch.equal(back.mlp(h), resident.mlp(h))
    # the state dict of the module round-trips too (the offset is extra state)
    fresh = pkg.load_fp4_layers(_Net(H, I).to(torch.bfloat16), path, device=dev(), nested="resident")
    fresh.mlp.down_proj.offset = 0.0
    fresh.mlp.down_proj.absmax_u8.zero_()
    fresh.mlp.down_proj.load_state_dict(resident.mlp.down_proj.state_dict())
    assert torch.equal(fresh.mlp.down_proj(rand((1, I), torch.bfloat16, 2)), resident.mlp.down_proj(rand((1, I), torch.bfloat16, 2)))


def test_an_expanded_load_takes_the_surgery_and_a_resident_one_after_expand_nested(nested_file):
    import torch_bnb_fp4 as pkg

    path, H, I, _ = nested_file
    expanded = pkg.load_fp4_layers(_Net(H, I).to(torch.bfloat16), path, device=dev())
    resident = pkg.load_fp4_layers(_Net(H, I).to(torch.bfloat16), path, device=dev(), nested="resident")
    assert pkg.fuse_gated_mlps(resident, nf4=True) == 0  # not recognised: compressed groups span rows
    pkg.expand_nested(resident)
    assert all(type(m) is not pkg.NestedNF4Linear for m in resident.modules())
    g = torch.Generator().manual_seed(4)
    r = 8
    adapter = {}
    for name, (M, K) in (("mlp.gate_proj", (I, H)), ("mlp.up_proj", (I, H)), ("mlp.down_proj", (H, I))):
        adapter[f"base_model.model.{name}.lora_A.weight"] = torch.randn(r, K, generator=g) / K**0.5
        adapter[f"base_model.model.{name}.lora_B.weight"] = torch.randn(M, r, generator=g) * 0.05
    outs = []
    for model in (expanded, resident):
        assert pkg.fuse_gated_mlps(model, nf4=True) == 1
        assert pkg.attach_lora(model, adapter, r=r, lora_alpha=16) == 2
        assert type(model.mlp.gate_up) is pkg.LoRANF4Linear
        for rows in (1, 8):
            y = model(rand((rows, H), torch.bfloat16, rows, 0.5))
            assert y.shape == (rows, H) and bool(torch.isfinite(y.float()).all())
            outs.append(y)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
