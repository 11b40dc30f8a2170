"""The fused NF4 decode epilogues on the host (no GPU): the two C entry points' argument validation (every call below returns
before any HIP call), the GPU suite's case lists against the restated dispatchers, and FusedNF4Linear / fuse_gated_mlps /
save_fp4_model through a numpy-backed fake extension."""
import ctypes
import types

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nf4_fused_cases as FC
import nf4_ref as R
import nf4_wide_cases as C
import torch_bnb_fp4 as pkg
from oracle import fp4_oracle as o
from test_nf4_host import RecordingNf4Ext
from torch_bnb_fp4 import functional as F_mod, fused as fused_mod, quant_data as qd_mod

NONE, GATED = 0, 1
OK, INVALID, UNSUPPORTED = 0, 1, 2
F16, F32, BF16 = 0, 1, 2


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


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_both_entry_points():
    assert {"fp4_hip_gemv_fused_nf4", "fp4_hip_gemm_fused_nf4"} <= set(hipabi.declared_symbols())
    assert _lib().fp4_hip_abi_version() == 7


def test_gemv_fused_nf4_argument_validation():
    l, d = _lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    gemv = lambda x, out, M, K, bs, dt, epi: l.fp4_hip_gemv_fused_nf4(x, d, d, None, None, out, M, K, bs, dt, epi, None)
    assert gemv(d, d, 64, 64, 64, BF16, 7) == INVALID and "unknown epilogue" in err()
    assert gemv(d, d, 63, 64, 64, BF16, GATED) == INVALID and "even row count" in err()
    assert gemv(d, d, -1, 64, 64, BF16, NONE) == INVALID
    assert gemv(d, d, 64, 33, 64, BF16, NONE) == INVALID  # odd K
    assert gemv(d, d, 64, 64, 64, 5, NONE) == UNSUPPORTED and "dtype" in err()
    assert gemv(None, None, 0, 64, 64, BF16, NONE) == OK  # M == 0: nothing to do
    assert gemv(None, None, 0, 64, 64, BF16, GATED) == OK
    assert gemv(None, d, 64, 64, 64, BF16, NONE) == INVALID and "null" in err()
    assert gemv(d, None, 64, 64, 64, BF16, NONE) == INVALID
    # outside the fast path, whatever the epilogue: reported, never computed (the plain entry point would run its generic kernel)
    for epi in (NONE, GATED):
        assert gemv(d, d, 64, 48, 16, BF16, epi) == UNSUPPORTED and "not available" in err()          # K % 32 != 0
        assert gemv(d, d, 64, 96, 96, BF16, epi) == UNSUPPORTED and "not available" in err()          # blocksize not a power of two
        assert gemv(d, d, 64, 64, 128, BF16, epi) == UNSUPPORTED                                       # blocksize does not divide K
        assert gemv(ctypes.c_void_p(0x1002), d, 64, 64, 64, BF16, epi) == UNSUPPORTED and "not available" in err()
    assert gemv(d, d, 64, 64, 64, F32, GATED) == UNSUPPORTED and "not available" in err()
    assert gemv(d, d, 1 << 31, 64, 64, BF16, NONE) == UNSUPPORTED


def test_gemm_fused_nf4_argument_validation():
    l, d = _lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    gemm = lambda x, out, B, M, K, bs, dt, epi: l.fp4_hip_gemm_fused_nf4(x, d, d, None, None, out, B, M, K, bs, dt, epi, None)
    assert gemm(d, d, 4, 64, 64, 64, BF16, 2) == INVALID and "unknown epilogue" in err()
    assert gemm(d, d, 4, 63, 64, 64, BF16, GATED) == INVALID and "even row count" in err()
    assert gemm(d, d, -1, 64, 64, 64, BF16, NONE) == INVALID
    assert gemm(d, d, 4, 64, 0, 64, BF16, NONE) == INVALID
    for epi in (NONE, GATED):
        assert gemm(d, d, 129, 64, 64, 64, BF16, epi) == UNSUPPORTED and "not covered" in err()
        assert gemm(d, d, 4, 64, 64, 32, BF16, epi) == UNSUPPORTED and "not covered" in err()   # blocksize != 64
        assert gemm(d, d, 4, 64, 96, 64, BF16, epi) == UNSUPPORTED                                # K % 64 != 0
        assert gemm(d, d, 4, 64, 64, 64, F32, epi) == UNSUPPORTED and "not covered" in err()
        assert gemm(ctypes.c_void_p(0x1008), d, 4, 64, 64, 64, F16, epi) == UNSUPPORTED
        assert gemm(None, None, 4, 0, 64, 64, BF16, epi) == OK
        assert gemm(None, None, 0, 64, 64, 64, BF16, epi) == OK
    assert gemm(None, d, 4, 64, 64, 64, BF16, NONE) == INVALID and "null" in err()
    assert gemm(d, None, 4, 64, 512, 64, BF16, GATED) == INVALID


# ---- the GPU suite's cases reach every dispatcher cell ------------------------------------------------------------------------------
def test_gemv_case_lists_reach_every_cell():
    """12 cells (ks, G, iters); the plain list and the gated (even M) list each see every cell once with M a multiple of the rows per
    workgroup and once with a row tail - where an even M can have one (two rows per workgroup: ks 4, iters 1 cannot)."""
    all_cells = {(ks, 1, it) for ks in (1, 2, 4) for it in (1, 2, 4)} | {(4, 2, it) for it in (1, 2, 4)}
    for cases, even in ((FC.GEMV_PLAIN, False), (FC.GEMV_GATED, True)):
        seen = {}
        for M, K in cases:
            assert K % 32 == 0 and 0 < K <= 32768 and M > 0 and not (even and M % 2)
            ks, G, it = R.gemv_cell(M, K)
            seen.setdefault((ks, G, it), set()).add(M % R.rows_per_workgroup(ks, it) != 0)
        assert set(seen) == all_cells
        for (ks, G, it), tails in seen.items():
            can_tail = not even or R.rows_per_workgroup(ks, it) > 2
            assert tails == ({False, True} if can_tail else {False}), (ks, G, it, tails)
    # the gated cases sit in the cells of the originals they were derived from
    assert [R.gemv_cell(*s) for s in FC.GEMV_GATED] == [R.gemv_cell(*s) for s in R.GEMV_CELL_CASES]
    assert {R.gemv_cell(*s)[0] for s in FC.GEMV_VARIANT_SHAPES} == {1, 2, 4} and {R.gemv_cell(*s)[1] for s in FC.GEMV_VARIANT_SHAPES} == {1, 2}


def test_batched_case_list_reaches_every_cell():
    seen, small = set(), 0
    for M, K in FC.BATCH_SHAPES:
        assert M % 2 == 0 and K % 64 == 0
        for B in FC.rows_for(K):
            for c in C.cells(B, M, K):
                if c == "small":
                    small += 1
                else:
                    seen.add(c)
    assert seen == C.ALL_CELLS and len(seen) == 16 and small >= 3
    assert [(M, K) for (M, K), (M0, _) in zip(FC.BATCH_SHAPES, C.SHAPES) if M != M0] == [(34, 576), (8, 1280), (258, 2048)]
    # both chunkings of the two-launch range, and a second chunk shorter than the first
    assert C.chunks(65) == [33, 32] and C.chunks(128) == [64, 64]


# ---- modules through a fake extension -----------------------------------------------------------------------------------------------
class FusedNf4Ext(RecordingNf4Ext):
    """RecordingNf4Ext plus the two fused ops, answered from the numpy restatement and the oracle's epilogues."""

    refuse_gemv = refuse_gemm = None

    def code_table(self, name):
        assert name == "nf4", "an NF4 layer asked for an FP4 table"
        return torch.from_numpy(R.CODE.copy())

    def _fused(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue, gemv):
        M, K = Bshape
        name = {torch.float16: "float16", torch.bfloat16: "bfloat16", torch.float32: "float32"}[A.dtype]
        w = R.dequantize_f32(B.numpy().ravel(), absmax.numpy(), blocksize, M * K).reshape(M, K).astype(np.float64)
        y = A.float().numpy().reshape(-1, K).astype(np.float64) @ w.T
        nb = None if bias is None else bias.float().numpy()
        nr = None if residual is None else residual.float().numpy().reshape(y.shape[0], -1)
        if not gemv and nb is not None:  # F.linear: the bias joins the f32 sum before the one rounding
            y, nb = y + nb.astype(np.float64), None
        if epilogue == 1:
            t = o.linear_epilogue(y, name, nb)
            t = o.silu_mul_epilogue(t[:, 0::2], t[:, 1::2], name, nr)
        else:
            t = o.linear_epilogue(y, name, nb, nr)
        return torch.from_numpy(np.asarray(t, np.float32)).to(A.dtype).view(*A.shape[:-1], -1)

    def gemv_nf4_fused(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue):
        self.calls.append("gemv_nf4_fused")
        if self.refuse_gemv:
            raise RuntimeError(self.refuse_gemv)
        assert A.is_contiguous() and A.numel() == Bshape[1]
        return self._fused(A, B, absmax, blocksize, Bshape, bias, residual, epilogue, True)

    def gemm_nf4_fused(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue):
        self.calls.append("gemm_nf4_fused")
        if self.refuse_gemm:
            raise RuntimeError(self.refuse_gemm)
        assert 1 <= A.numel() // Bshape[1] <= 128
        return self._fused(A, B, absmax, blocksize, Bshape, bias, residual, epilogue, False)


@pytest.fixture()
def fx(monkeypatch):
    r = FusedNf4Ext()
    for mod in (F_mod, qd_mod, fused_mod):
        monkeypatch.setattr(mod, "ext", r)
    monkeypatch.setattr(fused_mod, "nf4_code", lambda: torch.from_numpy(R.CODE.copy()))
    return r


def _packed(M, K, seed, bs=64):
    rng = np.random.default_rng(seed)
    p, a = R.quantize((rng.standard_normal(M * K) * 0.05).astype(np.float32), bs)
    return torch.from_numpy(p).reshape(-1, 1), torch.from_numpy(a)


class HostParams4bit(pkg.Params4bit):
    """A Params4bit that says it lives on a GPU: TorchFP4Linear insists on that, and these tests run its host logic on CPU tensors."""

    device = property(lambda self: torch.device("cuda", 0))


def _layer(packed, absmax, code, M, K, quant_type, bias):
    state = pkg.QuantState(absmax, (M, K), code, 64, quant_type=quant_type)
    shell = pkg.LinearFP4(K, M, bias=bias is not None, device="meta")
    shell._parameters["weight"] = HostParams4bit(packed, False, state, 64, quant_type)
    if bias is not None:
        shell._parameters["bias"] = nn.Parameter(bias, requires_grad=False)
    return pkg.TorchFP4Linear(shell)


def _nf4_layer(M, K, seed, bias=True):
    p, a = _packed(M, K, seed)
    b = torch.from_numpy(np.random.default_rng(seed + 100).standard_normal(M).astype(np.float32) * 0.1) if bias else None
    return _layer(p, a, torch.from_numpy(R.CODE.copy()), M, K, "nf4", b)


def _fp4_layer(M, K, seed):
    rng = np.random.default_rng(seed)
    p, a = o.quantize_fp4((rng.standard_normal(M * K) * 0.05).astype(np.float32), 64)
    return _layer(torch.from_numpy(p).reshape(-1, 1), torch.from_numpy(a), torch.from_numpy(o.TREE_TABLE.copy()), M, K, "fp4", None)


def test_fused_nf4_linear_is_exported_and_carries_the_nf4_state(fx):
    assert pkg.FusedNF4Linear is fused_mod.FusedNF4Linear and "FusedNF4Linear" in pkg.__all__
    assert issubclass(pkg.FusedNF4Linear, pkg.FusedFP4Linear)
    p, a = _packed(32, 128, 1)
    layer = pkg.FusedNF4Linear.from_packed(p, a, (32, 128), 64)
    qs = layer.quant_data.quant_state
    assert qs.quant_type == "nf4" and layer.quant_data.nf4
    assert np.array_equal(qs.code.numpy().view(np.uint32), R.CODE.view(np.uint32))
    gu = pkg.FusedNF4Linear.gate_up_from_packed((p, a), _packed(32, 128, 2), (32, 128), 64)
    assert gu.epilogue == fused_mod.EPILOGUE_SILU_MUL_PAIRS and gu.out_features == 32 and gu.quant_data.M == 64 and gu.quant_data.nf4
    # each class refuses the other's code
    with pytest.raises(ValueError, match="NF4"):
        pkg.FusedFP4Linear(layer.quant_data)
    with pytest.raises(ValueError, match="NF4"):
        pkg.FusedFP4Linear.from_linear(types.SimpleNamespace(quant_data=layer.quant_data))
    with pytest.raises(ValueError, match="FP4"):
        pkg.FusedNF4Linear.from_linear(_fp4_layer(32, 128, 3))


def test_routing_by_row_count_and_the_fallback_after_a_refusal(fx):
    M, K = 32, 128
    g, u = _nf4_layer(M, K, 1), _nf4_layer(M, K, 2)
    gu = pkg.FusedNF4Linear.gate_up(g, u)
    plain = pkg.FusedNF4Linear.from_linear(g)
    t = lambda rows, dtype=torch.bfloat16: torch.randn(rows, K).to(dtype)
    for rows, want in ((1, ["gemv_nf4_fused"]), (2, ["gemm_nf4_fused"]), (24, ["gemm_nf4_fused"]), (64, ["gemm_nf4_fused"]),
                       (65, ["qlinear_nf4_bias"]), (200, ["qlinear_nf4_bias"])):
        for layer, width in ((gu, M), (plain, M)):
            fx.calls.clear()
            x = t(rows)
            y = layer(x)
            assert fx.calls == want, (rows, fx.calls)
            assert tuple(y.shape) == (rows, width)
    # values: the fused ops and the unfused sequence agree (bf16 rounding apart)
    x = t(3)
    r = torch.randn(3, M).to(torch.bfloat16)
    want = torch.nn.functional.silu(g(x)) * u(x) + r
    assert (gu(x, r).float() - want.float()).abs().max() <= 2.0**-6 * want.float().abs().max()
    x1 = t(1)
    want1 = g(x1) + r[:1]
    assert (plain(x1, r[:1]).float() - want1.float()).abs().max() <= 2.0**-6 * want1.float().abs().max()
    # 3-D single token -> the GEMV op; f32 rows > 1 and a non-matching dtype -> unfused
    fx.calls.clear()
    assert tuple(gu(t(1).view(1, 1, K)).shape) == (1, 1, M) and fx.calls == ["gemv_nf4_fused"]
    g32 = pkg.FusedNF4Linear.gate_up(_nf4_layer(M, K, 1), _nf4_layer(M, K, 2))
    fx.calls.clear()
    g32(t(4, torch.float32))
    assert fx.calls == ["qlinear_nf4_bias"]
    # the measured tie (profiles/nf4_fused_epilogues.json): plain epilogue, more than 32 rows, K >= 8192 - the op runs without the
    # residual and torch adds it; 32 rows, the gated epilogue and shorter rows keep the add in the kernel
    seen = []
    real = fx.gemm_nf4_fused
    fx.gemm_nf4_fused = lambda A, B, am, bs, shape, bias, res, epi: (seen.append(res is not None), real(A, B, am, bs, shape, bias, res, epi))[1]
    long_plain = pkg.FusedNF4Linear.from_linear(_nf4_layer(8, 8192, 4))
    for layer, rows, want_in_kernel in ((long_plain, 33, False), (long_plain, 64, False), (long_plain, 32, True), (plain, 64, True)):
        xr = torch.randn(rows, layer.in_features).to(torch.bfloat16)
        rr = torch.randn(rows, layer.out_features).to(torch.bfloat16)
        y = layer(xr, rr)
        assert seen[-1] is want_in_kernel and torch.equal(y, layer(xr) + rr), (rows, seen[-1])
    del fx.gemm_nf4_fused
    # a refusal clears the flag: the op is tried once, the unfused sequence answers from then on
    fx.refuse_gemv = "fp4_hip_gemv_fused_nf4: the fused epilogue is not available for M=64 K=128"
    fx.calls.clear()
    y = gu(x1)
    assert fx.calls == ["gemv_nf4_fused", "gemv_nf4_bias"] and tuple(y.shape) == (1, M) and not gu._fused_ok
    fx.calls.clear()
    gu(x1)
    assert fx.calls == ["gemv_nf4_bias"]
    fx.refuse_gemm = "fp4_hip_gemm_fused_nf4: B=4 M=64 K=128 blocksize=64 dtype=2 is not covered"
    fx.calls.clear()
    gu(t(4))
    gu(t(4))
    assert fx.calls == ["gemm_nf4_fused", "qlinear_nf4_bias", "qlinear_nf4_bias"] and not gu._small_ok
    # any other error is not swallowed
    fx.refuse_gemv = "hipErrorLaunchFailure"
    with pytest.raises(RuntimeError, match="LaunchFailure"):
        plain(x1)


def _mlp(gate, up, down):
    mlp = nn.Module()
    mlp.gate_proj, mlp.up_proj, mlp.down_proj, mlp.act_fn = gate, up, down, nn.SiLU()
    root = nn.Module()
    root.mlp = mlp
    return root


def test_fuse_gated_mlps_takes_nf4_only_on_request_and_never_a_mixed_pair(fx):
    H, I = 128, 64
    root = _mlp(_nf4_layer(I, H, 1), _nf4_layer(I, H, 2), _nf4_layer(H, I, 3))
    before = root.mlp
    assert pkg.fuse_gated_mlps(root) == 0 and root.mlp is before
    assert pkg.fuse_gated_mlps(root, nf4=True) == 1
    assert isinstance(root.mlp, pkg.FusedGatedMLP) and type(root.mlp.gate_up) is pkg.FusedNF4Linear
    fx.calls.clear()
    y = root.mlp(torch.randn(1, H).to(torch.bfloat16))
    assert tuple(y.shape) == (1, H) and fx.calls == ["gemv_nf4_fused", "gemv_nf4_bias"]
    for gate, up in ((_nf4_layer(I, H, 1), _fp4_layer(I, H, 2)), (_fp4_layer(I, H, 1), _nf4_layer(I, H, 2))):
        mixed = _mlp(gate, up, nn.Identity())
        keep = mixed.mlp
        assert pkg.fuse_gated_mlps(mixed) == 0 and pkg.fuse_gated_mlps(mixed, nf4=True) == 0 and mixed.mlp is keep
        with pytest.raises(ValueError):
            pkg.FusedGatedMLP(gate, up, nn.Identity())


def test_fused_nf4_mlp_saves_as_its_two_projections_and_loads_unfused(fx, tmp_path, monkeypatch):
    from safetensors.torch import load_file

    from torch_bnb_fp4 import serialization as ser_mod

    monkeypatch.setattr(ser_mod, "Params4bit", HostParams4bit)

    H, I = 128, 64
    gate, up, down = _nf4_layer(I, H, 1), _nf4_layer(I, H, 2), _nf4_layer(H, I, 3, bias=False)
    want = {n: (l.quant_data.A.clone(), l.quant_data.absmax.clone(), None if l.bias is None else l.bias.clone())
            for n, l in (("gate_proj", gate), ("up_proj", up), ("down_proj", down))}
    root = _mlp(gate, up, down)
    assert pkg.fuse_gated_mlps(root, nf4=True) == 1
    path = str(tmp_path / "nf4_fused.safetensors")
    pkg.save_fp4_model(root, path)
    state = load_file(path)
    for n in want:
        assert f"mlp.{n}.weight.quant_state.bitsandbytes__nf4" in state and f"mlp.{n}.weight.quant_state.bitsandbytes__fp4" not in state
    assert not any("gate_up" in k for k in state)
    fresh = _mlp(nn.Linear(H, I), nn.Linear(H, I), nn.Linear(I, H, bias=False))
    fresh = pkg.load_fp4_layers(fresh, path, device="cpu")
    for n, (p, a, b) in want.items():
        layer = getattr(fresh.mlp, n)
        assert isinstance(layer, pkg.TorchFP4Linear) and layer.quant_data.nf4
        assert torch.equal(layer.quant_data.A.reshape(-1), p.reshape(-1)) and torch.equal(layer.quant_data.absmax, a)
        assert (layer.bias is None) == (b is None) and (b is None or torch.equal(layer.bias.float(), b.float()))
    assert pkg.fuse_gated_mlps(fresh, nf4=True) == 1
    assert torch.equal(fresh.mlp.gate_up.qweight, root.mlp.gate_up.qweight) and torch.equal(fresh.mlp.gate_up.absmax, root.mlp.gate_up.absmax)
