"""LoRA adapters beside NF4 weights on the host (no GPU): the three C entry points' argument validation (every call below returns
before any HIP call), LoRANF4Linear's routing through a numpy-backed fake extension defined here, the padding / stacking /
interleaving of adapters against a numpy restatement, and attach_lora / load_lora_adapter's key mapping and scaling."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nf4_lora_cases as LC
import nf4_ref as R
import torch_bnb_fp4 as pkg
from oracle import fp4_oracle as o
from test_nf4_fused_host import FusedNf4Ext, _mlp, _nf4_layer, _fp4_layer
from torch_bnb_fp4 import functional as F_mod, fused as fused_mod, quant_data as qd_mod

NONE, GATED = 0, 1
OK, INVALID, UNSUPPORTED = 0, 1, 2
F16, F32, BF16 = 0, 1, 2


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entry_points():
    assert {"fp4_hip_lora_down", "fp4_hip_gemv_lora_nf4", "fp4_hip_gemm_lora_nf4"} <= set(hipabi.declared_symbols())
    assert LC.lib().fp4_hip_abi_version() == 7


def test_lora_down_argument_validation():
    l, d = LC.lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    down = lambda x, A, Bt, Rr, K, dt=BF16, scale=d, t=d: l.fp4_hip_lora_down(x, A, scale, t, Bt, Rr, K, dt, None)
    assert down(d, d, -1, 8, 64) == INVALID and down(d, d, 1, -8, 64) == INVALID and down(d, d, 1, 8, -64) == INVALID
    assert down(d, d, 1, 8, 64, 5) == UNSUPPORTED and "dtype" in err()
    for Rr in (0, 4, 12, 264, 512):
        assert down(d, d, 1, Rr, 64) == UNSUPPORTED and "not covered" in err(), Rr
    assert down(d, d, 65, 8, 64) == UNSUPPORTED and "not covered" in err()
    assert down(d, d, 1, 8, 36) == UNSUPPORTED  # K % 8 != 0
    assert down(d, d, 1, 8, 0) == UNSUPPORTED
    assert down(ctypes.c_void_p(0x1002), d, 1, 8, 64) == UNSUPPORTED and down(d, ctypes.c_void_p(0x1008), 1, 8, 64) == UNSUPPORTED
    assert down(None, None, 0, 8, 64, scale=None, t=None) == OK  # no rows: nothing to do
    assert down(None, d, 1, 8, 64) == INVALID and "null" in err()
    assert down(d, d, 1, 8, 64, scale=None) == INVALID and down(d, d, 1, 8, 64, t=None) == INVALID


def test_gemv_lora_nf4_argument_validation():
    l, d = LC.lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    gemv = lambda x, out, M, K, bs, dt, epi, Rr=8, B=d, t=d: l.fp4_hip_gemv_lora_nf4(x, d, d, None, None, B, t, Rr, out, M, K, bs, dt, epi, None)
    assert gemv(d, d, 64, 64, 64, BF16, 7) == INVALID and "unknown epilogue" in err()
    assert gemv(d, d, 63, 64, 64, BF16, GATED) == INVALID and "even row count" in err()
    assert gemv(d, d, -1, 64, 64, BF16, NONE) == INVALID and gemv(d, d, 64, 33, 64, BF16, NONE) == INVALID
    assert gemv(d, d, 64, 64, 64, BF16, NONE, Rr=-8) == INVALID
    assert gemv(d, d, 64, 64, 64, 5, NONE) == UNSUPPORTED and "dtype" in err()
    assert gemv(None, None, 0, 64, 64, BF16, NONE, B=None, t=None) == OK  # M == 0
    assert gemv(None, d, 64, 64, 64, BF16, NONE) == INVALID and "null" in err()
    assert gemv(d, d, 64, 64, 64, BF16, NONE, B=None) == INVALID and gemv(d, d, 64, 64, 64, BF16, NONE, t=None) == INVALID
    for epi in (NONE, GATED):
        # the coverage of fp4_hip_gemv_fused_nf4 ...
        assert gemv(d, d, 64, 48, 16, BF16, epi) == UNSUPPORTED and "not available" in err()          # K % 32 != 0
        assert gemv(d, d, 64, 64, 16, BF16, epi) == UNSUPPORTED and "not available" in err()          # blocksize 16
        assert gemv(d, d, 64, 96, 96, BF16, epi) == UNSUPPORTED
        assert gemv(ctypes.c_void_p(0x1002), d, 64, 64, 64, BF16, epi) == UNSUPPORTED
        # ... and the adapter's own
        for Rr in (0, 12, 264):
            assert gemv(d, d, 64, 64, 64, BF16, epi, Rr=Rr) == UNSUPPORTED and "not available" in err(), Rr
        assert gemv(d, d, 64, 64, 64, BF16, epi, B=ctypes.c_void_p(0x1008)) == UNSUPPORTED and "not available" in err()
        assert gemv(d, d, 64, 64, 64, BF16, epi, t=ctypes.c_void_p(0x1004)) == UNSUPPORTED
    assert gemv(d, d, 64, 64, 64, F32, GATED) == UNSUPPORTED and "not available" in err()


def test_gemm_lora_nf4_argument_validation():
    l, d = LC.lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    gemm = lambda x, out, B, M, K, bs, dt, epi, Rr=8, lb=d, t=d: l.fp4_hip_gemm_lora_nf4(x, d, d, None, None, lb, t, Rr, out, B, M, K, bs, dt, epi, None)
    assert gemm(d, d, 4, 64, 64, 64, BF16, 2) == INVALID and "unknown epilogue" in err()
    assert gemm(d, d, 4, 63, 64, 64, BF16, GATED) == INVALID and "even row count" in err()
    assert gemm(d, d, -1, 64, 64, 64, BF16, NONE) == INVALID and gemm(d, d, 4, 64, 0, 64, BF16, NONE) == INVALID
    assert gemm(d, d, 4, 64, 64, 64, BF16, NONE, Rr=-1) == INVALID
    for epi in (NONE, GATED):
        assert gemm(d, d, 65, 64, 64, 64, BF16, epi) == UNSUPPORTED and "not covered" in err()   # the adapter forms stop at 64 rows
        assert gemm(d, d, 4, 64, 64, 32, BF16, epi) == UNSUPPORTED and "not covered" in err()
        assert gemm(d, d, 4, 64, 96, 64, BF16, epi) == UNSUPPORTED
        assert gemm(d, d, 4, 64, 64, 64, F32, epi) == UNSUPPORTED
        assert gemm(ctypes.c_void_p(0x1008), d, 4, 64, 64, 64, F16, epi) == UNSUPPORTED
        for Rr in (0, 12, 264):
            assert gemm(d, d, 4, 64, 64, 64, BF16, epi, Rr=Rr) == UNSUPPORTED and "not available" in err(), Rr
        assert gemm(d, d, 4, 64, 512, 64, BF16, epi, lb=ctypes.c_void_p(0x1002)) == UNSUPPORTED
        assert gemm(None, None, 4, 0, 64, 64, BF16, epi, lb=None, t=None) == OK
        assert gemm(None, None, 0, 64, 64, 64, BF16, epi, lb=None, t=None) == OK
    assert gemm(None, d, 4, 64, 64, 64, BF16, NONE) == INVALID and "null" in err()
    assert gemm(d, d, 4, 64, 64, 64, BF16, NONE, lb=None) == INVALID and gemm(d, d, 4, 64, 512, 64, BF16, GATED, t=None) == INVALID


# ---- the fake extension ----------------------------------------------------------------------------------------------------------------
class LoraExt(FusedNf4Ext):
    """FusedNf4Ext plus the three LoRA ops, answered from the numpy restatement: t in f32, the adapter term joins the float64 sum
    before the oracle's epilogue."""

    refuse_down = refuse_gemv_lora = refuse_gemm_lora = None

    def lora_down(self, x, A, scale):
        self.calls.append("lora_down")
        if self.refuse_down:
            raise RuntimeError(self.refuse_down)
        assert x.is_contiguous() and A.dtype == x.dtype and scale.dtype == torch.float32 and A.shape[0] % 8 == 0
        return ((x.reshape(-1, A.shape[1]).double() @ A.double().t()) * scale.double()).float()

    def _lora(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue, lora_B, t, gemv):
        M, K = Bshape
        assert lora_B.dtype == A.dtype and tuple(lora_B.shape) == (M, t.shape[1]) and t.dtype == torch.float32 and t.shape[1] % 8 == 0
        name = {torch.float16: "float16", torch.bfloat16: "bfloat16", torch.float32: "float32"}[A.dtype]
        w = R.dequantize_f32(B.numpy().ravel(), absmax.numpy(), blocksize, M * K).reshape(M, K).astype(np.float64)
        y = A.float().numpy().reshape(-1, K).astype(np.float64) @ w.T + t.double().numpy() @ lora_B.double().numpy().T
        nb = None if bias is None else bias.float().numpy()
        nr = None if residual is None else residual.float().numpy().reshape(y.shape[0], -1)
        if not gemv and nb is not None:
            y, nb = y + nb.astype(np.float64), None
        if epilogue == 1:
            v = o.linear_epilogue(y, name, nb)
            v = o.silu_mul_epilogue(v[:, 0::2], v[:, 1::2], name, nr)
        else:
            v = o.linear_epilogue(y, name, nb, nr)
        return torch.from_numpy(np.asarray(v, np.float32)).to(A.dtype).view(*A.shape[:-1], -1)

    def gemv_nf4_lora(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue, lora_B, t):
        self.calls.append("gemv_nf4_lora")
        if self.refuse_gemv_lora:
            raise RuntimeError(self.refuse_gemv_lora)
        assert A.is_contiguous() and A.numel() == Bshape[1] and t.shape[0] == 1
        return self._lora(A, B, absmax, blocksize, Bshape, bias, residual, epilogue, lora_B, t, True)

    def gemm_nf4_lora(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue, lora_B, t):
        self.calls.append("gemm_nf4_lora")
        if self.refuse_gemm_lora:
            raise RuntimeError(self.refuse_gemm_lora)
        assert 1 <= A.numel() // Bshape[1] <= 64 and t.shape[0] == A.numel() // Bshape[1]
        return self._lora(A, B, absmax, blocksize, Bshape, bias, residual, epilogue, lora_B, t, False)


@pytest.fixture()
def fx(monkeypatch):
    r = LoraExt()
    for mod in (F_mod, qd_mod, fused_mod):
        monkeypatch.setattr(mod, "ext", r)
    monkeypatch.setattr(fused_mod, "nf4_code", lambda: torch.from_numpy(R.CODE.copy()))
    return r


def _adapter(M, K, r, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(r, K, generator=g) / math.sqrt(K)).to(dtype), (torch.randn(M, r, generator=g) * 0.05).to(dtype)


def _dense(layer):
    qd = layer.quant_data
    return torch.from_numpy(R.dequantize_f32(qd.A.numpy().ravel(), qd.absmax.numpy(), 64, qd.M * qd.N).reshape(qd.M, qd.N)).double()


# ---- the layer ---------------------------------------------------------------------------------------------------------------------------
def test_lora_layer_is_exported_and_pads_the_rank(fx):
    assert pkg.LoRANF4Linear is fused_mod.LoRANF4Linear and issubclass(pkg.LoRANF4Linear, pkg.FusedNF4Linear)
    assert {"LoRANF4Linear", "attach_lora", "load_lora_adapter"} <= set(pkg.__all__)
    M, K = 32, 128
    base = _nf4_layer(M, K, 1)
    for r, want in ((4, 8), (8, 8), (9, 16), (64, 64), (100, 104)):
        A, B = _adapter(M, K, r, r)
        layer = pkg.LoRANF4Linear.from_linear(base, A, B, 2.0)
        assert layer.rank == r and tuple(layer.lora_A.shape) == (want, K) and tuple(layer.lora_B.shape) == (M, want)
        # numpy restatement of the padding: zeros after the adapter's own rows / columns / factors, which are untouched
        nA, nB = np.zeros((want, K), np.float32), np.zeros((M, want), np.float32)
        nA[:r], nB[:, :r] = A.float().numpy(), B.float().numpy()
        assert np.array_equal(layer.lora_A.float().numpy(), nA) and np.array_equal(layer.lora_B.float().numpy(), nB)
        assert np.array_equal(layer.lora_scale.numpy(), np.r_[np.full(r, 2.0, np.float32), np.zeros(want - r, np.float32)])
        assert layer.lora_scale.dtype == torch.float32 and layer._lora_ok
    assert "lora_rank=100" in repr(layer)
    big = pkg.LoRANF4Linear.from_linear(base, *_adapter(M, K, 260, 5), 1.0)
    assert not big._lora_ok  # above the kernels' rank: the adapter runs in torch
    with pytest.raises(ValueError, match="adapter shapes"):
        pkg.LoRANF4Linear.from_linear(base, torch.zeros(8, K + 1), torch.zeros(M, 8), 1.0)
    with pytest.raises(ValueError, match="adapter shapes"):
        pkg.LoRANF4Linear.from_linear(base, torch.zeros(8, K), torch.zeros(M + 1, 8), 1.0)
    with pytest.raises(ValueError, match="FP4"):
        pkg.LoRANF4Linear.from_linear(_fp4_layer(M, K, 3), torch.zeros(8, K), torch.zeros(M, 8), 1.0)


def test_gate_up_stacks_and_interleaves_the_adapters(fx):
    M, K = 32, 128
    g, u = _nf4_layer(M, K, 1), _nf4_layer(M, K, 2)
    (Ag, Bg), (Au, Bu) = _adapter(M, K, 4, 1), _adapter(M, K, 6, 2)
    layer = pkg.LoRANF4Linear.gate_up(g, u, (Ag, Bg, 2.0), (Au, Bu, 0.5))
    assert layer.epilogue == GATED and layer.out_features == M and layer.rank == 10 and tuple(layer.lora_B.shape) == (2 * M, 16)
    nA = np.zeros((16, K), np.float32)
    nA[:4], nA[4:10] = Ag.float().numpy(), Au.float().numpy()
    nB = np.zeros((2 * M, 16), np.float32)
    nB[0::2, :4], nB[1::2, 4:10] = Bg.float().numpy(), Bu.float().numpy()  # row 2i = gate_i, row 2i + 1 = up_i, as the weight's
    ns = np.r_[np.full(4, 2.0), np.full(6, 0.5), np.zeros(6)].astype(np.float32)
    assert np.array_equal(layer.lora_A.float().numpy(), nA) and np.array_equal(layer.lora_B.float().numpy(), nB)
    assert np.array_equal(layer.lora_scale.numpy(), ns)
    # and the weight's rows are interleaved the same way
    assert torch.equal(layer.qweight.reshape(2 * M, K // 2)[0::2], g.quant_data.A.reshape(M, K // 2))
    with pytest.raises(ValueError, match="same"):
        pkg.LoRANF4Linear.gate_up(g, u, (Ag, Bg, 2.0), (Au[:, :64], Bu, 0.5))
    with pytest.raises(ValueError, match="gate\\|up"):
        pkg.LoRANF4Linear.gate_up_from_fused(pkg.FusedNF4Linear.from_linear(g), (Ag, Bg, 2.0), (Au, Bu, 0.5))


def test_routing_by_rows_dtype_and_shape(fx):
    M, K = 32, 128
    g, u = _nf4_layer(M, K, 1), _nf4_layer(M, K, 2)
    plain = pkg.LoRANF4Linear.from_linear(g, *_adapter(M, K, 8, 1), 2.0)
    gu = pkg.LoRANF4Linear.gate_up(g, u, (*_adapter(M, K, 4, 1), 2.0), (*_adapter(M, K, 4, 2), 2.0))
    t = lambda rows, dtype=torch.bfloat16: torch.randn(rows, K).to(dtype)
    for rows, want in ((1, ["lora_down", "gemv_nf4_lora"]), (2, ["lora_down", "gemm_nf4_lora"]), (40, ["lora_down", "gemm_nf4_lora"]),
                       (64, ["lora_down", "gemm_nf4_lora"])):
        for layer in (plain, gu):
            fx.calls.clear()
            assert tuple(layer(t(rows)).shape) == (rows, M) and fx.calls == want, (rows, fx.calls)
    # 65+ rows: the base through the parent's path, the adapter in torch
    fx.calls.clear()
    assert tuple(plain(t(65)).shape) == (65, M) and tuple(gu(t(65)).shape) == (65, M)
    assert fx.calls == ["qlinear_nf4_bias", "qlinear_nf4_bias"]
    # a 3-D single token is a GEMV; f32 with several rows is outside the matrix-core kernels
    fx.calls.clear()
    assert tuple(gu(t(1).view(1, 1, K)).shape) == (1, 1, M) and fx.calls == ["lora_down", "gemv_nf4_lora"]
    p32 = pkg.LoRANF4Linear.from_linear(_nf4_layer(M, K, 1), *_adapter(M, K, 8, 1, torch.float32), 2.0)
    fx.calls.clear()
    p32(t(1, torch.float32))
    p32(t(4, torch.float32))
    assert fx.calls == ["lora_down", "gemv_nf4_lora", "qlinear_nf4_bias"]
    # a rank above 256 never reaches the ops
    big = pkg.LoRANF4Linear.from_linear(g, *_adapter(M, K, 260, 5), 1.0)
    fx.calls.clear()
    big(t(1))
    assert fx.calls == ["gemv_nf4_fused"]


def test_cells_that_measured_behind_take_the_fallback(fx):
    """profiles/nf4_lora.json: one row always; 2..64 rows up to the largest M * rows * rank at which a rank band measured ahead."""
    ahead = fused_mod.lora_fused_ahead
    assert all(ahead(1, M, 4096, r) for M in (4096, 28672) for r in (8, 64, 256))
    assert all(ahead(rows, 28672, 4096, 16) for rows in (2, 32, 64)) and ahead(64, 14336, 4096, 32) and not ahead(64, 28672, 4096, 32)
    assert ahead(64, 4096, 4096, 64) and ahead(8, 28672, 4096, 64) and ahead(8, 14336, 4096, 128) and ahead(8, 4096, 4096, 256)
    for rows, M, r in ((32, 14336, 64), (64, 14336, 64), (32, 28672, 64), (64, 28672, 64), (8, 28672, 128), (32, 14336, 128), (8, 14336, 256),
                       (32, 4096, 256)):
        assert not ahead(rows, M, 4096, r), (rows, M, r)
    assert ahead(64, 4096, 14336, 256) and ahead(64, 4096, 14336, 64)
    M, K = 4160, 64
    layer = pkg.LoRANF4Linear.from_linear(_nf4_layer(M, K, 1), *_adapter(M, K, 64, 1), 2.0)
    for rows, want in ((1, ["lora_down", "gemv_nf4_lora"]), (32, ["lora_down", "gemm_nf4_lora"]), (64, ["gemm_nf4_fused"])):
        fx.calls.clear()
        assert tuple(layer(torch.randn(rows, K).to(torch.bfloat16)).shape) == (rows, M) and fx.calls == want, (rows, fx.calls)


def test_values_of_every_route_agree_with_float64(fx):
    """fused ops (fake: exact sum, one rounding chain) and the torch fallback against W x + B (s A x) in float64; bf16 rounding apart."""
    M, K = 32, 128
    g, u = _nf4_layer(M, K, 1), _nf4_layer(M, K, 2)
    A, B = _adapter(M, K, 5, 3)
    plain = pkg.LoRANF4Linear.from_linear(g, A, B, 2.0)
    (Ag, Bg), (Au, Bu) = _adapter(M, K, 4, 1), _adapter(M, K, 6, 2)
    gu = pkg.LoRANF4Linear.gate_up(g, u, (Ag, Bg, 2.0), (Au, Bu, 0.5))
    full = lambda layer, x, A_, B_, s: x.double() @ _dense(layer).t() + layer.bias.double() + (x.double() @ A_.double().t() * s) @ B_.double().t()
    for rows in (1, 3, 70):
        x = torch.randn(rows, K).to(torch.bfloat16)
        r = torch.randn(rows, M).to(torch.bfloat16)
        want = full(g, x, A, B, 2.0) + r.double()
        assert (plain(x, r).double() - want).abs().max() <= 2.0**-6 * want.abs().max(), rows
        gate, up = full(g, x, Ag, Bg, 2.0), full(u, x, Au, Bu, 0.5)
        want = torch.nn.functional.silu(gate) * up
        assert (gu(x).double() - want).abs().max() <= 2.0**-5 * want.abs().max() + 1e-3, rows


def test_refusals_flip_the_flags_and_the_fallback_answers(fx):
    M, K = 32, 128
    g = _nf4_layer(M, K, 1)
    layer = pkg.LoRANF4Linear.from_linear(g, *_adapter(M, K, 8, 1), 2.0)
    x1, x4 = torch.randn(1, K).to(torch.bfloat16), torch.randn(4, K).to(torch.bfloat16)
    fx.refuse_gemv_lora = "fp4_hip_gemv_lora_nf4: the fused epilogue is not available for M=32 K=128"
    fx.calls.clear()
    y = layer(x1)
    # the refused op, then the fallback: the parent's own fused op is the same kernel family and is not tried again either
    assert fx.calls == ["lora_down", "gemv_nf4_lora", "gemv_nf4_bias"] and not layer._fused_ok and tuple(y.shape) == (1, M)
    fx.calls.clear()
    layer(x1)
    assert fx.calls == ["gemv_nf4_bias"]
    fx.refuse_gemm_lora = "fp4_hip_gemm_lora_nf4: B=4 M=32 K=128 blocksize=64 dtype=2 is not covered"
    fx.calls.clear()
    layer(x4)
    layer(x4)
    assert fx.calls == ["lora_down", "gemm_nf4_lora", "qlinear_nf4_bias", "qlinear_nf4_bias"] and not layer._small_ok
    other = pkg.LoRANF4Linear.from_linear(g, *_adapter(M, K, 8, 1), 2.0)
    fx.refuse_down = "fp4_hip_lora_down: Bt=1 R=8 K=128 is not covered"
    fx.calls.clear()
    other(x1)
    other(x4)
    assert fx.calls == ["lora_down", "gemv_nf4_fused", "gemm_nf4_fused"] and not other._lora_ok and other._fused_ok
    fx.refuse_down = "hipErrorLaunchFailure"
    third = pkg.LoRANF4Linear.from_linear(g, *_adapter(M, K, 8, 1), 2.0)
    with pytest.raises(RuntimeError, match="LaunchFailure"):
        third(x1)


# ---- surgery -----------------------------------------------------------------------------------------------------------------------------
def _toy(H=128, I=64):
    """Two decoder-like blocks: self_attn.q_proj / o_proj and a gated MLP, all NF4."""
    root = nn.Module()
    root.model = nn.Module()
    root.model.layers = nn.ModuleList()
    for i in range(2):
        blk = nn.Module()
        blk.self_attn = nn.Module()
        blk.self_attn.q_proj, blk.self_attn.o_proj = _nf4_layer(H, H, 10 * i + 1), _nf4_layer(H, H, 10 * i + 2, bias=False)
        blk.mlp = _mlp(_nf4_layer(I, H, 10 * i + 3), _nf4_layer(I, H, 10 * i + 4), _nf4_layer(H, I, 10 * i + 5)).mlp
        root.model.layers.append(blk)
    return root


def _peft_state(shapes, r, seed=0, adapter_name=None, prefix="base_model.model."):
    g = torch.Generator().manual_seed(seed)
    mid = f".{adapter_name}" if adapter_name else ""
    state = {}
    for path, (M, K) in shapes.items():
        state[f"{prefix}{path}.lora_A{mid}.weight"] = torch.randn(r, K, generator=g) / math.sqrt(K)
        state[f"{prefix}{path}.lora_B{mid}.weight"] = torch.randn(M, r, generator=g) * 0.05
    return state


def test_attach_lora_maps_peft_keys_and_scales(fx):
    H, I, r = 128, 64, 4
    shapes = {}
    for i in range(2):
        p = f"model.layers.{i}."
        shapes.update({p + "self_attn.q_proj": (H, H), p + "self_attn.o_proj": (H, H), p + "mlp.gate_proj": (I, H), p + "mlp.up_proj": (I, H),
                       p + "mlp.down_proj": (H, I)})
    for name, rslora, want_s in ((None, False, 16 / 4), ("default", True, 16 / 2.0)):
        root = _toy(H, I)
        assert pkg.fuse_gated_mlps(root, nf4=True) == 2
        state = _peft_state(shapes, r, adapter_name=name)
        assert pkg.attach_lora(root, state, r=r, lora_alpha=16, use_rslora=rslora) == 8  # 2 x (q, o, gate|up, down)
        blk = root.model.layers[1]
        q = blk.self_attn.q_proj
        mid = f".{name}" if name else ""
        assert type(q) is pkg.LoRANF4Linear and q.rank == r and tuple(q.lora_A.shape) == (8, H)
        assert torch.equal(q.lora_A[:r], state[f"base_model.model.model.layers.1.self_attn.q_proj.lora_A{mid}.weight"])
        assert np.array_equal(q.lora_scale.numpy(), np.r_[np.full(r, want_s), np.zeros(8 - r)].astype(np.float32))
        gu = blk.mlp.gate_up
        assert type(gu) is pkg.LoRANF4Linear and gu.rank == 2 * r and gu.epilogue == GATED and type(blk.mlp.down_proj) is pkg.LoRANF4Linear
        assert torch.equal(gu.lora_B[1::2, r:2 * r], state[f"base_model.model.model.layers.1.mlp.up_proj.lora_B{mid}.weight"])
        assert float(gu.lora_B[0::2, r:].abs().max()) == 0.0 and float(gu.lora_B[1::2, :r].abs().max()) == 0.0
        y = root.model.layers[0].mlp(torch.randn(1, H).to(torch.bfloat16))
        assert tuple(y.shape) == (1, H) and fx.calls[-4:] == ["lora_down", "gemv_nf4_lora", "lora_down", "gemv_nf4_lora"]
    # keys without the peft prefix, an unfused model, target_modules, and a gate adapter alone (the up half is zero)
    root = _toy(H, I)
    state = _peft_state({"model.layers.0.mlp.gate_proj": (I, H), "model.layers.0.self_attn.q_proj": (H, H)}, r, prefix="")
    assert pkg.attach_lora(root, state, r, 8, target_modules=["gate_proj"]) == 1
    assert type(root.model.layers[0].mlp.gate_proj) is pkg.LoRANF4Linear and type(root.model.layers[0].self_attn.q_proj) is pkg.TorchFP4Linear
    root = _toy(H, I)
    pkg.fuse_gated_mlps(root, nf4=True)
    assert pkg.attach_lora(root, _peft_state({"model.layers.0.mlp.gate_proj": (I, H)}, r), r, 8) == 1
    gu = root.model.layers[0].mlp.gate_up
    assert gu.rank == 2 * r and float(gu.lora_B[1::2].abs().max()) == 0.0 and float(gu.lora_B[0::2, :r].abs().max()) > 0


def test_attach_lora_refuses_keys_without_an_nf4_home(fx):
    H, I, r = 128, 64, 4
    root = _toy(H, I)
    with pytest.raises(KeyError, match="no such module"):
        pkg.attach_lora(root, _peft_state({"model.layers.7.self_attn.q_proj": (H, H)}, r), r, 8)
    root.model.layers[0].self_attn.k_proj = nn.Linear(H, H)
    with pytest.raises(ValueError, match="not an NF4 layer"):
        pkg.attach_lora(root, _peft_state({"model.layers.0.self_attn.k_proj": (H, H)}, r), r, 8)
    root.model.layers[0].self_attn.v_proj = _fp4_layer(H, H, 9)
    with pytest.raises(ValueError, match="not an NF4 layer"):
        pkg.attach_lora(root, _peft_state({"model.layers.0.self_attn.v_proj": (H, H)}, r), r, 8)
    with pytest.raises(KeyError, match="not a LoRA adapter key"):
        pkg.attach_lora(root, {"base_model.model.model.layers.0.self_attn.q_proj.weight": torch.zeros(H, H)}, r, 8)
    with pytest.raises(KeyError, match="lacks lora_B"):
        pkg.attach_lora(root, {"model.layers.0.self_attn.q_proj.lora_A.weight": torch.zeros(r, H)}, r, 8)
    with pytest.raises(ValueError, match="rank"):
        pkg.attach_lora(root, _peft_state({"model.layers.0.self_attn.q_proj": (H, H)}, r), 2 * r, 8)
    # nothing was replaced by the failed calls above, and an adapter is attached once
    assert type(root.model.layers[0].self_attn.q_proj) is pkg.TorchFP4Linear
    state = _peft_state({"model.layers.0.self_attn.q_proj": (H, H)}, r)
    assert pkg.attach_lora(root, state, r, 8) == 1
    with pytest.raises(ValueError, match="not an NF4 layer"):
        pkg.attach_lora(root, state, r, 8)
    # a state whose last key has no home raises before anything is replaced, the fused MLP's layer included
    root = _toy(H, I)
    pkg.fuse_gated_mlps(root, nf4=True)
    shapes = {"model.layers.0.self_attn.o_proj": (H, H), "model.layers.0.mlp.up_proj": (I, H), "model.layers.7.self_attn.q_proj": (H, H)}
    with pytest.raises(KeyError, match="no such module"):
        pkg.attach_lora(root, _peft_state(shapes, r), r, 8)
    assert type(root.model.layers[0].self_attn.o_proj) is pkg.TorchFP4Linear and type(root.model.layers[0].mlp.gate_up) is pkg.FusedNF4Linear


def test_load_lora_adapter_reads_a_peft_directory(fx, tmp_path):
    from safetensors.torch import save_file

    H, I, r = 128, 64, 4
    root = _toy(H, I)
    state = _peft_state({"model.layers.1.self_attn.o_proj": (H, H), "model.layers.1.mlp.down_proj": (H, I),
                         "model.layers.0.self_attn.q_proj": (H, H)}, r)
    save_file(state, str(tmp_path / "adapter_model.safetensors"))
    (tmp_path / "adapter_config.json").write_text(json.dumps({"r": r, "lora_alpha": 6, "use_rslora": True, "peft_type": "LORA",
                                                               "target_modules": ["o_proj", "down_proj"], "lora_dropout": 0.05}))
    assert pkg.load_lora_adapter(root, str(tmp_path)) == 2
    o_proj = root.model.layers[1].self_attn.o_proj
    assert type(o_proj) is pkg.LoRANF4Linear and type(root.model.layers[0].self_attn.q_proj) is pkg.TorchFP4Linear
    assert float(o_proj.lora_scale[0]) == pytest.approx(6 / math.sqrt(r)) and not hasattr(o_proj, "dropout")
    assert torch.equal(o_proj.lora_B[:, :r], state["base_model.model.model.layers.1.self_attn.o_proj.lora_B.weight"])
