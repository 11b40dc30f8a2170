"""Several LoRA adapters per batch on the host (no GPU): the three C entry points' declarations and argument validation (every call
below returns before any HIP call), the stacking / padding / interleaving of adapters against a numpy restatement,
AdapterSelection's in-place writes, MultiLoRANF4Linear's routing, refusals and flags through a numpy-backed fake extension defined
here, and attach_lora_adapters / load_lora_adapters' key mapping."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nf4_multi_lora_cases as MC
import nf4_ref as R
import torch_bnb_fp4 as pkg
from test_nf4_fused_host import _nf4_layer, _fp4_layer
from test_nf4_lora_host import LoraExt, _adapter, _dense, _peft_state, _toy
from torch_bnb_fp4 import functional as F_mod, fused as fused_mod, quant_data as qd_mod

NONE, GATED = 0, 1
OK, INVALID, UNSUPPORTED = 0, 1, 2
F16, F32, BF16 = 0, 1, 2


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entry_points_under_abi_7():
    assert {"fp4_hip_lora_down_multi", "fp4_hip_gemm_lora_multi_nf4", "fp4_hip_gemv_lora_multi_nf4"} <= set(hipabi.declared_symbols())
    assert MC.lib().fp4_hip_abi_version() == 7
    header = open(hipabi.HEADER).read()
    assert "#define FP4_HIP_ABI_VERSION 7" in header


def test_id_patterns_cover_what_the_kernels_branch_on():
    for rows in MC.ROWS:
        pats = MC.id_patterns(rows)
        assert all(len(p) == rows for p in pats.values())
        assert len(set(pats["equal"])) == 1 and pats["sorted"] == sorted(pats["sorted"])
        if rows >= 9:
            assert set(pats["sorted"]) == set(range(MC.N_ADAPTERS))
            every = pats["every_row"]
            assert all(every[b] != every[b + 1] for b in range(rows - 1))  # crosses every 4-row group, 8-row workgroup, 16-column tile
            assert set(MC.NO_ADAPTER) <= set(pats["with_none"]) and any(MC.valid(i) for i in pats["with_none"])


def test_lora_down_multi_argument_validation():
    l, d = MC.lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    down = lambda x, A, Bt, Rr, K, dt=BF16, scale=d, t=d, ids=d, n=3: l.fp4_hip_lora_down_multi(x, A, scale, ids, t, Bt, n, Rr, K, dt, None)
    assert down(d, d, -1, 8, 64) == INVALID and down(d, d, 1, -8, 64) == INVALID and down(d, d, 1, 8, -64) == INVALID
    assert down(d, d, 1, 8, 64, n=0) == INVALID and "n_adapters" in err()
    assert down(d, d, 1, 8, 64, n=-2) == INVALID
    assert down(d, d, 1, 8, 64, ids=None) == INVALID and "ids" in err()
    assert down(d, d, 1, 8, 64, 5) == UNSUPPORTED and "dtype" in err()
    for Rr in (0, 4, 12, 264, 512):
        assert down(d, d, 1, Rr, 64) == UNSUPPORTED and "not covered" in err(), Rr
    assert down(d, d, 65, 8, 64) == UNSUPPORTED and "not covered" in err()
    assert down(d, d, 1, 8, 36) == UNSUPPORTED and down(d, d, 1, 8, 0) == UNSUPPORTED
    assert down(ctypes.c_void_p(0x1002), d, 1, 8, 64) == UNSUPPORTED and down(d, ctypes.c_void_p(0x1002), 1, 8, 64) == UNSUPPORTED
    assert down(None, None, 0, 8, 64, scale=None, t=None) == OK  # no rows: nothing to do
    assert down(None, d, 1, 8, 64) == INVALID and "null" in err()
    assert down(d, d, 1, 8, 64, scale=None) == INVALID and down(d, d, 1, 8, 64, t=None) == INVALID


def test_gemv_and_gemm_lora_multi_argument_validation():
    l, d = MC.lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    gemv = lambda x, out, M, K, bs, dt, epi, Rr=8, B=d, t=d, ids=d, n=3: l.fp4_hip_gemv_lora_multi_nf4(x, d, d, None, None, B, ids, n, t, Rr, out,
                                                                                                      M, K, bs, dt, epi, None)
    gemm = lambda x, out, M, K, bs, dt, epi, Rr=8, B=d, t=d, ids=d, n=3, rows=4: l.fp4_hip_gemm_lora_multi_nf4(x, d, d, None, None, B, ids, n, t,
                                                                                                              Rr, out, rows, M, K, bs, dt, epi, None)
    for call in (gemv, gemm):
        assert call(d, d, 64, 64, 64, BF16, 7) == INVALID and "unknown epilogue" in err()
        assert call(d, d, 63, 64, 64, BF16, GATED) == INVALID and "even row count" in err()
        assert call(d, d, -1, 64, 64, BF16, NONE) == INVALID
        assert call(d, d, 64, 64, 64, BF16, NONE, Rr=-8) == INVALID
        assert call(d, d, 64, 64, 64, BF16, NONE, n=0) == INVALID and "n_adapters" in err()
        assert call(d, d, 64, 64, 64, BF16, NONE, ids=None) == INVALID and "ids" in err()
        assert call(None, d, 64, 64, 64, BF16, NONE) == INVALID and "null" in err()
        assert call(d, d, 64, 64, 64, BF16, NONE, B=None) == INVALID and call(d, d, 64, 64, 64, BF16, NONE, t=None) == INVALID
        for epi in (NONE, GATED):
            for Rr in (0, 12, 264):
                assert call(d, d, 64, 64, 64, BF16, epi, Rr=Rr) == UNSUPPORTED and "not available" in err(), Rr
            assert call(d, d, 64, 64, 64, BF16, epi, B=ctypes.c_void_p(0x1002)) == UNSUPPORTED and "not available" in err()
            assert call(d, d, 64, 64, 64, BF16, epi, t=ctypes.c_void_p(0x1004)) == UNSUPPORTED
            assert call(ctypes.c_void_p(0x1002), d, 64, 64, 64, BF16, epi) == UNSUPPORTED
        assert call(d, d, 64, 64, 64, F32, GATED) == UNSUPPORTED
    assert gemv(d, d, 64, 48, 16, BF16, NONE) == UNSUPPORTED and "not available" in err()      # the coverage of fp4_hip_gemv_fused_nf4
    assert gemv(None, None, 0, 64, 64, BF16, NONE, B=None, t=None) == OK
    assert gemm(d, d, 64, 64, 64, BF16, NONE, rows=65) == UNSUPPORTED and "not covered" in err()  # the coverage of fp4_hip_gemm_lora_nf4
    assert gemm(d, d, 64, 96, 64, BF16, NONE) == UNSUPPORTED and gemm(d, d, 64, 64, 32, BF16, NONE) == UNSUPPORTED
    assert gemm(d, d, 64, 64, 64, F32, NONE) == UNSUPPORTED
    assert gemm(None, None, 64, 64, 64, BF16, NONE, B=None, t=None, rows=0) == OK


# ---- the selection -------------------------------------------------------------------------------------------------------------------
def test_adapter_selection_is_written_in_place():
    sel = pkg.AdapterSelection(names=["a", "b", "c"])
    assert sel.capacity == 64 and len(sel) == 0 and sel.ids.numel() == 0 and sel.ids.dtype == torch.int32
    sel.set([0] * 64)
    ptr = sel.ids.data_ptr()
    for ids in ([2, -1, 0], torch.tensor([1, 1, 2, 0, -1]), torch.tensor([0, 5], dtype=torch.int64), list(range(-3, 61))):
        assert sel.set(ids) is sel
        want = [int(i) for i in ids]
        assert sel.ids.data_ptr() == ptr and len(sel) == len(want) and sel.ids.tolist() == want and sel.ids.is_contiguous()
    held = sel.ids
    sel.set([7] * 64)
    assert held.tolist() == [7] * 64  # a view taken earlier sees the rewrite: what a captured graph relies on
    with pytest.raises(ValueError, match="at most 64"):
        sel.set([0] * 65)
    with pytest.raises(TypeError, match="integers"):
        sel.set(torch.tensor([0.5]))
    assert sel.ids.data_ptr() == ptr and len(sel) == 64
    sel.set_by_name(["c", None, "a"])
    assert sel.ids.tolist() == [2, -1, 0]
    with pytest.raises(KeyError, match="no adapter named"):
        sel.set_by_name(["d"])
    assert pkg.AdapterSelection(capacity=128).set([1] * 70).ids.numel() == 70


# ---- the fake extension ----------------------------------------------------------------------------------------------------------------
class MultiLoraExt(LoraExt):
    """LoraExt plus the three multi-adapter ops, answered row by row from LoraExt's single-adapter restatement."""

    refuse_down_multi = refuse_gemv_multi = refuse_gemm_multi = None

    def lora_down_multi(self, x, A_stack, scale_stack, ids):
        self.calls.append("lora_down_multi")
        if self.refuse_down_multi:
            raise RuntimeError(self.refuse_down_multi)
        n, Rr, K = A_stack.shape
        xs = x.reshape(-1, K)
        assert x.is_contiguous() and A_stack.dtype == x.dtype and tuple(scale_stack.shape) == (n, Rr) and Rr % 8 == 0
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.numel() >= xs.shape[0]
        t = torch.zeros(xs.shape[0], Rr)
        for b, i in enumerate(ids.tolist()[: xs.shape[0]]):
            if 0 <= i < n:
                t[b] = ((xs[b].double() @ A_stack[i].double().t()) * scale_stack[i].double()).float()
        return t

    def _multi(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue, B_stack, ids, t, gemv):
        M, K = Bshape
        n = B_stack.shape[0]
        rows = A.numel() // K
        assert tuple(B_stack.shape[1:]) == (M, t.shape[1]) and ids.dtype == torch.int32 and ids.numel() >= rows and t.shape[0] == rows
        xs = A.reshape(rows, K)
        out = []
        for b, i in enumerate(ids.tolist()[:rows]):
            lB = B_stack[i] if 0 <= i < n else torch.zeros_like(B_stack[0])
            r = None if residual is None else residual.reshape(rows, -1)[b:b + 1]
            out.append(self._lora(xs[b:b + 1], B, absmax, blocksize, Bshape, bias, r, epilogue, lB, t[b:b + 1], gemv))
        return torch.cat(out).view(*A.shape[:-1], -1)

    def gemv_nf4_lora_multi(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue, B_stack, ids, t):
        self.calls.append("gemv_nf4_lora_multi")
        if self.refuse_gemv_multi:
            raise RuntimeError(self.refuse_gemv_multi)
        assert A.is_contiguous() and A.numel() == Bshape[1]
        return self._multi(A, B, absmax, blocksize, Bshape, bias, residual, epilogue, B_stack, ids, t, True)

    def gemm_nf4_lora_multi(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue, B_stack, ids, t):
        self.calls.append("gemm_nf4_lora_multi")
        if self.refuse_gemm_multi:
            raise RuntimeError(self.refuse_gemm_multi)
        assert 1 <= A.numel() // Bshape[1] <= 64
        return self._multi(A, B, absmax, blocksize, Bshape, bias, residual, epilogue, B_stack, ids, t, False)


@pytest.fixture()
def fx(monkeypatch):
    r = MultiLoraExt()
    for mod in (F_mod, qd_mod, fused_mod):
        monkeypatch.setattr(mod, "ext", r)
    monkeypatch.setattr(fused_mod, "nf4_code", lambda: torch.from_numpy(R.CODE.copy()))
    return r


def _layer(M, K, ranks, sel, seed=1, scales=None):
    base = _nf4_layer(M, K, seed)
    ads = [(*_adapter(M, K, r, 10 * seed + j), (scales or [2.0] * len(ranks))[j]) for j, r in enumerate(ranks)]
    return base, ads, pkg.MultiLoRANF4Linear.from_linear(base, ads, sel)


# ---- the layer ---------------------------------------------------------------------------------------------------------------------------
def test_layer_is_exported_and_stacks_the_adapters_at_one_common_rank(fx):
    assert pkg.MultiLoRANF4Linear is fused_mod.MultiLoRANF4Linear and issubclass(pkg.MultiLoRANF4Linear, pkg.FusedNF4Linear)
    assert {"AdapterSelection", "MultiLoRANF4Linear", "attach_lora_adapters", "load_lora_adapters"} <= set(pkg.__all__)
    M, K = 32, 128
    sel = pkg.AdapterSelection()
    for ranks, want in (((4, 8, 24), 24), ((4,), 8), ((9, 3), 16), ((64, 100), 104)):
        _, ads, layer = _layer(M, K, ranks, sel, scales=[2.0, 0.5, 1.5][: len(ranks)])
        n = len(ranks)
        assert layer.rank == want and layer.ranks == list(ranks) and layer.n_adapters == n and layer._lora_ok and layer.selection is sel
        assert tuple(layer.lora_A_stack.shape) == (n, want, K) and tuple(layer.lora_B_stack.shape) == (n, M, want)
        assert tuple(layer.lora_scale_stack.shape) == (n, want) and layer.lora_scale_stack.dtype == torch.float32
        # numpy restatement: each adapter's own rows / columns / factors untouched, zeros after them
        nA, nB, ns = np.zeros((n, want, K), np.float32), np.zeros((n, M, want), np.float32), np.zeros((n, want), np.float32)
        for j, (A, B, s) in enumerate(ads):
            r = A.shape[0]
            nA[j, :r], nB[j, :, :r], ns[j, :r] = A.float().numpy(), B.float().numpy(), s
        assert np.array_equal(layer.lora_A_stack.float().numpy(), nA) and np.array_equal(layer.lora_B_stack.float().numpy(), nB)
        assert np.array_equal(layer.lora_scale_stack.numpy(), ns)
        assert layer.lora_A_stack.is_contiguous() and layer.lora_B_stack.is_contiguous()
    assert "common_rank=104" in repr(layer)
    _, _, big = _layer(M, K, (8, 260), sel)
    assert big.rank == 264 and not big._lora_ok  # above the kernels' rank: the adapters run in torch
    base = _nf4_layer(M, K, 1)
    with pytest.raises(ValueError, match="adapter shapes"):
        pkg.MultiLoRANF4Linear.from_linear(base, [(torch.zeros(8, K + 1), torch.zeros(M, 8), 1.0)], sel)
    with pytest.raises(ValueError, match="at least one adapter"):
        pkg.MultiLoRANF4Linear.from_linear(base, [], sel)
    with pytest.raises(TypeError, match="AdapterSelection"):
        pkg.MultiLoRANF4Linear.from_linear(base, [(torch.zeros(8, K), torch.zeros(M, 8), 1.0)], torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="FP4"):
        pkg.MultiLoRANF4Linear.from_linear(_fp4_layer(M, K, 3), [(torch.zeros(8, K), torch.zeros(M, 8), 1.0)], sel)
    with pytest.raises(TypeError, match="needs adapters"):
        pkg.MultiLoRANF4Linear.from_packed()


def test_gate_up_stacks_and_interleaves_every_adapter(fx):
    M, K = 32, 128
    g, u = _nf4_layer(M, K, 1), _nf4_layer(M, K, 2)
    sel = pkg.AdapterSelection()
    pairs = [((*_adapter(M, K, 4, 1), 2.0), (*_adapter(M, K, 6, 2), 0.5)), ((*_adapter(M, K, 2, 3), 1.0), (*_adapter(M, K, 1, 4), 3.0))]
    layer = pkg.MultiLoRANF4Linear.gate_up_from_fused(pkg.FusedNF4Linear.gate_up(g, u), pairs, sel)
    assert layer.epilogue == GATED and layer.out_features == M and layer.rank == 16 and layer.ranks == [10, 3]
    nA, nB, ns = np.zeros((2, 16, K), np.float32), np.zeros((2, 2 * M, 16), np.float32), np.zeros((2, 16), np.float32)
    for j, ((Ag, Bg, sg), (Au, Bu, su)) in enumerate(pairs):
        rg, ru = Ag.shape[0], Au.shape[0]
        nA[j, :rg], nA[j, rg:rg + ru] = Ag.float().numpy(), Au.float().numpy()
        nB[j, 0::2, :rg], nB[j, 1::2, rg:rg + ru] = Bg.float().numpy(), Bu.float().numpy()  # row 2i = gate_i, row 2i + 1 = up_i
        ns[j, :rg], ns[j, rg:rg + ru] = sg, su
    assert np.array_equal(layer.lora_A_stack.float().numpy(), nA) and np.array_equal(layer.lora_B_stack.float().numpy(), nB)
    assert np.array_equal(layer.lora_scale_stack.numpy(), ns)
    with pytest.raises(ValueError, match="gate\\|up"):
        pkg.MultiLoRANF4Linear.gate_up_from_fused(pkg.FusedNF4Linear.from_linear(g), pairs, sel)


def test_routing_by_rows_dtype_and_shape(fx):
    M, K = 32, 128
    sel = pkg.AdapterSelection(capacity=128)
    _, _, plain = _layer(M, K, (8, 4, 16), sel)
    g, u = _nf4_layer(M, K, 1), _nf4_layer(M, K, 2)
    pairs = [((*_adapter(M, K, 4, 1), 2.0), (*_adapter(M, K, 4, 2), 2.0))] * 2
    gu = pkg.MultiLoRANF4Linear.gate_up_from_fused(pkg.FusedNF4Linear.gate_up(g, u), pairs, sel)
    t = lambda rows, dtype=torch.bfloat16: torch.randn(rows, K).to(dtype)
    for rows, want in ((1, ["lora_down_multi", "gemv_nf4_lora_multi"]), (2, ["lora_down_multi", "gemm_nf4_lora_multi"]),
                       (40, ["lora_down_multi", "gemm_nf4_lora_multi"]), (64, ["lora_down_multi", "gemm_nf4_lora_multi"])):
        sel.set([b % 4 - 1 for b in range(rows)])
        for layer in (plain, gu):
            fx.calls.clear()
            assert tuple(layer(t(rows)).shape) == (rows, M) and fx.calls == want, (rows, fx.calls)
    # 65+ rows: the base through the parent's path, the adapters in torch
    sel.set([b % 3 for b in range(65)])
    fx.calls.clear()
    assert tuple(plain(t(65)).shape) == (65, M) and tuple(gu(t(65)).shape) == (65, M)
    assert fx.calls == ["qlinear_nf4_bias", "qlinear_nf4_bias"]
    # a 3-D single token is a GEMV; f32 with several rows is outside the matrix-core kernels
    sel.set([1])
    fx.calls.clear()
    assert tuple(gu(t(1).view(1, 1, K)).shape) == (1, 1, M) and fx.calls == ["lora_down_multi", "gemv_nf4_lora_multi"]
    p32 = pkg.MultiLoRANF4Linear.from_linear(_nf4_layer(M, K, 1), [(*_adapter(M, K, 8, 1, torch.float32), 2.0)], sel)
    fx.calls.clear()
    p32(t(1, torch.float32))
    sel.set([0, -1, 0, 0])
    p32(t(4, torch.float32))
    assert fx.calls == ["lora_down_multi", "gemv_nf4_lora_multi", "qlinear_nf4_bias"]
    # a common rank above 256 never reaches the ops; the number of ids must be the number of rows
    _, _, big = _layer(M, K, (8, 260), sel)
    sel.set([1])
    fx.calls.clear()
    big(t(1))
    assert fx.calls == ["gemv_nf4_fused"]
    with pytest.raises(ValueError, match="one id per row"):
        plain(t(2))
    # the cells lora_fused_ahead leaves to the fallback are left to it here as well (profiles/nf4_lora.json)
    Mw, Kw = 4160, 64
    _, _, wide = _layer(Mw, Kw, (64,), sel)
    for rows, want in ((1, ["lora_down_multi", "gemv_nf4_lora_multi"]), (32, ["lora_down_multi", "gemm_nf4_lora_multi"]), (64, ["gemm_nf4_fused"])):
        sel.set([0] * rows)
        fx.calls.clear()
        assert tuple(wide(torch.randn(rows, Kw).to(torch.bfloat16)).shape) == (rows, Mw) and fx.calls == want, (rows, fx.calls)


def test_values_of_every_route_agree_with_float64_row_by_row(fx):
    """fused ops (fake: exact sum, one rounding chain) and the torch fallback against W x + B_a (s_a A_a x) in float64 with a = the
    row's adapter, and W x alone where the id names none; bf16 rounding apart.  Casts follow the activation dtype, once per dtype."""
    M, K = 32, 128
    sel = pkg.AdapterSelection(capacity=128)
    base, ads, layer = _layer(M, K, (5, 8, 3), sel, scales=[2.0, 0.5, 1.5])
    for rows in (1, 3, 40, 70):
        ids = [(1, -1, 0, 2, 3, -7, 2**31 - 1)[b % 7] for b in range(rows)]
        sel.set(ids)
        x = torch.randn(rows, K).to(torch.bfloat16)
        r = torch.randn(rows, M).to(torch.bfloat16)
        want = x.double() @ _dense(base).t() + base.bias.double() + r.double()
        for b, i in enumerate(ids):
            if 0 <= i < 3:
                A, B, s = ads[i]
                want[b] += (x[b].double() @ A.double().t() * s) @ B.double().t()
        got = layer(x, r)
        assert got.shape == (rows, M) and (got.double() - want).abs().max() <= 2.0**-6 * want.abs().max(), rows
    # adapters saved in float32 under bf16 activations: the stacks are cast once and kept, the buffers stay as attached
    f32 = pkg.MultiLoRANF4Linear.from_linear(_nf4_layer(M, K, 1), [(A.float(), B.float(), s) for A, B, s in ads], sel)
    sel.set([0, 1])
    x = torch.randn(2, K).to(torch.bfloat16)
    y = f32(x)
    cast = f32._cast[torch.bfloat16]
    assert torch.equal(f32(x), y) and torch.equal(y, layer(x))
    assert f32._cast[torch.bfloat16] is cast and cast[0].dtype == torch.bfloat16 and f32.lora_A_stack.dtype == torch.float32


def test_refusals_flip_the_flags_and_the_fallback_answers(fx):
    M, K = 32, 128
    sel = pkg.AdapterSelection()
    _, _, layer = _layer(M, K, (8, 8), sel)
    x1, x4 = torch.randn(1, K).to(torch.bfloat16), torch.randn(4, K).to(torch.bfloat16)
    fx.refuse_gemv_multi = "fp4_hip_gemv_lora_multi_nf4: the fused epilogue is not available for M=32 K=128"
    sel.set([1])
    fx.calls.clear()
    y = layer(x1)
    assert fx.calls == ["lora_down_multi", "gemv_nf4_lora_multi", "gemv_nf4_bias"] and not layer._fused_ok and tuple(y.shape) == (1, M)
    fx.calls.clear()
    layer(x1)
    assert fx.calls == ["gemv_nf4_bias"]
    fx.refuse_gemm_multi = "fp4_hip_gemm_lora_multi_nf4: B=4 M=32 K=128 blocksize=64 dtype=2 is not covered"
    sel.set([0, 1, -1, 0])
    fx.calls.clear()
    layer(x4)
    layer(x4)
    assert fx.calls == ["lora_down_multi", "gemm_nf4_lora_multi", "qlinear_nf4_bias", "qlinear_nf4_bias"] and not layer._small_ok
    _, _, other = _layer(M, K, (8, 8), sel)
    fx.refuse_down_multi = "fp4_hip_lora_down_multi: Bt=1 R=8 K=128 n_adapters=2 is not covered"
    fx.calls.clear()
    sel.set([1])
    other(x1)
    sel.set([0, 1, -1, 0])
    other(x4)
    assert fx.calls == ["lora_down_multi", "gemv_nf4_fused", "gemm_nf4_fused"] and not other._lora_ok and other._fused_ok
    fx.refuse_down_multi = "hipErrorLaunchFailure"
    _, _, third = _layer(M, K, (8, 8), sel)
    with pytest.raises(RuntimeError, match="LaunchFailure"):
        third(x4)


# ---- surgery -----------------------------------------------------------------------------------------------------------------------------
def _shapes(H, I, skip=()):
    shapes = {}
    for i in range(2):
        p = f"model.layers.{i}."
        shapes.update({p + "self_attn.q_proj": (H, H), p + "self_attn.o_proj": (H, H), p + "mlp.gate_proj": (I, H), p + "mlp.up_proj": (I, H),
                       p + "mlp.down_proj": (H, I)})
    return {k: v for k, v in shapes.items() if k not in skip}


def test_attach_lora_adapters_maps_keys_for_several_adapters(fx):
    H, I = 128, 64
    root = _toy(H, I)
    assert pkg.fuse_gated_mlps(root, nf4=True) == 2
    sa = _peft_state(_shapes(H, I), 4, seed=1)
    sb = _peft_state(_shapes(H, I, skip=("model.layers.1.self_attn.o_proj", "model.layers.1.mlp.up_proj")), 8, seed=2, adapter_name="default")
    sc = _peft_state({"model.layers.1.self_attn.o_proj": (H, H)}, 2, seed=3, prefix="")
    sel = pkg.attach_lora_adapters(root, {"a": (sa, 4, 16, False), "b": (sb, 8, 16, True), "c": (sc, 2, 2, False)})
    assert isinstance(sel, pkg.AdapterSelection) and sel.names == ["a", "b", "c"] and sel.n_layers == 8  # 2 x (q, o, gate|up, down)
    blk = root.model.layers[1]
    q, o_proj, gu = blk.self_attn.q_proj, blk.self_attn.o_proj, blk.mlp.gate_up
    assert all(type(m) is pkg.MultiLoRANF4Linear and m.selection is sel and m.n_adapters == 3 for m in (q, o_proj, gu, blk.mlp.down_proj))
    assert q.rank == 8 and q.ranks == [4, 8, 1] and torch.equal(q.lora_A_stack[0, :4], sa["base_model.model.model.layers.1.self_attn.q_proj.lora_A.weight"])
    assert torch.equal(q.lora_B_stack[1], sb["base_model.model.model.layers.1.self_attn.q_proj.lora_B.default.weight"])
    assert np.array_equal(q.lora_scale_stack.numpy(), np.array([[4.0] * 4 + [0.0] * 4, [16 / math.sqrt(8)] * 8, [0.0] * 8], np.float32))
    # an adapter that lacks a target module gets a zero slice there
    assert float(q.lora_A_stack[2].abs().max()) == 0.0 and float(q.lora_B_stack[2].abs().max()) == 0.0
    assert float(o_proj.lora_B_stack[1].abs().max()) == 0.0 and float(o_proj.lora_B_stack[2].abs().max()) > 0
    assert torch.equal(o_proj.lora_A_stack[2, :2], sc["model.layers.1.self_attn.o_proj.lora_A.weight"])
    # gate|up: adapter b has a gate part only in block 1 (its up half is zero), adapter c none
    assert gu.epilogue == GATED and gu.ranks == [8, 9, 2] and gu.rank == 16
    assert torch.equal(gu.lora_B_stack[1, 0::2, :8], sb["base_model.model.model.layers.1.mlp.gate_proj.lora_B.default.weight"])
    assert float(gu.lora_B_stack[1, 1::2].abs().max()) == 0.0 and float(gu.lora_B_stack[2].abs().max()) == 0.0
    assert torch.equal(gu.lora_B_stack[0, 1::2, 4:8], sa["base_model.model.model.layers.1.mlp.up_proj.lora_B.weight"])
    sel.set_by_name(["b", None, "a"])
    fx.calls.clear()
    y = root.model.layers[0].mlp(torch.randn(3, H).to(torch.bfloat16))
    assert tuple(y.shape) == (3, H) and fx.calls == ["lora_down_multi", "gemm_nf4_lora_multi"] * 2
    # target_modules restricts every adapter; an unfused model keeps its separate projections
    root = _toy(H, I)
    sel = pkg.attach_lora_adapters(root, {"a": (sa, 4, 16, False), "b": (sb, 8, 16, True)}, target_modules=["gate_proj"])
    assert sel.n_layers == 2 and type(root.model.layers[0].mlp.gate_proj) is pkg.MultiLoRANF4Linear
    assert type(root.model.layers[0].self_attn.q_proj) is pkg.TorchFP4Linear


def test_attach_lora_adapters_refuses_keys_without_an_nf4_home(fx):
    H, I, r = 128, 64, 4
    root = _toy(H, I)
    pkg.fuse_gated_mlps(root, nf4=True)
    good = _peft_state(_shapes(H, I), r, seed=1)
    with pytest.raises(KeyError, match="no such module"):
        pkg.attach_lora_adapters(root, {"a": (good, r, 8, False), "b": (_peft_state({"model.layers.7.self_attn.q_proj": (H, H)}, r), r, 8, False)})
    root.model.layers[0].self_attn.k_proj = nn.Linear(H, H)
    with pytest.raises(ValueError, match="not an NF4 layer"):
        pkg.attach_lora_adapters(root, {"a": (good, r, 8, False), "b": (_peft_state({"model.layers.0.self_attn.k_proj": (H, H)}, r), r, 8, False)})
    with pytest.raises(KeyError, match="not a LoRA adapter key"):
        pkg.attach_lora_adapters(root, {"a": ({"base_model.model.model.layers.0.self_attn.q_proj.weight": torch.zeros(H, H)}, r, 8, False)})
    with pytest.raises(ValueError, match="rank"):
        pkg.attach_lora_adapters(root, {"a": (good, 2 * r, 8, False)})
    with pytest.raises(ValueError, match="at least one adapter"):
        pkg.attach_lora_adapters(root, {})
    # nothing was replaced by the failed calls above, the fused MLP's layer included; and adapters are attached once
    assert type(root.model.layers[0].self_attn.q_proj) is pkg.TorchFP4Linear and type(root.model.layers[0].mlp.gate_up) is pkg.FusedNF4Linear
    assert pkg.attach_lora_adapters(root, {"a": (good, r, 8, False)}).n_layers == 8
    with pytest.raises(ValueError, match="not an NF4 layer|already carries"):
        pkg.attach_lora_adapters(root, {"a": (good, r, 8, False)})


def test_load_lora_adapters_reads_peft_directories(fx, tmp_path):
    from safetensors.torch import save_file

    H, I = 128, 64
    root = _toy(H, I)
    states = {"first": (_peft_state(_shapes(H, I), 4, seed=1), {"r": 4, "lora_alpha": 6, "use_rslora": True, "target_modules": ["o_proj", "down_proj"]}),
              "second": (_peft_state({"model.layers.1.self_attn.o_proj": (H, H), "model.layers.0.self_attn.q_proj": (H, H)}, 8, seed=2),
                         {"r": 8, "lora_alpha": 4, "target_modules": ["o_proj"]})}
    dirs = []
    for name, (state, cfg) in states.items():
        d = tmp_path / name
        d.mkdir()
        save_file(state, str(d / "adapter_model.safetensors"))
        (d / "adapter_config.json").write_text(json.dumps({**cfg, "peft_type": "LORA", "lora_dropout": 0.05}))
        dirs.append(str(d))
    sel = pkg.load_lora_adapters(root, dirs)
    assert sel.names == ["first", "second"] and sel.n_layers == 4  # o_proj and down_proj of both blocks
    o_proj = root.model.layers[1].self_attn.o_proj
    assert type(o_proj) is pkg.MultiLoRANF4Linear and type(root.model.layers[0].self_attn.q_proj) is pkg.TorchFP4Linear
    assert float(o_proj.lora_scale_stack[0, 0]) == pytest.approx(6 / math.sqrt(4)) and float(o_proj.lora_scale_stack[1, 0]) == pytest.approx(0.5)
    assert torch.equal(o_proj.lora_B_stack[1], states["second"][0]["base_model.model.model.layers.1.self_attn.o_proj.lora_B.weight"])
    assert float(root.model.layers[0].self_attn.o_proj.lora_B_stack[1].abs().max()) == 0.0  # "second" has no block-0 o_proj
    root2 = _toy(H, I)
    assert pkg.load_lora_adapters(root2, {"x": dirs[1], "y": dirs[0]}).names == ["x", "y"]
