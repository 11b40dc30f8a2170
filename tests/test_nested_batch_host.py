"""Double-quantised absmax in the 1..64-row kernels and beside an adapter, on the host (no GPU): the three declarations and exports
under ABI 7, their argument validation through ctypes (every call below returns before any HIP call), that the GPU suite's case lists
reach every dispatcher cell, and the routing of NestedNF4Linear / LoRANestedNF4Linear, attach_lora, fuse_gated_mlps and the saver
through a fake extension that records which op was called."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nested_batch_cases as NB
import nested_ref as N
import nf4_fused_cases as FC
import torch_bnb_fp4 as pkg
from test_nested_host import HostParams4bit, NestedExt, _nested_state, fx  # noqa: F401  (fx is a fixture)
from torch_bnb_fp4 import fused as fused_mod, nested as nested_mod, nn as nn_mod, serialization as ser_mod

OK, INVALID, UNSUPPORTED = 0, 1, 2
F16, F32, BF16 = 0, 1, 2
NEW = ["fp4_hip_gemm_nested_nf4", "fp4_hip_gemm_lora_nested_nf4", "fp4_hip_gemv_lora_nested_nf4"]


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entry_points_under_abi_7_and_the_library_exports_them():
    assert set(NEW) <= set(hipabi.declared_symbols())
    l = NB.lib()
    assert l.fp4_hip_abi_version() == 7
    header = open(hipabi.HEADER).read()
    assert int(header.split("#define FP4_HIP_ABI_VERSION")[1].split()[0]) == 7
    for name in NEW:
        assert getattr(l, name) is not None
    for op in ("gemm_nf4_nested", "gemm_nf4_lora_nested", "gemv_nf4_lora_nested"):
        assert callable(getattr(pkg.ext, op))


def _calls():
    l, d = NB.lib(), ctypes.c_void_p(0x1000)

    def gemm(x=d, P=d, q=d, nested=d, code=d, g=256, out=d, B=8, M=64, K=512, bs=64, dt=BF16, epi=0):
        return l.fp4_hip_gemm_nested_nf4(x, P, q, nested, code, 0.25, g, None, None, out, B, M, K, bs, dt, epi, None)

    def gemm_lora(x=d, P=d, q=d, nested=d, code=d, g=256, lB=d, t=d, R=8, out=d, B=8, M=64, K=512, bs=64, dt=BF16, epi=0):
        return l.fp4_hip_gemm_lora_nested_nf4(x, P, q, nested, code, 0.25, g, None, None, lB, t, R, out, B, M, K, bs, dt, epi, None)

    def gemv_lora(x=d, P=d, q=d, nested=d, code=d, g=256, lB=d, t=d, R=8, out=d, M=64, K=512, bs=64, dt=BF16, epi=0):
        return l.fp4_hip_gemv_lora_nested_nf4(x, P, q, nested, code, 0.25, g, None, None, lB, t, R, out, M, K, bs, dt, epi, None)

    return l, gemm, gemm_lora, gemv_lora


def test_argument_validation_of_the_three_entry_points():
    l, gemm, gemm_lora, gemv_lora = _calls()
    err = lambda: l.fp4_hip_last_error().decode()
    twins = {gemm: "fp4_hip_gemm_fused_nf4", gemm_lora: "fp4_hip_gemm_lora_nf4", gemv_lora: "fp4_hip_gemv_lora_nf4"}
    for call, twin in twins.items():
        assert call(epi=7) == INVALID and "unknown epilogue" in err()
        assert call(M=63, epi=1) == INVALID and "even row count" in err()
        for g in (0, -256):
            assert call(g=g) == INVALID and "nested_blocksize" in err()
        for g in (64, 128, 512, 4096, 100):  # only groups of 256 are read; the message names the expand route
            assert call(g=g) == UNSUPPORTED
            assert "nested_blocksize" in err() and "fp4_hip_absmax_unnest" in err() and twin in err()
        for null in ("x", "P", "q", "nested", "code", "out"):
            assert call(**{null: None}) == INVALID and "null" in err(), null
        assert call(M=0, x=None, P=None, q=None, nested=None, code=None, out=None) == OK  # nothing to do, whatever the pointers
        assert call(dt=5) == UNSUPPORTED
        assert call(x=ctypes.c_void_p(0x1002)) == UNSUPPORTED  # x not 16-byte aligned
    for call in (gemm_lora, gemv_lora):
        assert call(lB=None) == INVALID and call(t=None) == INVALID
        assert call(R=12) == UNSUPPORTED and call(R=264) == UNSUPPORTED and call(R=-8) == INVALID
    # the matrix-core kernels' own rules
    for call in (gemm, gemm_lora):
        assert call(B=0, x=None, out=None) == OK
        assert call(bs=32) == UNSUPPORTED and "not covered" in err()
        assert call(K=96) == UNSUPPORTED and "not covered" in err()
        assert call(dt=F32) == UNSUPPORTED and "not covered" in err()
        assert call(K=0) == INVALID and call(B=-1) == INVALID
    assert gemm(B=129) == UNSUPPORTED and "not covered" in err()
    assert gemm_lora(B=65) == UNSUPPORTED and "not covered" in err()
    # the GEMV's: its fast path, and the gated epilogue in 16 bits only
    assert gemv_lora(K=48, bs=16) == UNSUPPORTED and "not available" in err()
    assert gemv_lora(dt=F32, epi=1) == UNSUPPORTED
    assert gemv_lora(K=33) == INVALID


# ---- the case lists reach every dispatcher cell ---------------------------------------------------------------------------------------
def test_the_gpu_cases_reach_every_cell_of_both_dispatchers():
    small = {NB.small_cell(rows, M, K) for K in NB.SMALL_K for rows in NB.SMALL_ROWS for M in NB.SMALL_M + NB.SMALL_M_GATED}
    assert small == NB.ALL_SMALL_CELLS
    assert {NB.small_cell(r, 16, 2048)[1] for r in (2, 4)} == {4} and {NB.small_cell(r, 16, 2048)[1] for r in (5, 8)} == {8}
    assert {NB.small_cell(r, 16, 2048)[1] for r in (9, 16)} == {0}
    assert [NB.small_cell(2, 16, K)[0] for K in NB.SMALL_K] == [4, 2, 1]
    wide = {NB.wide_cell(rows, K, v) for K in NB.WIDE_K for rows in NB.WIDE_ROWS for v in (1, 2)}
    assert wide == NB.WC.ALL_CELLS
    assert all(K % 512 != 0 and K % 64 == 0 for K in NB.WIDE_K)  # so that one row stays in the wide kernel
    assert NB.WIDE_M < 6144 and NB.WIDE_M % 32 != 0 and NB.WIDE_M > 32  # RT 2 through the hook; a second workgroup that is a tail
    for rows, M, K in NB.CHUNKED:
        assert len(NB.WC.chunks(rows)) == 2 and NB.WC.cells(rows, M, K) != ["small"]
    # group geometry: blocks per row, groups per row, whether the block count is a multiple of 256
    geo = {(rows, M, K): (K // 64, M * K // 64) for rows, M, K, _ in NB.GEOMETRY}
    assert geo[(17, 17, 32768)] == (512, 17 * 512) and geo[(2, 17, 32768)][0] == 2 * 256
    assert geo[(8, 33, 1536)] == (24, 792) and 792 % 256 != 0 and 256 % 24 != 0  # a boundary mid-row, inside a 16-row tile (384 blocks)
    assert geo[(17, 64, 320)] == (5, 320) and 256 % 5 != 0
    assert geo[(3, 16, 512)] == (8, 128)
    assert any(o < 0 for o in NB.OFFSETS) and 0.0 in NB.OFFSETS and any(o > 0 for o in NB.OFFSETS)
    # LoRA: both kernels, both padded ranks
    assert {NB.WC.cells(rows, M, K)[0] == "small" for rows in NB.LORA_ROWS for M, K in NB.LORA_SHAPES} == {True, False}
    assert NB.LORA_RANKS == [8, 24] and len(FC.GEMV_VARIANT_SHAPES) == 4


# ---- routing through a fake extension -------------------------------------------------------------------------------------------------
class RouteExt(NestedExt):
    """Records the op each forward reaches and answers with zeros of the right shape; `refuse` makes the named ops answer
    "not covered"."""

    def __init__(self, real):
        super().__init__(real)
        self.refuse = set()

    def _answer(self, name, A, Bshape, residual=None):
        self.calls.append((name, A.numel() // A.shape[-1], residual is not None))
        if name in self.refuse:
            raise RuntimeError(f"{name}: B=.. is not covered (..)")
        return torch.zeros(A.shape[:-1] + (Bshape[0],), dtype=A.dtype)

    def qlinear_nf4_nested(self, A, B, q, nested, code, offset, g, M, K, bs, bias):
        return self._answer("qlinear_nf4_nested", A, [M, K])

    def gemv_nf4_nested(self, A, B, q, nested, code, offset, g, bs, Bshape, bias, residual, epi):
        return self._answer("gemv_nf4_nested", A, Bshape, residual)

    def gemm_nf4_nested(self, A, B, q, nested, code, offset, g, bs, Bshape, bias, residual, epi):
        assert q.dtype == torch.uint8 and isinstance(offset, float) and g == 256 and epi == 0
        return self._answer("gemm_nf4_nested", A, Bshape, residual)

    def lora_down(self, x, A, scale):
        self.calls.append(("lora_down", x.numel() // x.shape[-1], False))
        if "lora_down" in self.refuse:
            raise RuntimeError("lora_down: R=.. is not covered")
        return torch.zeros(x.numel() // x.shape[-1], A.shape[0])

    def gemv_nf4_lora_nested(self, A, B, q, nested, code, offset, g, bs, Bshape, bias, residual, epi, lB, t):
        assert lB.shape == (Bshape[0], t.shape[1]) and t.dtype == torch.float32
        return self._answer("gemv_nf4_lora_nested", A, Bshape, residual)

    def gemm_nf4_lora_nested(self, A, B, q, nested, code, offset, g, bs, Bshape, bias, residual, epi, lB, t):
        assert lB.shape == (Bshape[0], t.shape[1]) and t.shape[0] == A.numel() // A.shape[-1]
        return self._answer("gemm_nf4_lora_nested", A, Bshape, residual)


@pytest.fixture()
def route(monkeypatch):
    fake = RouteExt(nested_mod.ext)
    for mod in (nested_mod, nn_mod, fused_mod):
        monkeypatch.setattr(mod, "ext", fake)
    monkeypatch.setattr(ser_mod, "Params4bit", HostParams4bit)
    return fake


def _layer(M=48, K=512, bias=True, seed=0):
    state, _, meta = _nested_state("nf4", M, K, bias=bias, seed=seed)
    return pkg.NestedNF4Linear(state["l.weight"], state["l.weight.absmax"], state["l.weight.nested_absmax"], state["l.weight.nested_quant_map"],
                               meta["nested_offset"], (M, K), 64, state.get("l.bias"), torch.bfloat16)


def test_nested_linear_routing(route):
    layer = _layer()
    x = lambda rows, dtype=torch.bfloat16: torch.zeros(rows, 512, dtype=dtype)
    r = lambda rows: torch.zeros(rows, 48, dtype=torch.bfloat16)
    # default: off, every batched call expands as before
    for rows in (2, 16, 24, 64, 65):
        layer(x(rows))
    assert [c[0] for c in route.calls] == ["qlinear_nf4_nested"] * 5
    # the two switches, as on an expanded layer: nf4 -> 2..16 rows where K % 512 == 0; nf4_wide -> 17..64 (and 2..16 where K % 512 != 0)
    root = nn.Sequential(layer)
    assert pkg.set_small_batch_fused(root, True) == 0 and not layer.small_batch_fused_nf4
    assert pkg.set_small_batch_fused(root, True, nf4=True) == 1 and layer.small_batch_fused_nf4 and not layer.wide_batch_fused_nf4
    route.calls.clear()
    for rows in (1, 2, 16, 17, 64):
        layer(x(rows), r(rows))
    assert route.calls == [("gemv_nf4_nested", 1, True), ("gemm_nf4_nested", 2, True), ("gemm_nf4_nested", 16, True),
                           ("qlinear_nf4_nested", 17, False), ("qlinear_nf4_nested", 64, False)]
    assert pkg.set_small_batch_fused(root, True, nf4_wide=True) == 1 and layer.wide_batch_fused_nf4
    route.calls.clear()
    for rows in (2, 17, 64, 65):
        layer(x(rows), r(rows))
    layer(x(8, torch.float32))  # not a 16-bit dtype: the expand path
    layer(x(8))
    assert route.calls == [("gemm_nf4_nested", 2, True), ("gemm_nf4_nested", 17, True), ("gemm_nf4_nested", 64, True),
                           ("qlinear_nf4_nested", 65, False), ("qlinear_nf4_nested", 8, False), ("gemm_nf4_nested", 8, False)]
    # K % 512 != 0: the small switch alone routes nothing, the wide one every row count
    other = _layer(32, 320, bias=False)
    other.small_batch_fused_nf4 = True
    route.calls.clear()
    other(torch.zeros(4, 320, dtype=torch.float16))
    other.wide_batch_fused_nf4 = True
    other(torch.zeros(4, 320, dtype=torch.float16))
    assert [c[0] for c in route.calls] == ["qlinear_nf4_nested", "gemm_nf4_nested"]
    # the one cell FusedNF4Linear excludes from the fused residual add: more than 32 rows against rows of 8192 and more weights
    assert layer._residual_in_kernel(64, 4096) and layer._residual_in_kernel(32, 8192) and not layer._residual_in_kernel(33, 8192)
    for rows, K in ((64, 4096), (32, 8192), (33, 8192), (64, 14336)):
        fused = pkg.FusedNF4Linear.__new__(pkg.FusedNF4Linear)
        fused.epilogue = 0
        assert layer._residual_in_kernel(rows, K) == pkg.FusedNF4Linear._residual_in_kernel(fused, rows, K)
    # "not covered" clears the flag: not tried again
    route.refuse.add("gemm_nf4_nested")
    route.calls.clear()
    layer(x(8))
    layer(x(8))
    assert [c[0] for c in route.calls] == ["gemm_nf4_nested", "qlinear_nf4_nested", "qlinear_nf4_nested"] and not layer._batched_ok
    # off again
    assert pkg.set_small_batch_fused(root, False, nf4=True, nf4_wide=True) == 1
    assert not layer.small_batch_fused_nf4 and not layer.wide_batch_fused_nf4


def _adapter(M, K, r, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, K, generator=g) / K**0.5, torch.randn(M, r, generator=g) * 0.05


def test_lora_nested_linear_routing(route):
    A, B = _adapter(48, 512, 4)
    layer = pkg.LoRANestedNF4Linear.from_nested(_layer(), A, B, 2.0)
    assert isinstance(layer, pkg.NestedNF4Linear) and layer.rank == 4 and layer.lora_A.shape == (8, 512) and layer.lora_B.shape == (48, 8)
    assert bool((layer.lora_A[4:] == 0).all()) and bool((layer.lora_B[:, 4:] == 0).all()) and layer.lora_scale.tolist() == [2.0] * 4 + [0.0] * 4
    x = lambda rows: torch.zeros(rows, 512, dtype=torch.bfloat16)
    r = lambda rows: torch.zeros(rows, 48, dtype=torch.bfloat16)
    for rows in (1, 2, 64):
        y = layer(x(rows), r(rows))
        assert y.shape == (rows, 48) and y.dtype == torch.bfloat16
    assert route.calls == [("lora_down", 1, False), ("gemv_nf4_lora_nested", 1, True), ("lora_down", 2, False), ("gemm_nf4_lora_nested", 2, True),
                           ("lora_down", 64, False), ("gemm_nf4_lora_nested", 64, True)]
    # the adapter follows the activation dtype
    layer(torch.zeros(2, 512, dtype=torch.float16))
    assert layer._cast[torch.float16][0].dtype == torch.float16
    # over 64 rows: the layer's own path (here the expand path) and the adapter in torch
    route.calls.clear()
    layer(x(65))
    assert route.calls == [("qlinear_nf4_nested", 65, False)]
    # where lora_fused_ahead says no, the base runs through the layer's own path - the nested batched op once the switch is on
    big = pkg.LoRANestedNF4Linear.from_nested(_layer(), *_adapter(48, 512, 4), 2.0)
    big.wide_batch_fused_nf4 = big.small_batch_fused_nf4 = True
    import torch_bnb_fp4.fused as fz
    real = fz.lora_fused_ahead
    try:
        fz.lora_fused_ahead = lambda rows, M, K, rank: rows == 1
        route.calls.clear()
        big(x(8), r(8))
        big(x(1))
        assert route.calls == [("gemm_nf4_nested", 8, False), ("lora_down", 1, False), ("gemv_nf4_lora_nested", 1, False)]
    finally:
        fz.lora_fused_ahead = real
    # a refusal clears the flag of the op that refused
    route.refuse.add("gemm_nf4_lora_nested")
    route.calls.clear()
    layer(x(8))
    layer(x(8))
    layer(x(1))
    assert [c[0] for c in route.calls] == ["lora_down", "gemm_nf4_lora_nested", "qlinear_nf4_nested", "qlinear_nf4_nested", "lora_down",
                                           "gemv_nf4_lora_nested"]
    assert not layer._gemm_lora_ok and layer._gemv_lora_ok
    # ranks above 256 never reach the ops
    wide = pkg.LoRANestedNF4Linear.from_nested(_layer(), *_adapter(48, 512, 260), 1.0)
    route.calls.clear()
    wide(x(1))
    assert [c[0] for c in route.calls] == ["gemv_nf4_nested"] and not wide._lora_ok
    with pytest.raises(ValueError, match="adapter shapes"):
        pkg.LoRANestedNF4Linear.from_nested(_layer(), A, B[:40], 2.0)


class _MLP(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = nn.Linear(H, I, bias=False), nn.Linear(H, I, bias=False), nn.Linear(I, H)
        self.act_fn = nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


def _resident_mlp(H=512, I=64):
    mlp = _MLP(H, I)
    mlp.gate_proj, mlp.up_proj, mlp.down_proj = _layer(I, H, False, 1), _layer(I, H, False, 2), _layer(H, I, True, 3)
    root = nn.Module()
    root.mlp = mlp
    return root


def test_attach_lora_recognises_resident_targets_and_fuse_gated_mlps_ignores_them(route):
    H, I, r = 512, 64, 8
    root = _resident_mlp(H, I)
    assert pkg.fuse_gated_mlps(root, nf4=True) == 0
    adapter = {}
    for name, (M, K) in (("mlp.gate_proj", (I, H)), ("mlp.up_proj", (I, H)), ("mlp.down_proj", (H, I))):
        adapter[f"base_model.model.{name}.lora_A.weight"], adapter[f"base_model.model.{name}.lora_B.weight"] = _adapter(M, K, r, len(name))
    assert pkg.attach_lora(root, adapter, r=r, lora_alpha=16, target_modules=["gate_proj", "down_proj"]) == 2
    assert type(root.mlp.gate_proj) is pkg.LoRANestedNF4Linear and type(root.mlp.up_proj) is pkg.NestedNF4Linear
    assert type(root.mlp.down_proj) is pkg.LoRANestedNF4Linear and root.mlp.down_proj.lora_scale.tolist() == [2.0] * 8
    assert root.mlp.down_proj.absmax_u8.dtype == torch.uint8 and root.mlp.down_proj.bias is not None
    assert pkg.fuse_gated_mlps(root, nf4=True) == 0
    with pytest.raises(ValueError, match="attached once"):  # an adapter is attached once
        pkg.attach_lora(root, adapter, r=r, lora_alpha=16, target_modules=["gate_proj"])
    assert pkg.set_small_batch_fused(root, True, nf4=True, nf4_wide=True) == 3
    # several adapters at once stay expand-first
    with pytest.raises(ValueError, match="not an NF4 layer"):
        pkg.attach_lora_adapters(_resident_mlp(H, I), {"a": (adapter, r, 16, False)})
    # expand_nested keeps the adapter
    pkg.expand_nested(root)
    assert type(root.mlp.gate_proj) is pkg.LoRANF4Linear and type(root.mlp.up_proj) is pkg.TorchFP4Linear
    assert root.mlp.gate_proj.lora_A.shape == (8, H) and root.mlp.gate_proj.lora_scale.tolist() == [2.0] * 8


def test_saving_writes_the_resident_base_of_an_adapter_layer_verbatim(fx, tmp_path):
    from safetensors.torch import load_file

    state, want, meta = _nested_state("nf4", bias=True)
    root = nn.Module()
    base = pkg.fp4_linear_from_bnb_state(state, "l.", device="cpu", nested="resident")
    root.l = pkg.LoRANestedNF4Linear.from_nested(base, *_adapter(48, 512, 8), 2.0)
    path = str(tmp_path / "nested.safetensors")
    pkg.save_fp4_model(root, path, nested=True)
    back = load_file(path)
    assert set(back) == set(state) and all(torch.equal(back[k], state[k]) for k in state if "quant_state" not in k)
    assert "absmax_nest" not in fx.calls  # verbatim: nothing is re-quantised; the adapter is not part of the checkpoint
    assert {"LoRANestedNF4Linear"} <= set(pkg.__all__)
