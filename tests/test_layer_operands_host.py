"""The host twin of tests/test_gpu_layer_operands.py (no GPU): the same sweep over the same presentations, with the CPU doubles in
STRICT mode (tests/fake_ext.Strict), in which an op refuses what its C entry point refuses - a 16-bit activation off a 16-byte
boundary, a block size it does not cover - in the words recorded in tests/golden/*_entry_refusals.json.  Assertion 1 (no exception),
assertion 4 (no lasting effect) and the routes of the block-size cases are checked here; values and graph capture need the kernels.

A double that accepts any address cannot see this seam at all: first the strict mode itself is held to the recorded refusals."""
import json
import os

import numpy as np
import pytest
import torch

import layer_operand_cases as L
import nf4_ref as R
import torch_bnb_fp4 as pkg
from fake_ext import STRICT_RULES, FakeExt, Strict, strict_refusal
from oracle import fp4_oracle as o
from test_nested_batch_host import RouteExt, _layer as nested_layer
from test_nested_host import HostParams4bit
from test_nf4_fused_host import _nf4_layer, _packed
from test_nf4_lora_host import _adapter
from test_nf4_multi_lora_host import MultiLoraExt
from test_nf4_small_batch_host import _nf4_qd
from test_nf4_wide_batch_host import RecordingWideExt
from torch_bnb_fp4 import functional as F_mod, fused as fused_mod, nested as nested_mod, nn as nn_mod, quant_data as qd_mod, serialization as ser_mod

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT16 = [BF16, F16]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CPU = torch.device("cpu")


def install(monkeypatch, double, also=(F_mod,)):
    """The recording proxy over the strict double where activations are routed; the strict double itself in the modules of ``also``."""
    strict = Strict(double)
    for mod in also:
        monkeypatch.setattr(mod, "ext", strict)
    monkeypatch.setattr(ser_mod, "Params4bit", HostParams4bit)
    monkeypatch.setattr(fused_mod, "nf4_code", lambda: torch.from_numpy(R.CODE.copy()))
    monkeypatch.setattr(fused_mod, "fp4_code", lambda: torch.from_numpy(o.TREE_TABLE.copy()))
    return L.install(monkeypatch, strict)


def run(rec, name, dtype, build, K, M_out, rows, residual=False, before=None):
    records, failures = L.sweep(rec, build(), build(), K, M_out, rows, dtype, CPU, residual=residual, before=before, name=name)
    assert not failures, "\n".join(failures)
    return records


# ---- the strict mode itself ------------------------------------------------------------------------------------------------------------
def off16(n, dtype=BF16):
    return torch.zeros(n + 8, dtype=dtype)[1:1 + n]


def test_strict_mode_speaks_the_recorded_refusals():
    fp4, nf4 = (json.load(open(os.path.join(GOLDEN, f"{w}_entry_refusals.json"))) for w in ("fp4", "nf4"))
    d = torch.zeros(1)
    # the recorded call itself gives the recorded text, character for character
    assert strict_refusal("gemm_small_fp4", (off16(4 * 512).view(4, 512), d, d, 64, [64, 512], None)) == fp4["fp4_hip_gemm_small"]["4 rows: misaligned x"][1]
    assert strict_refusal("gemv_fp4_fused", (off16(1024), d, d, 64, [64, 1024], None, None, 1)) == fp4["fp4_hip_gemv_fused"]["gate|up, misaligned x"][1]
    assert strict_refusal("gemv_nf4_fused", (off16(1024), d, d, 64, [64, 1024], None, None, 0)) == nf4["fp4_hip_gemv_fused_nf4"]["misaligned x"][1]
    assert (strict_refusal("gemm_nf4_nested", (off16(4 * 512).view(4, 512), d, d, d, d, 0.0, 256, 64, [64, 512], None, None, 0))
            == nf4["fp4_hip_gemm_nested_nf4"]["misaligned x"][1])
    assert (strict_refusal("gemm_nf4_lora_multi", (off16(4 * 512).view(4, 512), d, d, 64, [64, 512], None, None, 0, d, d, d))
            == nf4["fp4_hip_gemm_lora_multi_nf4"]["misaligned x"][1].replace("1..64 rows", "1..128 rows"))
    # what the layers catch: the two wordings, by op family
    for op, (kind, entry, _) in STRICT_RULES.items():
        assert entry.startswith("fp4_hip_") and kind in ("small_fp4", "gemv_fp4_gated", "nf4_gemv", "nf4_gemm", "lora_down")
    assert "not covered" in strict_refusal("lora_down", (off16(512).view(1, 512), torch.zeros(16, 512, dtype=BF16), d))
    assert strict_refusal("lora_down", (torch.zeros(1, 512, dtype=BF16), torch.zeros(16, 512, dtype=BF16), d)) is None
    # the plain epilogue of the FP4 GEMV takes any address (its generic kernel); f32 rows of the small-batch op are GEMV launches
    assert strict_refusal("gemv_fp4_fused", (off16(1024), d, d, 64, [64, 1024], None, None, 0)) is None
    assert strict_refusal("gemm_small_fp4", (off16(2 * 64, F32).view(2, 64), d, d, 16, [24, 64], None)) is None
    # block sizes: a power of two from 32 that divides K; anything else is refused at an aligned address as well
    x = lambda rows, K: torch.zeros(rows, K, dtype=F16)  # noqa: E731
    for bs, K in L.BLOCKSIZE_CASES:
        got = strict_refusal("gemm_small_fp4", (x(2, K), d, d, bs, [24, K], None))
        assert (got is None) == L.fused_blocksize(bs), (bs, K, got)
        if got is not None:
            assert got == f"fp4_hip_gemm_small: shape B=2 M=24 K={K} blocksize={bs} dtype=0 is not covered; use dequant + GEMM"
    assert strict_refusal("gemm_small_fp4", (x(9, 512), d, d, 128, [24, 512], None)) is not None  # above 8 rows: blocksize 64 only
    assert strict_refusal("qlinear", (off16(1024), d, d, 64, 1024, 64)) is None and strict_refusal("gemv_nf4", (off16(1024),)) is None


def test_a_strict_double_records_the_refused_call_and_raises():
    fake = Strict(FakeExt(pkg.ext))
    p, a = o.quantize_fp4((np.random.default_rng(0).standard_normal(24 * 64) * 0.05).astype(np.float32), 64)
    P, A = torch.from_numpy(p).view(1, -1), torch.from_numpy(a)
    with pytest.raises(RuntimeError, match="is not covered; use dequant"):
        fake.gemm_small_fp4(off16(2 * 64).view(2, 64), P, A, 64, [24, 64], None)
    assert fake.calls == ["gemm_small_fp4"]
    y = fake.gemm_small_fp4(torch.zeros(2, 64, dtype=BF16), P, A, 64, [24, 64], None)
    assert tuple(y.shape) == (2, 24) and fake.calls == ["gemm_small_fp4"] * 2


# ---- QuantData under each switch ---------------------------------------------------------------------------------------------------------
class Forward:
    def __init__(self, qd):
        self.qd = qd

    def __call__(self, x):
        return self.qd.forward(x)


def fp4_qd(M, K, bs=64, seed=1, **kw):
    p, a = o.quantize_fp4((np.random.default_rng(seed).standard_normal(M * K) * 0.05).astype(np.float32), bs)
    state = pkg.QuantState(torch.from_numpy(a), (M, K), torch.from_numpy(o.TREE_TABLE.copy()), bs, quant_type="fp4")
    bias = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal(M).astype(np.float32) * 0.1)
    return qd_mod.QuantData(torch.from_numpy(p).view(-1, 1), state, state.shape, bias=bias, **kw)


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DT16 + [F32], ids=lambda d: str(d)[6:])
def test_fp4_quant_data_under_the_switch(monkeypatch, dtype, shape):
    M, K = shape
    rec = install(monkeypatch, FakeExt(pkg.ext))
    rows = L.ROWS_F32 if dtype == F32 else L.ROWS + L.ROWS_FP4_MORE
    records = run(rec, "QuantData fp4 small_batch_fused", dtype, lambda: Forward(fp4_qd(M, K, small_batch_fused=True)), K, M, rows)
    for r, how, route, _ in records:
        assert ("gemm_small_fp4" in L.ops(route)) == (L.n_rows(r) >= 2), (r, how, route)


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DT16, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("switch", ["small_batch_fused_nf4", "wide_batch_fused_nf4"])
def test_nf4_quant_data_under_each_switch(monkeypatch, switch, dtype, shape):
    M, K = shape
    rec = install(monkeypatch, RecordingWideExt())
    bias = L.random(M, F32, 3, CPU, 0.1)

    def build():
        qd = _nf4_qd(M, K, **{switch: True})
        qd.bias = bias.clone()  # the helper draws an unseeded one: both layer objects get the same
        return Forward(qd)
    records = run(rec, f"QuantData nf4 {switch}", dtype, build, K, M, L.ROWS)
    op = {"small_batch_fused_nf4": "gemm_small_nf4", "wide_batch_fused_nf4": "gemm_wide_nf4"}[switch]
    for r, how, route, _ in records:
        n = L.n_rows(r)
        want = (2 <= n <= 16 and K % 512 == 0) if op == "gemm_small_nf4" else (17 <= n <= 64 or (2 <= n <= 16 and K % 512 != 0))
        assert (op in L.ops(route)) == want, (r, how, route)


# ---- the fused layers --------------------------------------------------------------------------------------------------------------------
def fp4_packed(M, K, seed, bs=64):
    p, a = o.quantize_fp4((np.random.default_rng(seed).standard_normal(M * K) * 0.05).astype(np.float32), bs)
    return torch.from_numpy(p).view(-1, 1), torch.from_numpy(a)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gate|up"])
@pytest.mark.parametrize("dtype", DT16, ids=lambda d: str(d)[6:])
def test_fused_fp4_linear(monkeypatch, dtype, gated):
    M, K = L.MAIN if not gated else (64, 512)
    rec = install(monkeypatch, FakeExt(pkg.ext))
    if gated:
        build = lambda: pkg.FusedFP4Linear.gate_up_from_packed(fp4_packed(M, K, 11), fp4_packed(M, K, 12), (M, K), 64)  # noqa: E731
    else:
        build = lambda: pkg.FusedFP4Linear.from_packed(*fp4_packed(M, K, 1), (M, K), 64, torch.zeros(M))  # noqa: E731
    records = run(rec, f"FusedFP4Linear gated={gated}", dtype, build, K, M, [1, (1, 1), 2, 8, 17, 65], residual=True)
    for r, how, route, _ in records:
        assert L.ops(route) == ["gemv_fp4_fused" if L.n_rows(r) == 1 else "gemm_small_fp4_fused"], (r, how, route)


NF4_ROWS = [1, (1, 1), 2, 17, 64]


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gate|up"])
@pytest.mark.parametrize("dtype", DT16, ids=lambda d: str(d)[6:])
def test_fused_nf4_and_lora_linear(monkeypatch, dtype, gated):
    M, K = 64, 512
    rec = install(monkeypatch, MultiLoraExt())
    g, u = _nf4_layer(M, K, 1), _nf4_layer(M, K, 2)
    ad = lambda seed: (*_adapter(M, K, L.RANK, seed, dtype), 2.0)  # noqa: E731
    if gated:
        fused = lambda: pkg.FusedNF4Linear.gate_up(g, u)  # noqa: E731
        lora = lambda: pkg.LoRANF4Linear.gate_up(g, u, ad(3), ad(4))  # noqa: E731
    else:
        fused = lambda: pkg.FusedNF4Linear.from_linear(g)  # noqa: E731
        lora = lambda: pkg.LoRANF4Linear.from_linear(g, *ad(3))  # noqa: E731
    for r, how, route, _ in run(rec, f"FusedNF4Linear gated={gated}", dtype, fused, K, M, NF4_ROWS, residual=True):
        assert L.ops(route) == ["gemv_nf4_fused" if L.n_rows(r) == 1 else "gemm_nf4_fused"], (r, how, route)
    for r, how, route, _ in run(rec, f"LoRANF4Linear gated={gated}", dtype, lora, K, M, NF4_ROWS, residual=True):
        assert L.ops(route) == ["lora_down", "gemv_nf4_lora" if L.n_rows(r) == 1 else "gemm_nf4_lora"], (r, how, route)


@pytest.mark.parametrize("dtype", DT16, ids=lambda d: str(d)[6:])
def test_multi_lora_linear(monkeypatch, dtype):
    M, K = 64, 512
    rec = install(monkeypatch, MultiLoraExt())
    base = _nf4_layer(M, K, 1)
    ads = [(*_adapter(M, K, 16, 5, dtype), 2.0), (*_adapter(M, K, 8, 6, dtype), 0.5)]
    sel = pkg.AdapterSelection()
    ids = [0, 1, -1]
    records = run(rec, "MultiLoRANF4Linear", dtype, lambda: pkg.MultiLoRANF4Linear.from_linear(base, ads, sel), K, M, NF4_ROWS, residual=True,
                  before=lambda n: sel.set([ids[(b + n) % 3] for b in range(n)]))
    for r, how, route, _ in records:
        assert L.ops(route) == ["lora_down_multi", "gemv_nf4_lora_multi" if L.n_rows(r) == 1 else "gemm_nf4_lora_multi"], (r, how, route)


@pytest.mark.parametrize("lora", [False, True], ids=["NestedNF4Linear", "LoRANestedNF4Linear"])
def test_nested_linear_under_both_switches(monkeypatch, lora):
    M, K = 48, 512
    rec = install(monkeypatch, RouteExt(nested_mod.ext), also=(nn_mod,))

    def build():
        layer = nested_layer(M, K)
        assert pkg.set_small_batch_fused(layer, True, nf4=True, nf4_wide=True) == 1
        return pkg.LoRANestedNF4Linear.from_nested(layer, *_adapter(M, K, 16, 7), 2.0) if lora else layer
    records = run(rec, "nested", BF16, build, K, M, L.ROWS, residual=True)
    if not lora:
        for r, how, route, _ in records:
            assert ("gemm_nf4_nested" in L.ops(route)) == (L.n_rows(r) >= 2), (r, how, route)


# ---- block sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16 + [F32], ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("bs,K", L.BLOCKSIZE_CASES)
def test_blocksize_routes(monkeypatch, bs, K, dtype):
    """The two copies of the FP4 predicate (QuantData.forward, FusedFP4Linear._batched_covers) against the strict double: a block size
    the entry point does not take never reaches it."""
    M = L.BLOCKSIZE_M
    rec = install(monkeypatch, FakeExt(pkg.ext))
    qd = fp4_qd(M, K, bs, seed=bs, small_batch_fused=True)
    layer = pkg.FusedFP4Linear.from_packed(*fp4_packed(M, K, bs, bs), (M, K), bs, torch.zeros(M))
    for rows in L.BLOCKSIZE_ROWS:
        x = L.random((rows, K), dtype, rows, CPU)
        for how in L.PLACEMENTS:
            rec.take()
            y = qd.forward(L.placed(x, how))
            route = L.ops(rec.take())
            assert tuple(y.shape) == (rows, M)
            if dtype == F32 or L.fused_blocksize(bs):
                assert route == ["gemm_small_fp4"], (rows, how, route)
            else:
                assert len(route) == 1 and route[0].startswith("qlinear"), (rows, how, route)
            layer(L.placed(x, how))  # the batched fused op is 16-bit: f32 runs the unfused sequence at every blocksize
            route = L.ops(rec.take())
            fused = dtype != F32 and L.fused_blocksize(bs)
            assert (route == ["gemm_small_fp4_fused"]) if fused else (len(route) == 1 and route[0].startswith("qlinear")), route
