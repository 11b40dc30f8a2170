"""NF4 on the host (no GPU): the format restatement against bitsandbytes' published constants, the C ABI's table and argument
checks, the safetensors key set, and QuantData's dispatch of an NF4 quant_state (through a numpy-backed fake extension)."""
import os
import re
import types

import numpy as np
import pytest
import torch

import nf4_ref as R
import torch_bnb_fp4 as pkg
from torch_bnb_fp4 import fused as fused_mod, functional as F_mod, quant_data as qd_mod

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "torch-bnb-fp4_amd", "csrc")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the format ----------------------------------------------------------------------------------------------------------------
def test_thresholds_are_the_midpoints_of_the_code():
    assert (_bits(R.THRESHOLD_DECIMAL) == _bits(R.midpoint_thresholds())).all()
    assert (np.diff(R.CODE) > 0).all() and R.CODE[0] == -1.0 and R.CODE[7] == 0.0 and R.CODE[15] == 1.0
    assert not np.signbit(R.CODE[7])


def test_kernel_sources_carry_the_same_literals():
    common = open(os.path.join(CSRC, "fp4_common.h")).read()
    table = re.search(r"#define FP4_NF4_BITS(.*?)\n\s*static", common, re.S).group(1)
    assert [int(h, 16) for h in re.findall(r"0x([0-9A-F]{8})u", table)] == _bits(R.CODE).tolist()
    quant = open(os.path.join(CSRC, "quantize_nf4.hip")).read()
    thr = re.search(r"kNf4ThrBits\[15\] = \{(.*?)\};", quant, re.S).group(1)
    assert [int(h, 16) for h in re.findall(r"0x([0-9A-F]{8})u", thr)] == _bits(R.THRESHOLDS).tolist()


def _tree_vectorised(x):
    """dQuantizeNF4's tree, as its 4 levels of compares (node indices of the tree: 7; 3 | 11; 1 5 9 13; 0 2 ... 14)."""
    T = R.THRESHOLDS
    i = np.where(x > T[7], 8, 0)
    i = i + 4 * (x > T[i + 3])
    i = i + 2 * (x > T[i + 1])
    return i + (x > T[i])


def test_count_rule_equals_the_decision_tree():
    """Both forms are compare-only step functions of x; they are compared on a sweep of the f32 patterns of [-2, 2] (every 97th,
    both signs), on every threshold and its 4 neighbours on either side, and on NaN / +-inf / +-0."""
    pos = np.arange(0, 0x40000001, 97, dtype=np.uint32)
    sweep = np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)
    with np.errstate(invalid="ignore"):
        assert (R.rank(sweep) == _tree_vectorised(sweep)).all()
    edge = [R.THRESHOLDS]
    for direction in (np.inf, -np.inf):
        v = R.THRESHOLDS.copy()
        for _ in range(4):
            v = np.nextafter(v, np.float32(direction))
            edge.append(v)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 2.0, -2.0], np.float32)
    edge = np.concatenate(edge + [special, R.CODE])
    with np.errstate(invalid="ignore"):
        assert (R.rank(edge) == R.rank_tree(edge)).all()
        assert (R.rank(edge) == _tree_vectorised(edge)).all()
    assert R.rank(np.float32(np.nan)) == 0 and R.rank(np.float32(np.inf)) == 15 and R.rank(np.float32(-np.inf)) == 0
    assert (R.rank(R.THRESHOLDS) == np.arange(15)).all()  # strict '>': a value on T[i] stays below it


def test_all_zero_block_is_zero_bytes_and_dequantises_to_minus_zero():
    packed, absmax = R.quantize(np.zeros(64, np.float32), 64)
    assert (packed == 0).all() and absmax[0] == 0.0
    out = R.dequantize_f32(packed, absmax, 64, 64)
    assert (_bits(out) == 0x80000000).all()


def test_odd_length_pads_with_a_ranked_zero():
    """An odd n leaves the low nibble of the last byte spare; it holds rank(0.0 * (1/absmax)) of the last block's scale, as
    bitsandbytes' quantiser (zero-filled last block, ceil(n/2) bytes stored) and the kernel write it - not a bare 0."""
    packed, absmax = R.quantize(np.array([0.5, 0.1, 0.3], np.float32), 32)
    assert packed.tobytes() == bytes([0xF9, 0xD7]) and absmax.tolist() == [0.5]
    cases = [  # last block -> spare nibble
        (np.float32(0.25), 7),     # finite, non-zero scale: 0 * 4 = 0 -> 7
        (np.float32(np.inf), 7),   # infinite scale: 0 * 0 = 0 -> 7
        (np.float32(0.0), 0),      # zero scale: 0 * inf = NaN -> 0
        (np.float32(np.nan), 0),   # NaN scale: NaN -> 0
        (np.float32(1e-40), 0),    # subnormal scale: 1/absmax overflows to inf, 0 * inf = NaN -> 0
    ]
    for bs in (32, 64, 4096):
        for v, want in cases:
            for n in (1, 3, bs + 1, 2 * bs - 1):
                w = np.full(n, 0.01, np.float32)
                w[(n - 1) // bs * bs:] = v  # the whole last block
                p, a = R.quantize(w, bs)
                assert p.size == (n + 1) // 2 and a.size == -(-n // bs)
                assert p[-1] & 15 == want, (bs, float(v), n)
                assert (R.unpack(p, n + 1)[:n] == R.unpack(R.quantize(np.append(w, np.float32(0)), bs)[0], n)).all()  # pad: its own byte
    for n in (2, 64):  # even n: no pad nibble
        p, _ = R.quantize(np.full(n, 0.5, np.float32), 32)
        assert p.size == n // 2 and (p == 0xFF).all()


def test_gemv_cases_reach_every_dispatch_cell():
    """tests/test_gpu_nf4_gemv.py runs R.GEMV_CELL_CASES: under the restated rule of dispatch_nf4 they reach all 12 cells
    (ks in 1, 2, 4; G = 2 only at ks = 4; iters in 1, 2, 4), each once with M a multiple of its rows per workgroup and once with
    a row tail, and the K values include partial last passes and more than one pass."""
    all_cells = {(ks, 1, it) for ks in (1, 2, 4) for it in (1, 2, 4)} | {(4, 2, it) for it in (1, 2, 4)}
    seen = {}
    for M, K in R.GEMV_CELL_CASES:
        assert K % 32 == 0 and 0 < K <= 32768 and 0 < M
        ks, G, it = R.gemv_cell(M, K)
        seen.setdefault((ks, G, it), set()).add(M % R.rows_per_workgroup(ks, it) != 0)
    assert set(seen) == all_cells and len(all_cells) == 12
    assert all(v == {False, True} for v in seen.values()), seen
    passes = [-(-(K >> 5) // (G * 32 * ks)) for M, K in R.GEMV_CELL_CASES for ks, G, _ in [R.gemv_cell(M, K)]]
    partial = [(K >> 5) % (G * 32 * ks) != 0 for M, K in R.GEMV_CELL_CASES for ks, G, _ in [R.gemv_cell(M, K)]]
    assert max(passes) >= 4 and sum(p > 1 for p in passes) >= 4 and sum(partial) >= 12
    # the thresholds the cases sit on either side of (issue: iters 2 from 4096 / 2048 / 1024 rows, 4 from 8192 / 4096 / 2048)
    for ks, K, lo2, lo4 in ((1, 1024, 4096, 8192), (2, 2048, 2048, 4096), (4, 4096, 1024, 2048)):
        assert R.gemv_cell(lo2 - 1, K)[2] == 1 and R.gemv_cell(lo2, K)[2] == 2
        assert R.gemv_cell(lo4 - 1, K)[2] == 2 and R.gemv_cell(lo4, K)[2] == 4


# ---- C ABI (host-side paths only: no GPU work) ------------------------------------------------------------------------------------
def test_abi_code_table():
    assert (_bits(R.code_table()) == _bits(R.CODE)).all()
    assert (_bits(pkg.ext.code_table("nf4").numpy()) == _bits(R.CODE)).all()
    assert (_bits(pkg.nf4_code().numpy()) == _bits(R.CODE)).all()


def test_abi_argument_validation():
    import ctypes

    l = R.lib()
    vp = ctypes.c_void_p
    dummy = vp(0x1000)
    # gemv: odd K, odd blocksize, negative M -> invalid; bad dtype -> unsupported; null pointers -> invalid; M == 0 -> no-op
    assert l.fp4_hip_gemv_nf4(dummy, dummy, dummy, None, dummy, 4, 33, 64, 0, None) == 1
    assert l.fp4_hip_gemv_nf4(dummy, dummy, dummy, None, dummy, 4, 64, 63, 0, None) == 1
    assert l.fp4_hip_gemv_nf4(dummy, dummy, dummy, None, dummy, -1, 64, 64, 0, None) == 1
    assert l.fp4_hip_gemv_nf4(dummy, dummy, dummy, None, dummy, 4, 64, 64, 7, None) == 2
    assert "dtype" in l.fp4_hip_last_error().decode()
    assert l.fp4_hip_gemv_nf4(None, dummy, dummy, None, dummy, 4, 64, 64, 0, None) == 1
    assert l.fp4_hip_gemv_nf4(dummy, dummy, dummy, None, None, 4, 64, 64, 0, None) == 1
    assert l.fp4_hip_gemv_nf4(None, None, None, None, None, 0, 64, 64, 0, None) == 0
    assert l.fp4_hip_gemv_nf4(dummy, dummy, dummy, None, dummy, 1 << 31, 64, 64, 0, None) == 2
    # quantiser: blocksize outside 32..4096 / not a power of two -> unsupported; n < 0 -> invalid; bad dtype; nulls; alignment
    for bs in (16, 48, 8192):
        assert l.fp4_hip_quantize_blockwise_nf4(dummy, 0, dummy, dummy, 64, bs, None) == 2
    assert l.fp4_hip_quantize_blockwise_nf4(dummy, 0, dummy, dummy, -1, 64, None) == 1
    assert l.fp4_hip_quantize_blockwise_nf4(dummy, 5, dummy, dummy, 64, 64, None) == 2
    assert l.fp4_hip_quantize_blockwise_nf4(None, 0, dummy, dummy, 64, 64, None) == 1
    assert l.fp4_hip_quantize_blockwise_nf4(vp(0x1002), 0, dummy, dummy, 64, 64, None) == 2
    assert l.fp4_hip_quantize_blockwise_nf4(None, 0, None, None, 0, 64, None) == 0
    # dequant: the NF4 table id is accepted (n == 0: nothing to do), the next one is not
    assert l.fp4_hip_dequantize_blockwise(None, None, None, 64, 0, 0, R.TABLE_NF4, 0, None) == 0
    assert l.fp4_hip_dequantize_blockwise(None, None, None, 64, 0, 0, 3, 0, None) == 1
    assert l.fp4_hip_code_table(3, vp(0x1000)) == 1


# ---- serialization key set ------------------------------------------------------------------------------------------------------
def _nf4_quant_data(M=64, K=128, bs=64, bias=True, **kw):
    rng = np.random.default_rng(1)
    w = (rng.standard_normal(M * K) * 0.05).astype(np.float32)
    packed, am = R.quantize(w, bs)
    state = pkg.QuantState(torch.from_numpy(am), (M, K), torch.from_numpy(R.CODE.copy()), bs, quant_type="nf4")
    b = torch.from_numpy(rng.standard_normal(M).astype(np.float32)) if bias else None
    qd = pkg.QuantData(torch.from_numpy(packed).reshape(-1, 1), state, (M, K), bias=b, **kw)
    return qd, w


def test_nf4_state_keys_match_the_installed_transformers_loader():
    import json

    from transformers import BitsAndBytesConfig
    from transformers.quantizers.quantizer_bnb_4bit import Bnb4BitHfQuantizer

    conv = Bnb4BitHfQuantizer(BitsAndBytesConfig(load_in_4bit=True, bnb_4bit_quant_type="nf4"), pre_quantized=True).get_weight_conversions()
    patterns = set(conv[0].source_patterns)
    qd, _ = _nf4_quant_data()
    layer = types.SimpleNamespace(quant_data=qd, bias=qd.bias)
    prefix = "model.layers.0.mlp.down_proj."
    state = pkg.fp4_linear_to_bnb_state(layer, prefix)
    ours = {k[len(prefix):] for k in state} - {"bias"}
    assert ours == {p for p in patterns if "nested" not in p and "fp4" not in p}, ours
    meta = json.loads(bytes(state[prefix + "weight.quant_state.bitsandbytes__nf4"].tolist()).decode())
    assert meta == {"quant_type": "nf4", "blocksize": 64, "dtype": "float16", "shape": [64, 128]}
    assert (_bits(state[prefix + "weight.quant_map"].numpy()) == _bits(R.CODE)).all()


def test_load_refuses_a_custom_quant_map():
    qd, _ = _nf4_quant_data()
    state = pkg.fp4_linear_to_bnb_state(types.SimpleNamespace(quant_data=qd, bias=None), "")
    state["weight.quant_map"] = state["weight.quant_map"].clone()
    state["weight.quant_map"][3] = float(np.nextafter(np.float32(state["weight.quant_map"][3]), np.float32(1)))
    with pytest.raises(ValueError, match="quant_map"):
        pkg.fp4_linear_from_bnb_state(state, "", device="cpu")


# ---- dispatch ------------------------------------------------------------------------------------------------------------------
class RecordingNf4Ext:
    """Stands in for the extension: NF4 ops answer from the numpy restatement, FP4 ops fail the test."""

    def __init__(self):
        self.calls = []

    def _w(self, A, absmax, M, N, blocksize):
        return torch.from_numpy(R.dequantize_f32(A.numpy().ravel(), absmax.numpy(), blocksize, M * N).reshape(M, N))

    def dequantize_nf4(self, A, absmax, blocksize, M, N, o_type):
        self.calls.append("dequantize_nf4")
        return self._w(A, absmax, M, N, blocksize)

    def _gemv(self, name, A, B, absmax, blocksize, dtype, Bshape, bias=None):
        self.calls.append(name)
        M, K = Bshape
        y = (A.float().reshape(1, K) @ self._w(B, absmax, M, K, blocksize).t()).to(A.dtype)
        return y + bias if bias is not None else y

    def gemv_nf4(self, A, B, absmax, blocksize, dtype, Bshape):
        return self._gemv("gemv_nf4", A, B, absmax, blocksize, dtype, Bshape)

    def gemv_nf4_bias(self, A, B, absmax, blocksize, dtype, Bshape, bias):
        return self._gemv("gemv_nf4_bias", A, B, absmax, blocksize, dtype, Bshape, bias)

    def _ql(self, name, A_in, A, absmax, M, N, blocksize, bias=None):
        self.calls.append(name)
        return torch.nn.functional.linear(A_in.float(), self._w(A, absmax, M, N, blocksize), None if bias is None else bias.float()).to(A_in.dtype)

    def qlinear_nf4(self, A_in, A, absmax, M, N, blocksize):
        return self._ql("qlinear_nf4", A_in, A, absmax, M, N, blocksize)

    def qlinear_nf4_bias(self, A_in, A, absmax, M, N, blocksize, bias):
        return self._ql("qlinear_nf4_bias", A_in, A, absmax, M, N, blocksize, bias)

    def __getattr__(self, name):
        raise AssertionError(f"an NF4 layer called the FP4 op {name}")


@pytest.fixture()
def rec(monkeypatch):
    r = RecordingNf4Ext()
    monkeypatch.setattr(F_mod, "ext", r)
    monkeypatch.setattr(qd_mod, "ext", r)
    return r


@pytest.mark.parametrize("codebook", [True, False])
@pytest.mark.parametrize("reduced", [True, False])
def test_nf4_quant_state_dispatches_to_the_nf4_ops(rec, codebook, reduced):
    qd, w = _nf4_quant_data(use_codebook_dequant=codebook, allow_reduced_precision_linear=reduced, small_batch_fused=True)
    x = torch.randn(1, 128)
    y = qd.forward(x)
    assert rec.calls == ["gemv_nf4_bias"]
    wq = R.dequantize_f32(qd.A.numpy().ravel(), qd.absmax.numpy(), 64, 64 * 128).reshape(64, 128)
    ref = x.numpy().astype(np.float64) @ wq.T.astype(np.float64) + qd.bias.numpy()
    np.testing.assert_allclose(y.numpy(), ref, rtol=1e-4, atol=1e-4)
    rec.calls.clear()
    qd.forward(x.reshape(1, 1, 128))
    assert rec.calls == ["gemv_nf4_bias"]
    for rows in (2, 8, 200):  # small_batch_fused is ignored for NF4: every batch > 1 is dequant + GEMM
        rec.calls.clear()
        assert tuple(qd.forward(torch.randn(rows, 128)).shape) == (rows, 64)
        assert rec.calls == ["qlinear_nf4_bias"]
    rec.calls.clear()
    qd.bias = None
    qd.forward(torch.randn(3, 128))
    qd.forward(torch.randn(1, 128))
    assert rec.calls == ["qlinear_nf4", "gemv_nf4"]


def test_unknown_quant_type_raises():
    qd, _ = _nf4_quant_data()
    for qt in ("int4", None, "NF4"):
        state = pkg.QuantState(qd.absmax, (64, 128), qd.code, 64, quant_type=qt)
        with pytest.raises(ValueError, match="quant_type"):
            pkg.QuantData(qd.A, state, (64, 128))
    with pytest.raises(ValueError, match="quant_type"):
        pkg.LinearFP4(128, 64, quant_type="int4")


def test_fp4_only_paths_refuse_nf4():
    qd, _ = _nf4_quant_data()
    layer = types.SimpleNamespace(quant_data=qd, use_codebook_dequant=True)
    with pytest.raises(ValueError, match="NF4"):
        pkg.TorchFP4Linear.fuse([layer, layer])
    with pytest.raises(ValueError, match="NF4"):
        fused_mod.FusedFP4Linear(qd)
    with pytest.raises(ValueError, match="NF4"):
        fused_mod.FusedFP4Linear.from_linear(layer)
    with pytest.raises(ValueError, match="NF4"):
        fused_mod.FusedFP4Linear.gate_up(layer, layer)


def test_nn_stand_ins_carry_the_quant_type():
    assert pkg.LinearNF4(128, 64).quant_type == "nf4"
    assert pkg.Linear4bit(128, 64, quant_type="nf4").quant_type == "nf4"
    assert pkg.Linear4bit(128, 64).quant_type == "fp4"
    assert isinstance(pkg.LinearNF4(128, 64), pkg.LinearFP4)
    assert pkg.LinearNF4(128, 64).weight.quant_type == "nf4"
