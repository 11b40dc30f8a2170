"""Double-quantised (nested) absmax on the host (no GPU): the dynamic map's digest, the three C entry points' declaration and
argument validation (every call below returns before any HIP call), and the loader / saver through a fake extension whose
``absmax_unnest`` / ``absmax_nest`` are the numpy oracle of tests/nested_ref.py."""
import ctypes
import hashlib
import json
import types

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nested_ref as N
import nf4_ref as R
import torch_bnb_fp4 as pkg
from oracle import fp4_oracle as o
from torch_bnb_fp4 import nested as nested_mod, nn as nn_mod, serialization as ser_mod

OK, INVALID, UNSUPPORTED = 0, 1, 2
F16, F32, BF16 = 0, 1, 2


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_dynamic_map_digest_and_values():
    for table in (N.dynamic_map(), nested_mod.dynamic_map().numpy()):
        assert table.dtype == np.float32 and table.shape == (256,) and bool((np.diff(table) > 0).all())
        assert hashlib.sha256(table.astype("<f4").tobytes()).hexdigest() == N.DYNAMIC_MAP_SHA256
        want = {0: -0.992968738079071, 1: -0.9789062738418579, 127: 0.0, 128: 5.500000384017767e-07, 254: 0.992968738079071, 255: 1.0}
        for i, v in want.items():
            assert table[i] == np.float32(v), (i, table[i])


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entry_points_under_abi_7():
    assert {"fp4_hip_absmax_unnest", "fp4_hip_absmax_nest", "fp4_hip_gemv_nested_nf4"} <= set(hipabi.declared_symbols())
    assert N.lib().fp4_hip_abi_version() == 7
    header = open(hipabi.HEADER).read()
    assert int(header.split("#define FP4_HIP_ABI_VERSION")[1].split()[0]) == 7


def test_unnest_and_nest_argument_validation():
    l, d = N.lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    un = lambda q, nested, code, g, nb, out: l.fp4_hip_absmax_unnest(q, nested, code, 0.5, g, nb, out, None)
    ne = lambda a, nb, code, g, q, nested: l.fp4_hip_absmax_nest(a, nb, 0.5, code, g, q, nested, None)
    for g in (0, 32, 48, 100, 8192, -256):
        assert un(d, d, d, g, 1000, d) == UNSUPPORTED and "nested_blocksize" in err()
        assert ne(d, 1000, d, g, d, d) == UNSUPPORTED and "nested_blocksize" in err()
    for g in (64, 256, 4096):  # nb == 0: nothing to do, whatever the pointers
        assert un(None, None, None, g, 0, None) == OK
        assert ne(None, 0, None, g, None, None) == OK
    assert un(d, d, d, 256, -1, d) == INVALID and ne(d, -1, d, 256, d, d) == INVALID
    for args in ((None, d, d, 256, 10, d), (d, None, d, 256, 10, d), (d, d, None, 256, 10, d), (d, d, d, 256, 10, None)):
        assert un(*args) == INVALID and "null" in err()
    for args in ((None, 10, d, 256, d, d), (d, 10, None, 256, d, d), (d, 10, d, 256, None, d), (d, 10, d, 256, d, None)):
        assert ne(*args) == INVALID and "null" in err()
    assert un(d, d, d, 256, (1 << 31) + 1, d) == UNSUPPORTED and ne(d, (1 << 31) + 1, d, 256, d, d) == UNSUPPORTED


def test_gemv_nested_argument_validation():
    l, d = N.lib(), ctypes.c_void_p(0x1000)
    err = lambda: l.fp4_hip_last_error().decode()
    gemv = lambda x, q, nested, code, g, out, M, K, bs, dt, epi: l.fp4_hip_gemv_nested_nf4(x, d, q, nested, code, 0.25, g, None, None, out,
                                                                                           M, K, bs, dt, epi, None)
    assert gemv(d, d, d, d, 256, d, 64, 64, 64, BF16, 7) == INVALID and "unknown epilogue" in err()
    assert gemv(d, d, d, d, 256, d, 63, 64, 64, BF16, 1) == INVALID and "even row count" in err()
    assert gemv(d, d, d, d, 0, d, 64, 64, 64, BF16, 0) == INVALID and "nested_blocksize" in err()
    assert gemv(d, d, None, d, 256, d, 64, 64, 64, BF16, 0) == INVALID and "null" in err()
    assert gemv(d, d, d, None, 256, d, 64, 64, 64, BF16, 0) == INVALID and "null" in err()
    assert gemv(d, None, d, d, 256, d, 64, 64, 64, BF16, 0) == INVALID and "null" in err()
    assert gemv(None, d, d, d, 256, d, 64, 64, 64, BF16, 0) == INVALID
    assert gemv(d, d, d, d, 256, None, 64, 64, 64, BF16, 0) == INVALID
    assert gemv(None, None, None, None, 256, None, 0, 64, 64, BF16, 0) == OK  # M == 0
    for g in (64, 128, 512, 4096, 100):  # only groups of 256 are read by the GEMV
        assert gemv(d, d, d, d, g, d, 64, 64, 64, BF16, 0) == UNSUPPORTED and "nested_blocksize" in err()
    # outside the fused entry point's fast path: reported, never computed
    assert gemv(d, d, d, d, 256, d, 64, 48, 16, BF16, 0) == UNSUPPORTED and "not available" in err()
    assert gemv(d, d, d, d, 256, d, 64, 96, 96, BF16, 0) == UNSUPPORTED
    assert gemv(d, d, d, d, 256, d, 64, 64, 128, BF16, 0) == UNSUPPORTED
    assert gemv(ctypes.c_void_p(0x1002), d, d, d, 256, d, 64, 64, 64, BF16, 0) == UNSUPPORTED and "not available" in err()
    assert gemv(d, d, d, d, 256, d, 64, 64, 64, F32, 1) == UNSUPPORTED  # the gated epilogue is 16-bit only
    assert gemv(d, d, d, d, 256, d, 64, 64, 64, 5, 0) == UNSUPPORTED and "dtype" in err()
    assert gemv(d, d, d, d, 256, d, 64, 33, 64, BF16, 0) == INVALID  # odd K


# ---- loader and saver through a fake extension ----------------------------------------------------------------------------------------
class NestedExt:
    """The two statistics ops answered by the numpy oracle; everything else is the real extension's host-side code."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def absmax_unnest(self, q, nested, code, offset, g):
        self.calls.append("absmax_unnest")
        assert q.dtype == torch.uint8 and nested.dtype == torch.float32 and code.numel() == 256 and isinstance(offset, float)
        return torch.from_numpy(N.unnest(q.numpy(), nested.numpy(), code.numpy(), offset, g))

    def absmax_nest(self, absmax, offset, code, g):
        self.calls.append("absmax_nest")
        q, nested, _ = N.nest(absmax.numpy(), offset, code.numpy(), g)
        return torch.from_numpy(q), torch.from_numpy(nested)


class HostParams4bit(pkg.Params4bit):
    """A Params4bit that says it lives on a GPU: TorchFP4Linear insists on that, and these tests run its host logic on CPU tensors."""

    device = property(lambda self: torch.device("cuda", 0))


@pytest.fixture()
def fx(monkeypatch):
    fake = NestedExt(nested_mod.ext)
    for mod in (nested_mod, nn_mod):
        monkeypatch.setattr(mod, "ext", fake)
    monkeypatch.setattr(ser_mod, "Params4bit", HostParams4bit)
    return fake


def _nested_state(quant_type, M=48, K=512, bs=64, g=256, seed=0, prefix="l.", bias=False):
    """A well-formed double-quantised state as bitsandbytes writes it, the oracle's expanded absmax, and the pieces."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(M * K) * 0.05).astype(np.float32)
    if quant_type == "nf4":
        packed, absmax = R.quantize(w, bs)
        code = R.CODE.copy()
    else:
        packed, absmax = o.quantize_fp4(w, bs)
        code = o.TREE_TABLE.copy()
    table = N.dynamic_map()
    offset = float(np.float32(absmax.mean()))
    q, nested, _ = N.nest(absmax, offset, table, g)
    meta = {"quant_type": quant_type, "blocksize": bs, "dtype": "bfloat16", "shape": [M, K], "nested_blocksize": g,
            "nested_dtype": "float32", "nested_offset": offset}
    state = {
        prefix + "weight": torch.from_numpy(packed).reshape(-1, 1),
        prefix + "weight.absmax": torch.from_numpy(q),
        prefix + "weight.quant_map": torch.from_numpy(code),
        prefix + "weight.nested_absmax": torch.from_numpy(nested),
        prefix + "weight.nested_quant_map": torch.from_numpy(table.copy()),
        prefix + f"weight.quant_state.bitsandbytes__{quant_type}": torch.tensor(list(json.dumps(meta).encode()), dtype=torch.uint8),
    }
    if bias:
        state[prefix + "bias"] = torch.from_numpy(rng.standard_normal(M).astype(np.float32))
    return state, N.unnest(q, nested, table, offset, g), meta


@pytest.mark.parametrize("quant_type,M,K,g", [("nf4", 48, 512, 256), ("fp4", 48, 512, 256), ("nf4", 40, 416, 256), ("fp4", 33, 64, 64)])
def test_a_well_formed_nested_state_loads_expanded(fx, quant_type, M, K, g):
    """Fails on the parent commit, which raises on the first nested layer."""
    bs = 64 if K % 64 == 0 else 32
    state, want, _ = _nested_state(quant_type, M, K, bs, g, bias=True)
    for kw in ({}, {"nested": "expand"}):
        layer = pkg.fp4_linear_from_bnb_state(state, "l.", device="cpu", **kw)
        assert type(layer) is pkg.TorchFP4Linear and layer.quant_data.quant_type == quant_type
        assert layer.quant_data.absmax.dtype == torch.float32
        assert np.array_equal(_bits(layer.quant_data.absmax.numpy()), _bits(want))
        assert np.array_equal(_bits(layer.absmax.numpy()), _bits(want)) and not layer.quant_data.quant_state.nested
        assert torch.equal(layer.qweight, state["l.weight"]) and layer.bias is not None
        assert layer.quant_data.quant_state.dtype == torch.bfloat16
    assert fx.calls == ["absmax_unnest"] * 2
    # the table is taken from the file, whatever it holds: a permuted one decodes differently and is not refused
    odd = dict(state)
    odd["l.weight.nested_quant_map"] = state["l.weight.nested_quant_map"].flip(0).contiguous()
    got = pkg.fp4_linear_from_bnb_state(odd, "l.", device="cpu").quant_data.absmax.numpy()
    meta = json.loads(bytes(state[f"l.weight.quant_state.bitsandbytes__{quant_type}"].tolist()).decode())
    flipped = N.unnest(state["l.weight.absmax"].numpy(), state["l.weight.nested_absmax"].numpy(), N.dynamic_map()[::-1].copy(),
                       meta["nested_offset"], g)
    assert np.array_equal(_bits(got), _bits(flipped)) and not np.array_equal(_bits(got), _bits(want))


def _with_meta(state, quant_type, **changes):
    key = f"l.weight.quant_state.bitsandbytes__{quant_type}"
    meta = json.loads(bytes(state[key].tolist()).decode())
    for k, v in changes.items():
        if v is None:
            meta.pop(k)
        else:
            meta[k] = v
    out = dict(state)
    out[key] = torch.tensor(list(json.dumps(meta).encode()), dtype=torch.uint8)
    return out


@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
@pytest.mark.parametrize("mode", ["expand", "resident"])
def test_ill_formed_nested_states_are_refused(fx, quant_type, mode):
    state, want, meta = _nested_state(quant_type)
    load = lambda s: pkg.fp4_linear_from_bnb_state(s, "l.", device="cpu", nested=mode)
    drop = lambda k: {a: b for a, b in state.items() if a != k}
    put = lambda k, v: {**state, k: v}
    cases = {
        # the state of tests/test_gpu_module.py:334 - an f32 absmax, a 1-element nested_absmax, no map
        "f32 absmax beside a nested key": {**drop("l.weight.nested_quant_map"), "l.weight.absmax": torch.from_numpy(want),
                                           "l.weight.nested_absmax": torch.zeros(1)},
        "f32 absmax, everything else nested": put("l.weight.absmax", torch.from_numpy(want)),
        "f32 absmax beside nested JSON fields only": {k: v for k, v in put("l.weight.absmax", torch.from_numpy(want)).items() if "nested" not in k},
        "missing map": drop("l.weight.nested_quant_map"),
        "missing nested_absmax": drop("l.weight.nested_absmax"),
        "uint8 absmax alone": {k: v for k, v in _with_meta(state, quant_type, nested_blocksize=None, nested_dtype=None, nested_offset=None).items()
                               if "nested" not in k},
        "short map": put("l.weight.nested_quant_map", state["l.weight.nested_quant_map"][:255].clone()),
        "wrong nested_absmax size": put("l.weight.nested_absmax", torch.cat([state["l.weight.nested_absmax"], torch.ones(1)])),
        "wrong absmax size": put("l.weight.absmax", state["l.weight.absmax"][:-1].clone()),
        "f16 nested_absmax": put("l.weight.nested_absmax", state["l.weight.nested_absmax"].half()),
        "no nested_blocksize": _with_meta(state, quant_type, nested_blocksize=None),
        "no nested_dtype": _with_meta(state, quant_type, nested_dtype=None),
        "no nested_offset": _with_meta(state, quant_type, nested_offset=None),
        "f16 nested_dtype": _with_meta(state, quant_type, nested_dtype="float16"),
        "bad nested_blocksize": _with_meta(state, quant_type, nested_blocksize=100),
    }
    for what, bad in cases.items():
        with pytest.raises(ValueError, match="nested"):
            load(bad)
            pytest.fail(f"{what}: accepted")
    assert "absmax_unnest" not in fx.calls  # refused before anything is decoded
    assert type(load(state)) in (pkg.TorchFP4Linear, pkg.NestedNF4Linear)  # the well-formed one still loads
    with pytest.raises(ValueError, match="nested"):
        pkg.fp4_linear_from_bnb_state(state, "l.", device="cpu", nested="compressed")


def test_resident_mode_keeps_covered_nf4_weights_and_lists_the_rest(fx, tmp_path):
    from safetensors.torch import save_file

    tensors, want = {}, {}
    for name, qt, M, K, bs, g in (("a", "nf4", 48, 512, 64, 256), ("b", "fp4", 48, 512, 64, 256), ("c", "nf4", 33, 64, 64, 64),
                                  ("d", "nf4", 16, 48, 16, 256)):
        state, want[name], _ = _nested_state(qt, M, K, bs, g, seed=ord(name), prefix=name + ".", bias=name == "a")
        tensors.update(state)
    plain, plain_am = R.quantize((np.random.default_rng(9).standard_normal(32 * 64) * 0.05).astype(np.float32), 64)
    tensors.update({"e.weight": torch.from_numpy(plain).reshape(-1, 1), "e.weight.absmax": torch.from_numpy(plain_am),
                    "e.weight.quant_map": torch.from_numpy(R.CODE.copy()),
                    "e.weight.quant_state.bitsandbytes__nf4": torch.tensor(list(json.dumps(
                        {"quant_type": "nf4", "blocksize": 64, "dtype": "float16", "shape": [32, 64]}).encode()), dtype=torch.uint8)})
    path = str(tmp_path / "nested.safetensors")
    save_file({k: v.contiguous() for k, v in tensors.items()}, path)

    def fresh():
        m = nn.Module()
        m.a, m.b, m.c, m.d, m.e = nn.Linear(512, 48), nn.Linear(512, 48, bias=False), nn.Linear(64, 33, bias=False), nn.Linear(48, 16, bias=False), nn.Linear(64, 32, bias=False)
        return m

    model = pkg.load_fp4_layers(fresh(), path, device="cpu", nested="resident")
    assert type(model.a) is pkg.NestedNF4Linear and not isinstance(model.a, pkg.TorchFP4Linear)
    assert model.fp4_nested_expanded == ["b", "c", "d"]  # FP4; groups of 64; a blocksize the GEMV does not take
    for name in "bcd":
        layer = getattr(model, name)
        assert type(layer) is pkg.TorchFP4Linear and np.array_equal(_bits(layer.quant_data.absmax.numpy()), _bits(want[name]))
    assert type(model.e) is pkg.TorchFP4Linear and np.array_equal(_bits(model.e.absmax.numpy()), _bits(plain_am))
    a = model.a
    assert a.absmax_u8.dtype == torch.uint8 and torch.equal(a.absmax_u8, tensors["a.weight.absmax"])
    assert torch.equal(a.nested_absmax, tensors["a.weight.nested_absmax"]) and torch.equal(a.nested_code, tensors["a.weight.nested_quant_map"])
    assert isinstance(a.offset, float) and a.bias is not None and (a.in_features, a.out_features) == (512, 48)
    assert np.array_equal(_bits(a.expanded_absmax().numpy()), _bits(want["a"]))
    # expand() / expand_nested: the ordinary layer the default mode builds
    default = pkg.load_fp4_layers(fresh(), path, device="cpu")
    assert default.fp4_nested_expanded == [] and type(default.a) is pkg.TorchFP4Linear
    pkg.expand_nested(model)
    assert type(model.a) is pkg.TorchFP4Linear and model.a.quant_data.nf4
    assert torch.equal(model.a.absmax, default.a.absmax) and torch.equal(model.a.qweight, default.a.qweight)
    assert torch.equal(model.a.bias, default.a.bias)
    # state_dict round trip of the resident module: the offset travels as extra state
    m1 = pkg.load_fp4_layers(fresh(), path, device="cpu", nested="resident").a
    sd = m1.state_dict()
    m2 = pkg.NestedNF4Linear(torch.zeros_like(m1.qweight), torch.zeros_like(m1.absmax_u8), torch.zeros_like(m1.nested_absmax),
                             torch.zeros_like(m1.nested_code), 0.0, (48, 512), 64, torch.zeros(48), code=m1.code)
    m2.load_state_dict(sd)
    assert m2.offset == m1.offset and all(torch.equal(getattr(m2, k), getattr(m1, k)) for k in ("qweight", "absmax_u8", "nested_absmax", "nested_code", "bias"))
    with pytest.raises(ValueError, match="not covered"):
        pkg.NestedNF4Linear(torch.zeros(16 * 24, 1, dtype=torch.uint8), torch.zeros(48, dtype=torch.uint8), torch.zeros(1), torch.zeros(256), 0.0, (16, 48), 16)


def _patterns(quant_type):
    from transformers import BitsAndBytesConfig
    from transformers.quantizers.quantizer_bnb_4bit import Bnb4BitHfQuantizer

    conv = Bnb4BitHfQuantizer(BitsAndBytesConfig(load_in_4bit=True, bnb_4bit_quant_type=quant_type), pre_quantized=True).get_weight_conversions()
    assert len(conv) == 1
    other = "fp4" if quant_type == "nf4" else "nf4"
    return {p for p in conv[0].source_patterns if not p.endswith("__" + other)}


@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
def test_nested_save_writes_the_loaders_full_key_set_and_the_default_is_unchanged(fx, quant_type):
    state, want, _ = _nested_state(quant_type, bias=True)
    layer = pkg.fp4_linear_from_bnb_state(state, "l.", device="cpu")
    prefix = "model.layers.0.mlp.down_proj."
    patterns = _patterns(quant_type)
    assert any("nested" in p for p in patterns)
    nested = pkg.fp4_linear_to_bnb_state(layer, prefix, nested=True)
    assert {k[len(prefix):] for k in nested} - {"bias"} == patterns
    meta = json.loads(bytes(nested[prefix + f"weight.quant_state.bitsandbytes__{quant_type}"].tolist()).decode())
    assert set(meta) == {"quant_type", "blocksize", "dtype", "shape", "nested_blocksize", "nested_dtype", "nested_offset"}
    assert meta["nested_blocksize"] == 256 and meta["nested_dtype"] == "float32"
    assert meta["nested_offset"] == float(layer.quant_data.absmax.mean())  # bitsandbytes' choice: the mean
    assert nested[prefix + "weight.absmax"].dtype == torch.uint8 and nested[prefix + "weight.absmax"].numel() == want.size
    assert nested[prefix + "weight.nested_absmax"].dtype == torch.float32 and nested[prefix + "weight.nested_absmax"].numel() == -(-want.size // 256)
    assert hashlib.sha256(nested[prefix + "weight.nested_quant_map"].numpy().astype("<f4").tobytes()).hexdigest() == N.DYNAMIC_MAP_SHA256
    # what was written is what loads: the file reproduces itself
    again = pkg.fp4_linear_from_bnb_state(nested, prefix, device="cpu")
    q, ns, _ = N.nest(want, meta["nested_offset"], N.dynamic_map(), 256)
    assert np.array_equal(_bits(again.quant_data.absmax.numpy()), _bits(N.unnest(q, ns, N.dynamic_map(), meta["nested_offset"], 256)))
    # the default: exactly the non-nested key set, an f32 absmax with the expanded values
    for plain in (pkg.fp4_linear_to_bnb_state(layer, prefix), pkg.fp4_linear_to_bnb_state(layer, prefix, nested=False)):
        assert {k[len(prefix):] for k in plain} - {"bias"} == {p for p in patterns if "nested" not in p}
        assert plain[prefix + "weight.absmax"].dtype == torch.float32 and np.array_equal(_bits(plain[prefix + "weight.absmax"].numpy()), _bits(want))
        meta = json.loads(bytes(plain[prefix + f"weight.quant_state.bitsandbytes__{quant_type}"].tolist()).decode())
        assert set(meta) == {"quant_type", "blocksize", "dtype", "shape"}


def test_resident_layers_save_verbatim_or_expanded(fx, tmp_path):
    from safetensors.torch import load_file

    state, want, meta = _nested_state("nf4", bias=True)
    root = nn.Module()
    root.l = pkg.fp4_linear_from_bnb_state(state, "l.", device="cpu", nested="resident")
    assert type(root.l) is pkg.NestedNF4Linear
    p1, p2 = str(tmp_path / "nested.safetensors"), str(tmp_path / "plain.safetensors")
    pkg.save_fp4_model(root, p1, nested=True)
    back = load_file(p1)
    assert set(back) == set(state) and all(torch.equal(back[k], state[k]) for k in state if "quant_state" not in k)
    assert json.loads(bytes(back["l.weight.quant_state.bitsandbytes__nf4"].tolist()).decode()) == meta
    assert "absmax_nest" not in fx.calls  # verbatim: nothing is re-quantised
    pkg.save_fp4_model(root, p2)
    plain = load_file(p2)
    assert set(plain) == {k for k in state if "nested" not in k}
    assert plain["l.weight.absmax"].dtype == torch.float32 and np.array_equal(_bits(plain["l.weight.absmax"].numpy()), _bits(want))


def test_quant_state_carries_the_bitsandbytes_attributes(fx):
    plain = pkg.QuantState(torch.ones(4), (4, 64), torch.from_numpy(R.CODE.copy()), 64, quant_type="nf4")
    assert plain.nested is False and plain.offset is None and plain.state2 is None
    state, want, meta = _nested_state("nf4")
    s2 = pkg.QuantState(state["l.weight.nested_absmax"], None, state["l.weight.nested_quant_map"], 256, torch.float32)
    qs = pkg.QuantState(state["l.weight.absmax"], (48, 512), state["l.weight.quant_map"], 64, torch.bfloat16, "nf4",
                        offset=meta["nested_offset"], state2=s2)
    assert qs.nested is True and qs.state2.blocksize == 256 and qs.state2.code.numel() == 256 and qs.state2.absmax.numel() == 2
    # the dispatcher expands a nested state once instead of reading the codes as scales
    qd = pkg.QuantData(state["l.weight"], qs, (48, 512))
    assert np.array_equal(_bits(qd.absmax.numpy()), _bits(want)) and not qd.quant_state.nested
    # bitsandbytes keeps the offset as a 0-d tensor
    qs.offset = torch.tensor(meta["nested_offset"])
    assert np.array_equal(_bits(pkg.QuantData(state["l.weight"], qs, (48, 512)).absmax.numpy()), _bits(want))
    assert {"NestedNF4Linear", "expand_nested"} <= set(pkg.__all__)
