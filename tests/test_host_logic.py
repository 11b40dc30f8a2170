"""Host-side logic of the torch_bnb_fp4 mirror package on CPU: enum, dispatch table of
QuantData.forward (reference torch_bnb_fp4/__init__.py:560-618), bias handling, surgery helpers.
The extension is replaced by tests/fake_ext.py (oracle-backed) so no GPU is needed."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import torch_bnb_fp4 as pkg
from fake_ext import FakeExt
from oracle import fp4_oracle as o
from torch_bnb_fp4 import functional as F_mod, quant_data as qd_mod


@pytest.fixture()
def fake(monkeypatch):
    f = FakeExt(pkg.ext)
    monkeypatch.setattr(F_mod, "ext", f)
    monkeypatch.setattr(qd_mod, "ext", f)
    return f


def make_quant_data(M=128, K=256, bias=True, **kw):
    rng = np.random.default_rng(0)
    w = (rng.standard_normal(M * K) * 0.05).astype(np.float32)
    packed, am = o.quantize_fp4(w, 64)
    state = pkg.QuantState(torch.from_numpy(am), (M, K), torch.from_numpy(o.TREE_TABLE.copy()), 64)
    lin = nn.Linear(K, M, bias=bias)
    qd = pkg.QuantData(torch.from_numpy(packed).view(-1, 1), state, state.shape, original_lin=lin, **kw)
    wq = torch.from_numpy(o.dequantize_f32(packed, am, 64, M * K)).view(M, K)
    return qd, wq, lin


def test_public_surface_matches_reference_names():
    for name in ["ScalarType", "dequantize_fp4", "dequantize_fp4_codebook_invoke_qtype", "dequantize_fp4_codebook_invoke",
                 "gemm_4bit_inference", "gemm_4bit_inference_qtype", "dequantize_fp4_qtype", "QuantData", "TorchFP4Linear",
                 "swap_linear_with_bnb_linear", "check_if_name_contained_in_list", "todevice_if_necessary",
                 "recursively_replace_with_fp4_linear"]:
        assert hasattr(pkg, name), name
    assert hasattr(pkg.TorchFP4Linear, "from_linear")
    for op in ["dequantize_fp4", "dequantize_fp4_codebook", "gemv_fp4", "qlinear", "qlinear_bias", "qlinear_codebook",
               "qlinear_codebook_bias", "ScalarType"]:
        assert hasattr(pkg.ext, op), op  # reference csrc/torch_fp4.cpp:125-139


def test_scalar_type_enum():
    S = pkg.ScalarType
    assert S.from_torch_dtype(torch.bfloat16) is S.bfloat16 and S.from_str("float16") is S.float16
    assert S.float32.torch_dtype == torch.float32
    assert int(S.float16.value) == 0 and int(S.float32.value) == 1 and int(S.bfloat16.value) == 2  # torch_fp4.cpp:22-26
    with pytest.raises(ValueError):
        S.from_torch_dtype(torch.int8)
    with pytest.raises(ValueError):
        S.from_str("int8")


def test_ext_rejects_cpu_and_noncontiguous_tensors():
    # CHECK_CUDA of the reference (csrc/torch_fp4.cpp:19,42-45) -> RuntimeError
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        pkg.dequantize_fp4(torch.zeros(32, 1, dtype=torch.uint8), torch.ones(1), 64, 8, 8)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        pkg.gemm_4bit_inference(torch.zeros(1, 64), torch.zeros(1, 32, dtype=torch.uint8), torch.ones(1), torch.zeros(16), 64,
                                torch.float32, [1, 64])
    with pytest.raises(TypeError):
        pkg.ext.dequantize_fp4(torch.zeros(32, dtype=torch.uint8), torch.ones(1), 64, 8, 8, 3)  # not a ScalarType


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_dispatch_table(fake, dtype):
    M, K = 128, 256
    qd, wq, lin = make_quant_data(M, K)
    tol = {torch.float32: 1e-5, torch.bfloat16: 6e-2, torch.float16: 1e-2}[dtype]
    gen = torch.Generator().manual_seed(1)
    cases = [((1, K), "gemv_fp4_bias", (1, M)), ((1, 1, K), "gemv_fp4_bias", (1, 1, M)), ((2, K), "qlinear_codebook_bias", (2, M)),
             ((1, 5, K), "qlinear_codebook_bias", (1, 5, M)), ((1, 1, 1, K), "qlinear_codebook_bias", (1, 1, 1, M))]
    for shape, want_call, want_shape in cases:
        fake.calls.clear()
        x = torch.randn(*shape, generator=gen).to(dtype)
        y = qd.forward(x)
        assert fake.calls == [want_call], (shape, fake.calls)
        assert o.expected_dispatch(shape, K, 64) == ("gemv" if "gemv" in want_call else "qlinear")
        assert tuple(y.shape) == want_shape and y.dtype == dtype
        ref = torch.nn.functional.linear(x.float(), wq, lin.bias.float())
        assert (y.float() - ref).abs().max() <= tol * max(1.0, ref.abs().max().item())
    assert qd.o_type == dtype and qd.bias.dtype == dtype  # bias cast on first call (:417-421)
    # empty input -> empty output of the right shape, no op called (:580-589)
    fake.calls.clear()
    assert tuple(qd.forward(torch.empty(0, K, dtype=dtype)).shape) == (0, M) and fake.calls == []
    assert tuple(qd.forward(torch.empty(1, 0, K, dtype=dtype)).shape) == (1, 0, M)


def test_dispatch_non_multiple_of_blocksize_and_non_contiguous(fake):
    # K % blocksize != 0 with a single token falls back to qlinear (:593-594); blocksize 32 makes 96 legal to quantise
    rng = np.random.default_rng(2)
    M, K = 16, 96
    packed, am = o.quantize_fp4(rng.standard_normal(M * K).astype(np.float32), 32)
    state = pkg.QuantState(torch.from_numpy(am), (M, K), torch.from_numpy(o.TREE_TABLE.copy()), 64)  # layer claims bs 64
    qd = pkg.QuantData(torch.from_numpy(packed).view(-1, 1), state, state.shape, original_lin=nn.Linear(K, M, bias=False))
    qd.forward(torch.randn(1, K))
    assert fake.calls == ["qlinear_codebook"]  # = dequant (codebook table) + linear in one extension call
    # non-contiguous single token -> made contiguous, then GEMV (:596-597)
    qd2, wq, lin = make_quant_data(64, 128, bias=False)
    fake.calls.clear()
    x = torch.randn(128, 2)[:, 0].view(1, 128)  # stride 2
    assert not x.is_contiguous()
    y = qd2.forward(x)
    assert fake.calls == ["gemv_fp4"] and torch.allclose(y, x @ wq.t(), atol=1e-4)


def test_unfused_bias_and_tree_and_low_precision_paths(fake):
    qd, wq, lin = make_quant_data(32, 128, fuse_bias=False, use_codebook_dequant=False)
    x = torch.randn(1, 128)
    y = qd.forward(x)
    assert fake.calls == ["gemv_fp4"] and torch.allclose(y, x @ wq.t() + lin.bias, atol=1e-4)
    fake.calls.clear()
    qd.forward(torch.randn(3, 128))
    assert fake.calls == ["qlinear_bias"]  # tree dequant (:456-469) + linear
    fake.calls.clear()
    qd.dequantize()
    assert fake.calls == ["dequantize_fp4"]  # the stand-alone dequantize() of the reference is still there
    for codebook, name in ((True, "qlinear_codebook_bias"), (False, "qlinear_bias")):
        qd2, _, _ = make_quant_data(32, 128, allow_reduced_precision_linear=True, use_codebook_dequant=codebook)
        fake.calls.clear()
        qd2.forward(torch.randn(3, 128))
        assert fake.calls == [name]
    qd3, _, _ = make_quant_data(32, 128, bias=False, allow_reduced_precision_linear=True)
    qd3.bias = None
    fake.calls.clear()
    qd3.forward(torch.randn(3, 128))
    assert fake.calls == ["qlinear_codebook"]


def test_small_batch_opt_in(fake):
    qd, wq, lin = make_quant_data(64, 128, small_batch_fused=True)
    x = torch.randn(3, 128).to(torch.bfloat16)
    y = qd.forward(x)
    assert fake.calls == ["gemm_small_fp4"] and y.shape == (3, 64)
    ref = torch.nn.functional.linear(x.float(), wq, lin.bias.float())
    assert (y.float() - ref).abs().max() <= 6e-2 * max(1.0, ref.abs().max().item())
    fake.calls.clear()
    qd.forward(torch.randn(9, 128).to(torch.bfloat16))  # blocksize 64, K % 64 == 0: fused up to 128 rows
    assert fake.calls == ["gemm_small_fp4"]
    fake.calls.clear()
    qd.forward(torch.randn(129, 128).to(torch.bfloat16))  # more rows: the reference path
    assert fake.calls == ["qlinear_codebook_bias"]
    fake.calls.clear()
    qd.forward(torch.randn(1, 128).to(torch.bfloat16))  # single token is still the GEMV
    assert fake.calls == ["gemv_fp4_bias"]
    # f32 activations: up to 8 rows (one f32 GEMV launch per row inside the op), the reference path above that
    qd32, _, _ = make_quant_data(64, 128, small_batch_fused=True)
    fake.calls.clear()
    assert qd32.forward(torch.randn(8, 128)).shape == (8, 64) and fake.calls == ["gemm_small_fp4"]
    fake.calls.clear()
    qd32.forward(torch.randn(9, 128))
    assert fake.calls == ["qlinear_codebook_bias"]


def test_fused_layers_dispatch_and_fall_back(fake, monkeypatch):
    """torch_bnb_fp4.fused on CPU (oracle-backed ops): row interleaving, the single-token fused call, the unfused fallback for
    batches and for shapes the kernel reports as not covered, residual semantics."""
    from torch_bnb_fp4 import fused

    monkeypatch.setattr(fused, "ext", fake)
    M, K = 32, 128
    rng = np.random.default_rng(3)
    wg, wu = ((rng.standard_normal(M * K) * 0.05).astype(np.float32) for _ in range(2))
    (pg, ag), (pu, au) = o.quantize_fp4(wg, 64), o.quantize_fp4(wu, 64)
    tg = (torch.from_numpy(pg).view(-1, 1), torch.from_numpy(ag))
    tu = (torch.from_numpy(pu).view(-1, 1), torch.from_numpy(au))
    packed, absmax, shape = fused.interleave_rows(tg, tu, (M, K), 64)
    assert shape == (2 * M, K)
    full = o.dequantize_f32(packed.numpy().reshape(-1), absmax.numpy(), 64, 2 * M * K).reshape(2 * M, K)
    assert np.array_equal(full[0::2], o.dequantize_f32(pg, ag, 64, M * K).reshape(M, K))
    assert np.array_equal(full[1::2], o.dequantize_f32(pu, au, 64, M * K).reshape(M, K))
    with pytest.raises(ValueError):
        fused.interleave_rows(tg, tu, (M, K + 64), 64)

    monkeypatch.setattr(fused, "fp4_code", lambda: torch.from_numpy(o.TREE_TABLE.copy()))
    gu = fused.FusedFP4Linear.gate_up_from_packed(tg, tu, (M, K), 64)
    assert gu.out_features == M and gu.in_features == K
    x = torch.randn(1, K).to(torch.bfloat16)
    y = gu(x)
    assert fake.calls == ["gemv_fp4_fused"] and y.shape == (1, M)
    g64 = o.gemv_exact(x.float().numpy().reshape(-1), pg, ag, M, K, 64)
    u64 = o.gemv_exact(x.float().numpy().reshape(-1), pu, au, M, K, 64)
    want = o.silu_mul_epilogue(g64, u64, "bfloat16")
    assert np.array_equal(y.float().numpy().reshape(-1), want)
    # 2..128 rows (blocksize 64, K % 64 == 0): the same epilogue on the small-batch kernels; more rows: the unfused sequence
    # (de-interleaving the rows)
    fake.calls.clear()
    xb = torch.cat([x, x])
    yb = gu(xb)
    assert fake.calls == ["gemm_small_fp4_fused"] and yb.shape == (2, M)
    assert (yb[0].float() - y[0].float()).abs().max() <= 0.05 * max(1.0, y.float().abs().max().item())
    for rows, want_fused in ((40, True), (128, True), (129, False)):
        fake.calls.clear()
        yr = gu(x.repeat(rows, 1))
        assert yr.shape == (rows, M) and ("gemm_small_fp4_fused" in fake.calls) == want_fused, (rows, fake.calls)
        assert "gemv_fp4_fused" not in fake.calls
        assert (yr[7].float() - y[0].float()).abs().max() <= 0.05 * max(1.0, y.float().abs().max().item())
    # plain layer: residual in the epilogue for one token, added separately for a batch
    dn = fused.FusedFP4Linear.from_packed(*tg, (M, K), 64)
    r = torch.randn(1, M).to(torch.bfloat16)
    fake.calls.clear()
    z = dn(x, residual=r)
    assert fake.calls == ["gemv_fp4_fused"]
    assert np.array_equal(z.float().numpy().reshape(-1), o.linear_epilogue(g64, "bfloat16", None, r.float().numpy().reshape(-1)))
    assert dn(xb, residual=torch.cat([r, r])).shape == (2, M)
    # f32 activations: the kernel reports the gated epilogue as not available -> unfused from then on, no error
    gu32 = fused.FusedFP4Linear.gate_up_from_packed(tg, tu, (M, K), 64)
    fake.calls.clear()
    y32 = gu32(x.float())
    assert y32.shape == (1, M) and not gu32._fused_ok and fake.calls[0] == "gemv_fp4_fused" and "gemv_fp4" in fake.calls
    with pytest.raises(ValueError):
        fused.FusedFP4Linear(dn.quant_data, epilogue=5)


def test_the_fused_layers_share_one_forward_ladder():
    from torch_bnb_fp4 import fused

    assert fused.FusedNF4Linear.forward is fused.FusedFP4Linear.forward
    assert fused.LoRANF4Linear.forward is not fused.FusedFP4Linear.forward  # its two-launch sequence is its own


def test_residual_in_kernel_rule_at_its_corners(monkeypatch):
    """The measured exception of the NF4 layers: the plain epilogue with more than 32 rows against rows of 8192 and more weights
    leaves the residual add to torch; every other cell, and the FP4 layer everywhere, adds it in the kernel."""
    from torch_bnb_fp4 import fused

    monkeypatch.setattr(fused, "fp4_code", lambda: torch.from_numpy(o.TREE_TABLE.copy()))
    monkeypatch.setattr(fused, "nf4_code", lambda: torch.from_numpy(o.TREE_TABLE.copy()))
    packed, absmax = torch.zeros(32 * 64 // 2, 1, dtype=torch.uint8), torch.ones(32)
    for epilogue in (fused.EPILOGUE_NONE, fused.EPILOGUE_SILU_MUL_PAIRS):
        fp4 = fused.FusedFP4Linear.from_packed(packed, absmax, (32, 64), 64, epilogue=epilogue)
        nf4 = fused.FusedNF4Linear.from_packed(packed, absmax, (32, 64), 64, epilogue=epilogue)
        for rows in (32, 33):
            for K in (8191, 8192):
                left_to_torch = epilogue == fused.EPILOGUE_NONE and rows == 33 and K == 8192
                assert fp4._residual_in_kernel(rows, K) is True
                assert nf4._residual_in_kernel(rows, K) is (not left_to_torch), (epilogue, rows, K)
                assert fused.LoRANF4Linear._residual_in_kernel(nf4, rows, K) is (not left_to_torch)


def test_surgery_helpers_cpu():
    assert pkg.check_if_name_contained_in_list("model.lm_head", ["lm_head"])
    assert not pkg.check_if_name_contained_in_list("proj", ["lm_head", "pooler"])
    lin = nn.Linear(64, 32)
    fp4 = pkg.swap_linear_with_bnb_linear(lin, dtype=torch.bfloat16)
    assert isinstance(fp4, pkg.LinearFP4) and fp4.weight.quant_state is None
    assert torch.equal(fp4.weight.data, lin.weight.data) and fp4.weight.data.data_ptr() != lin.weight.data.data_ptr()
    assert torch.equal(fp4.bias.data, lin.bias.data) and not fp4.weight.requires_grad and not fp4.bias.requires_grad
    x = torch.randn(3, 64)
    assert torch.allclose(fp4(x), lin(x), atol=1e-6)  # dense until it reaches a GPU
    assert fp4.to(torch.bfloat16).weight.dtype == torch.bfloat16 and isinstance(fp4.weight, pkg.Params4bit)
    with pytest.raises(AssertionError, match="cuda"):
        pkg.recursively_replace_with_fp4_linear(nn.Sequential(lin), device=torch.device("cpu"))
    with pytest.raises(ValueError):
        pkg.TorchFP4Linear(lin)  # not an FP4 layer
    with pytest.raises(ValueError):
        pkg.TorchFP4Linear(fp4)  # FP4 layer type, but not quantised / not on a GPU


def test_product_package_never_imports_the_oracle():
    import os
    import re

    root = os.path.dirname(os.path.abspath(pkg.__file__))
    for dirpath, _, files in os.walk(os.path.dirname(root)):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f
                assert "fp4_oracle" not in text.replace("oracle/fp4_oracle.py", ""), f


def test_bnb_state_keys_match_the_installed_transformers_loader():
    """the on-disk layout is pinned against something other than ourselves - the key patterns the
    installed transformers' pre-quantised bitsandbytes 4-bit loader collects per Linear (quantizer_bnb_4bit.get_weight_conversions;
    importable without bitsandbytes).  What stays 'parity unpinned': the JSON payload of weight.quant_state.bitsandbytes__fp4 -
    a genuine bitsandbytes file carries quant_type, blocksize, dtype, shape (plus nested_blocksize / nested_dtype / nested_offset
    when double quantisation is on, which neither the reference, README.md:223-224, nor this package supports); ours writes the
    same four fields, restated from bitsandbytes' QuantState.as_dict, with no bitsandbytes-written file available to compare."""
    import json
    import types

    from transformers import BitsAndBytesConfig
    from transformers.quantizers.quantizer_bnb_4bit import Bnb4BitHfQuantizer

    conv = Bnb4BitHfQuantizer(BitsAndBytesConfig(load_in_4bit=True, bnb_4bit_quant_type="fp4"), pre_quantized=True).get_weight_conversions()
    assert len(conv) == 1 and conv[0].target_patterns == ["weight"]
    patterns = set(conv[0].source_patterns)
    qd, _, lin = make_quant_data(64, 128)
    qd.bias = lin.bias.detach()
    layer = types.SimpleNamespace(quant_data=qd, bias=qd.bias)
    prefix = "model.layers.0.self_attn.q_proj."
    state = pkg.fp4_linear_to_bnb_state(layer, prefix)
    ours = {k[len(prefix):] for k in state} - {"bias"}
    assert ours <= patterns, ours - patterns                      # every key we write is one the loader collects
    required = {p for p in patterns if "nested" not in p and "nf4" not in p}
    assert ours == required, (ours, required)                     # and we write all of the non-nested FP4 ones
    meta = json.loads(bytes(state[prefix + "weight.quant_state.bitsandbytes__fp4"].tolist()).decode())
    assert meta == {"quant_type": "fp4", "blocksize": 64, "dtype": "float16", "shape": [64, 128]}
    assert state[prefix + "weight"].dtype == torch.uint8 and tuple(state[prefix + "weight"].shape) == (64 * 128 // 2, 1)
    assert state[prefix + "weight.absmax"].dtype == torch.float32 and state[prefix + "weight.quant_map"].numel() == 16


def test_fused_layer_dtype_casts_never_touch_the_scales(fake, monkeypatch):
    """model.half() / .to(torch.bfloat16) / .to(device, dtype) on a model holding FusedFP4Linear layers (fuse_gated_mlps
    followed by the usual cast) must leave the f32 absmax and the packed bytes exactly as they are - in the running layer,
    in state_dict() and after a load_state_dict round trip - as TorchFP4Linear._apply already guarantees."""
    from torch_bnb_fp4 import fused

    monkeypatch.setattr(fused, "ext", fake)
    monkeypatch.setattr(fused, "fp4_code", lambda: torch.from_numpy(o.TREE_TABLE.copy()))
    M, K = 32, 128
    rng = np.random.default_rng(8)
    # scales that do not survive a 16-bit rounding: tiny (fp16 subnormal / flush range) and with a full f32 mantissa
    w = (rng.standard_normal(M * K) * np.repeat(10.0 ** rng.uniform(-7, 0, M * K // 64), 64)).astype(np.float32)
    p, a = o.quantize_fp4(w, 64)
    assert (torch.from_numpy(a).half().float().numpy() != a).any() and (torch.from_numpy(a).bfloat16().float().numpy() != a).any()
    bias = torch.randn(M)

    def fresh():
        return fused.FusedFP4Linear.from_packed(torch.from_numpy(p.copy()).view(-1, 1), torch.from_numpy(a.copy()), (M, K), 64, bias.clone())

    for cast in (lambda m: m.half(), lambda m: m.to(torch.bfloat16), lambda m: m.to("cpu", torch.float16), lambda m: m.float()):
        holder = nn.Sequential(fresh())
        layer = cast(holder)[0]
        for scales in (layer.absmax, layer.quant_data.absmax, layer.state_dict()["absmax"]):
            assert scales.dtype == torch.float32 and np.array_equal(scales.numpy(), a)
        assert layer.qweight.dtype == torch.uint8 and np.array_equal(layer.qweight.numpy().reshape(-1), p)
        assert layer.quant_data.A.data_ptr() == layer.qweight.data_ptr() and layer.quant_data.absmax.data_ptr() == layer.absmax.data_ptr()
        # state_dict round trip into a fresh layer (different scales to start from): bit-identical scales again
        other = fused.FusedFP4Linear.from_packed(torch.zeros(M * K // 2, 1, dtype=torch.uint8), torch.ones(M * K // 64), (M, K), 64, bias.clone())
        other.load_state_dict(layer.state_dict())
        assert other.absmax.dtype == torch.float32 and np.array_equal(other.quant_data.absmax.numpy(), a)
        assert np.array_equal(other.quant_data.A.numpy().reshape(-1), p)
        # and the layer still computes with the exact scales
        x = torch.randn(1, K).to(torch.bfloat16)
        y = layer(x)
        want = o.linear_epilogue(o.gemv_exact(x.float().numpy().reshape(-1), p, a, M, K, 64), "bfloat16", bias.to(torch.bfloat16).float().numpy())
        assert np.array_equal(y.float().numpy().reshape(-1), want)


def test_save_fp4_model_dtype_metadata_and_tensor_parallel_guard(monkeypatch, tmp_path):
    """save_fp4_model: (a) a plain FusedFP4Linear records the dtype its weight was quantised from (its quant_state's), not a
    hard-coded float16; (b) a model holding tensor-parallel wrappers (one rank's shard each) is refused with a clear message instead
    of being written as complete-looking layers of the wrong size that load back without their collective."""
    import json
    import socket

    import torch.distributed as dist
    from safetensors.torch import load_file

    from torch_bnb_fp4 import fused, parallel as par, serialization as ser

    monkeypatch.setattr(fused, "fp4_code", lambda: torch.from_numpy(o.TREE_TABLE.copy()))
    monkeypatch.setattr(par, "fp4_code", lambda: torch.from_numpy(o.TREE_TABLE.copy()))
    M, K = 32, 128
    rng = np.random.default_rng(3)
    p, a = o.quantize_fp4((rng.standard_normal(M * K) * 0.05).astype(np.float32), 64)
    P, A = torch.from_numpy(p).view(-1, 1), torch.from_numpy(a)
    net = nn.Sequential(fused.FusedFP4Linear.from_packed(P, A, (M, K), 64, dtype=torch.bfloat16), fused.FusedFP4Linear.from_packed(P.clone(), A.clone(), (M, K), 64))
    path = str(tmp_path / "m.safetensors")
    ser.save_fp4_model(net, path)
    state = load_file(path)
    meta = [json.loads(bytes(state[f"{i}.weight.quant_state.bitsandbytes__fp4"].tolist()).decode()) for i in (0, 1)]
    assert meta[0]["dtype"] == "bfloat16" and meta[1]["dtype"] == "float16" and meta[0]["shape"] == [M, K]
    assert np.array_equal(state["0.weight"].numpy().reshape(-1), p)
    # from_linear keeps the source layer's recorded dtype
    import types

    src = types.SimpleNamespace(quant_data=net[0].quant_data)
    assert fused.FusedFP4Linear.from_linear(src).quant_data.quant_state.dtype == torch.bfloat16

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        for layer in (par.ColumnParallelFP4Linear(P, A, (M, K), 64), par.RowParallelFP4Linear(P, A, (M, K), 64),
                      par.FusedColumnParallelFP4([(P, A, (M, K)), (P, A, (M, K))], 64)):
            with pytest.raises(ValueError, match="one rank's shard"):
                ser.save_fp4_model(nn.Sequential(nn.Linear(4, 4), layer), str(tmp_path / "tp.safetensors"))
    finally:
        dist.destroy_process_group()


def test_tools_and_bench_keep_away_from_the_oracle():
    """The oracle is test infrastructure: besides tests/, only __graft_entry__.smoke() and bench.py's `cpu_baseline` leg may touch it.
    tools/ (sweeps, decode harnesses, experiments) must not import it at all; bench.py exactly once, inside cpu_baseline()."""
    import ast
    import os

    repo = os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__)))
    repo = os.path.dirname(repo) if os.path.basename(repo) == "torch-bnb-fp4_amd" else repo
    tools = os.path.join(repo, "tools")

    def oracle_imports(path):
        found = []
        tree = ast.parse(open(path).read())
        parents = {}
        for node in ast.walk(tree):
            for child in ast.iter_child_nodes(node):
                parents[child] = node
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            if any(n == "oracle" or n.startswith("oracle.") for n in names):
                fn = node
                while fn in parents and not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    fn = parents[fn]
                found.append(fn.name if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)) else "<module>")
        return found

    for f in sorted(os.listdir(tools)):
        if f.endswith(".py"):
            assert oracle_imports(os.path.join(tools, f)) == [], f
    assert oracle_imports(os.path.join(repo, "bench.py")) == ["cpu_baseline"]


def test_a_missing_or_broken_stream_probe_never_fails_the_build(monkeypatch, tmp_path, capsys):
    """tools/stream_probe.hip is bench.py's measuring stick, not the product: build_all() (test session, __graft_entry__.build()) carries
    on without it, and packaging (setup.py) does not ask for it at all."""
    import importlib.util

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fp4_build_probe_test", os.path.join(repo, "torch-bnb-fp4_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "build_hip_lib", lambda force=False: mod.HIP_LIB)
    monkeypatch.setattr(mod, "build_torch_ext", lambda force=False: mod.EXT_LIB)
    monkeypatch.setattr(mod, "PROBE_SRC", str(tmp_path / "absent.hip"))
    assert mod.build_all() == [mod.HIP_LIB, mod.EXT_LIB] and "absent" in capsys.readouterr().err
    broken = tmp_path / "broken.hip"
    broken.write_text("this is not HIP\n")
    monkeypatch.setattr(mod, "PROBE_SRC", str(broken))
    monkeypatch.setattr(mod, "PROBE_LIB", str(tmp_path / "libprobe.so"))
    assert mod.build_all() == [mod.HIP_LIB, mod.EXT_LIB] and "did not build" in capsys.readouterr().err
    assert mod.build_all(probe=False) == [mod.HIP_LIB, mod.EXT_LIB]
    assert "build_all(probe=False)" in open(os.path.join(repo, "torch-bnb-fp4_amd", "setup.py")).read()
