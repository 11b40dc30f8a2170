"""Host-side checks of the NF4 small-batch path (no GPU): the hi/lo split of the codes that csrc/gemm_small_nf4.hip feeds to the
matrix cores, the routing of QuantData / set_small_batch_fused, and the header."""
import os
import re

import numpy as np
import pytest
import torch

import nf4_ref as R
import torch_bnb_fp4.functional as F_mod
import torch_bnb_fp4.quant_data as qd_mod
from test_nf4_host import RecordingNf4Ext

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the split ---------------------------------------------------------------------------------------------------------------------------
def split(dtype, shift=0):
    """hi = T(code), lo = T((code - hi) * 2^shift) as float64, with torch's RNE conversions (code - hi is exact in f32)."""
    c = torch.from_numpy(R.CODE)
    hi = c.to(dtype).float()
    lo = ((c - hi) * float(2**shift)).to(dtype).float()
    return hi.double().numpy(), lo.double().numpy()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_hi_plus_lo_represents_every_code_to_1e_5_and_hi_alone_does_not(dtype):
    """Why the kernel issues two matrix instructions per k-set: 1e-5 * sum |x w| is the bar's slack beside the final rounding."""
    code = R.CODE.astype(np.float64)
    hi, lo = split(dtype)
    nz = code != 0
    both = np.abs(hi + lo - code)[nz] / np.abs(code)[nz]
    alone = np.abs(hi - code)[nz] / np.abs(code)[nz]
    assert both.max() < 1e-5
    assert alone.max() > 1e-4
    assert both.max() == pytest.approx({torch.bfloat16: 5.45e-6, torch.float16: 1.05e-7}[dtype], rel=0.01)
    assert hi[7] == 0 and lo[7] == 0 and lo[0] == 0 and lo[15] == 0  # 0 and +-1 are exact


def test_fp16_lo_is_mostly_subnormal_and_the_scaled_table_is_not():
    """fp16's smallest normal is 2^-14: eight of the thirteen non-zero lo values lie below it (nibbles 4-6 and 8-12).  The kernel
    therefore stores lo * 2^24 (all normal, none above 4096) and folds 2^-24 in after the matrix instructions, with no loss."""
    _, lo = split(torch.float16)
    sub = [n for n in range(16) if 0 < abs(lo[n]) < 2.0**-14]
    assert sub == [4, 5, 6, 8, 9, 10, 11, 12]
    assert np.abs(lo).max() < 2.0**-12
    hi, lo_scaled = split(torch.float16, shift=24)
    nzl = lo_scaled != 0
    assert nzl.sum() == 13 and np.abs(lo_scaled[nzl]).min() >= 2.0**-14 and np.abs(lo_scaled).max() <= 4096
    code = R.CODE.astype(np.float64)
    nz = code != 0
    assert (np.abs(hi + lo_scaled * 2.0**-24 - code)[nz] / np.abs(code)[nz]).max() < 1.1e-7
    # bf16 has f32's exponent range: no lo comes anywhere near its smallest normal
    _, lo_bf = split(torch.bfloat16)
    assert np.abs(lo_bf[lo_bf != 0]).min() > 1e-30


# ---- routing -----------------------------------------------------------------------------------------------------------------------------
class RecordingSmallExt(RecordingNf4Ext):
    """RecordingNf4Ext plus the new op (and the FP4 small-batch op, for the FP4 QuantData below)."""

    def gemm_small_nf4(self, A, B, absmax, blocksize, Bshape, bias):
        self.calls.append("gemm_small_nf4")
        M, K = Bshape
        assert A.is_contiguous() and A.shape[-1] == K and tuple(B.shape) == (1, M * K // 2)
        w = self._w(B, absmax, M, K, blocksize)
        return torch.nn.functional.linear(A.float(), w, None if bias is None else bias.float()).to(A.dtype)

    def gemm_small_fp4(self, A, B, absmax, blocksize, Bshape, bias):
        self.calls.append("gemm_small_fp4")
        return torch.zeros(A.shape[:-1] + (Bshape[0],), dtype=A.dtype)

    def qlinear(self, A_in, A, absmax, M, N, blocksize):
        self.calls.append("qlinear")
        return torch.zeros(A_in.shape[:-1] + (M,), dtype=A_in.dtype)

    qlinear_codebook = None


@pytest.fixture()
def rec(monkeypatch):
    r = RecordingSmallExt()
    monkeypatch.setattr(F_mod, "ext", r)
    monkeypatch.setattr(qd_mod, "ext", r)
    return r


def _nf4_qd(M, K, blocksize=64, bias=True, **kw):
    from torch_bnb_fp4.nn import QuantState, nf4_code

    rng = np.random.default_rng(M + K)
    packed, absmax = R.quantize(rng.standard_normal(M * K).astype(np.float32), blocksize)
    state = QuantState(absmax=torch.from_numpy(absmax), shape=torch.Size([M, K]), code=nf4_code(), blocksize=blocksize, quant_type="nf4",
                       dtype=torch.float32)
    return qd_mod.QuantData(torch.from_numpy(packed).view(-1, 1), state, state.shape, bias=torch.randn(M) * 0.1 if bias else None,
                            allow_reduced_precision_linear=True, **kw)


def test_default_is_off_and_the_old_switch_still_does_nothing_for_nf4(rec):
    qd = _nf4_qd(32, 512, small_batch_fused=True)
    assert qd.small_batch_fused_nf4 is False
    for rows in (2, 8, 16, 200):
        rec.calls.clear()
        qd.forward(torch.randn(rows, 512).to(torch.bfloat16))
        assert rec.calls == ["qlinear_nf4_bias"], rows


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_switch_on_routes_2_to_16_rows_of_a_supported_shape(rec, dtype):
    qd = _nf4_qd(32, 1024, small_batch_fused_nf4=True)
    w = R.dequantize_f32(qd.A.numpy().ravel(), qd.absmax.numpy(), 64, 32 * 1024).reshape(32, 1024).astype(np.float64)
    for shape, want in [((1, 1024), "gemv_nf4_bias"), ((1, 1, 1024), "gemv_nf4_bias"), ((2, 1024), "gemm_small_nf4"),
                        ((3, 1024), "gemm_small_nf4"), ((16, 1024), "gemm_small_nf4"), ((2, 4, 1024), "gemm_small_nf4"),
                        ((4, 4, 1024), "gemm_small_nf4"), ((17, 1024), "qlinear_nf4_bias"), ((200, 1024), "qlinear_nf4_bias"),
                        ((3, 6, 1024), "qlinear_nf4_bias")]:
        rec.calls.clear()
        x = torch.randn(*shape).to(dtype)
        y = qd.forward(x)
        assert rec.calls == [want], shape
        assert tuple(y.shape) == shape[:-1] + (32,) and y.dtype == dtype
        ref = x.double().numpy() @ w.T + qd.bias.double().numpy()
        np.testing.assert_allclose(y.double().numpy(), ref, rtol=2e-2, atol=2e-2)
    rec.calls.clear()
    qd.bias = None
    qd.forward(torch.randn(5, 1024).to(dtype))
    assert rec.calls == ["gemm_small_nf4"]
    assert tuple(qd.forward(torch.empty(0, 1024).to(dtype)).shape) == (0, 32)


def test_switch_on_leaves_uncovered_inputs_where_they_were(rec):
    # K % 512 != 0
    qd = _nf4_qd(16, 576, small_batch_fused_nf4=True)
    qd.forward(torch.randn(4, 576).to(torch.bfloat16))
    assert rec.calls == ["qlinear_nf4_bias"]
    # blocksize != 64
    rec.calls.clear()
    qd = _nf4_qd(16, 1024, blocksize=128, small_batch_fused_nf4=True)
    qd.forward(torch.randn(4, 1024).to(torch.float16))
    assert rec.calls == ["qlinear_nf4_bias"]
    # f32 activations
    rec.calls.clear()
    qd = _nf4_qd(16, 1024, small_batch_fused_nf4=True)
    qd.forward(torch.randn(4, 1024))
    assert rec.calls == ["qlinear_nf4_bias"]


def test_an_fp4_weight_ignores_the_nf4_switch(rec):
    from torch_bnb_fp4.nn import QuantState

    M, K = 16, 1024
    state = QuantState(absmax=torch.ones(M * K // 64), shape=torch.Size([M, K]), code=torch.zeros(16), blocksize=64, quant_type="fp4",
                       dtype=torch.float32)
    packed = torch.zeros(M * K // 2, 1, dtype=torch.uint8)
    qd = qd_mod.QuantData(packed, state, state.shape, use_codebook_dequant=False, allow_reduced_precision_linear=True,
                          small_batch_fused_nf4=True)
    assert not qd.nf4
    qd.forward(torch.randn(4, K).to(torch.bfloat16))
    assert rec.calls == ["qlinear"]
    rec.calls.clear()
    qd.small_batch_fused = True
    qd.forward(torch.randn(4, K).to(torch.bfloat16))
    assert rec.calls == ["gemm_small_fp4"]


def test_set_small_batch_fused_counts_fp4_and_nf4_layers_only_when_asked():
    import torch_bnb_fp4 as pkg
    from torch import nn

    def shell(qd):  # a TorchFP4Linear around a host-side QuantData (its constructor wants a weight on the GPU)
        layer = pkg.TorchFP4Linear.__new__(pkg.TorchFP4Linear)
        nn.Module.__init__(layer)
        layer.quant_data = qd
        return layer

    from torch_bnb_fp4.nn import QuantState

    state = QuantState(absmax=torch.ones(32 * 64 // 64), shape=torch.Size([32, 64]), code=torch.zeros(16), blocksize=64, quant_type="fp4",
                       dtype=torch.float32)
    fp4 = qd_mod.QuantData(torch.zeros(32 * 64 // 2, 1, dtype=torch.uint8), state, state.shape)
    nf4 = _nf4_qd(32, 64)
    root = nn.Sequential(shell(nf4), nn.ReLU(), shell(fp4), nn.Linear(64, 8))
    assert nf4.nf4 and not fp4.nf4
    assert pkg.set_small_batch_fused(root) == 1
    assert fp4.small_batch_fused and not nf4.small_batch_fused and not nf4.small_batch_fused_nf4 and not fp4.small_batch_fused_nf4
    assert pkg.set_small_batch_fused(root, True, nf4=True) == 2
    assert fp4.small_batch_fused and nf4.small_batch_fused_nf4 and not nf4.small_batch_fused and not fp4.small_batch_fused_nf4
    assert pkg.set_small_batch_fused(root, False, nf4=True) == 2
    assert not fp4.small_batch_fused and not nf4.small_batch_fused_nf4
    assert pkg.set_small_batch_fused(nn.Sequential(root[0]), True) == 0 and not nf4.small_batch_fused_nf4


# ---- header and build recipe ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_under_abi_version_7():
    text = open(os.path.join(REPO, "include", "torch_bnb_fp4_hip.h")).read()
    assert re.search(r"#define\s+FP4_HIP_ABI_VERSION\s+7\b", text)
    m = re.search(r"FP4_HIP_API\s+int\s+fp4_hip_gemm_small_nf4\s*\(([^;]*)\)\s*;", text)
    assert m, "fp4_hip_gemm_small_nf4 is not declared"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const void *x", "const uint8_t *packed", "const float *absmax", "const void *bias", "void *out", "int64_t B",
                    "int64_t M", "int64_t K", "int blocksize", "int dtype", "void *stream"]


def test_the_new_source_is_built_and_its_kernels_are_tied_to_it():
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("fp4_build_for_nf4_small", os.path.join(REPO, "torch-bnb-fp4_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "gemm_small_nf4.hip" in build.HIP_SOURCES
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import source_digest
    finally:
        sys.path.pop(0)
    files = source_digest.sources_of("gemm_nf4_mfma_kernel<2, 4, 4>")
    assert files and any(f.endswith("gemm_small_nf4.hip") for f in files)
    assert not any(f.endswith("gemm_small_fp4.hip") for f in files)
    assert any(f.endswith("gemm_small_fp4.hip") for f in source_digest.sources_of("gemm16_mfma_kernel<2, 4, 1, 4>"))
    # the shared headers: rebuilt on an edit, and among the sources of the matrix-core kernels that include them - and of no other
    assert {"mfma_common.h", "nf4_mfma.h", "launchers.h"} <= set(build.HIP_HEADERS)
    names = lambda kernel: {os.path.basename(f) for f in source_digest.sources_of(kernel)}
    assert {"mfma_common.h", "nf4_mfma.h"} <= names("gemm_nf4_mfma_kernel<2, 4, 4>")
    for fp4_kernel in ("gemm16_mfma_kernel<2, 4, 1, 4>", "gemm16_small_kernel<2, 4>"):
        assert "mfma_common.h" in names(fp4_kernel) and "nf4_mfma.h" not in names(fp4_kernel)
    for other in ("gemv16_regx_kernel<2, 4>", "gemv_nf4_kernel<2, 4>", "dequant_tiles_kernel<2>", "quantize_nf4_kernel<2>", "lora_down_kernel<2>"):
        assert not {"mfma_common.h", "nf4_mfma.h"} & names(other), other
    # the wave-private LDS images: the header of the three translation units that stage through them, and of no other
    assert "wave_image.h" in build.HIP_HEADERS
    for image_kernel in ("gemm_nf4_mfma_kernel<2, 4, 4>", "gemm_wide_nf4_kernel<2, 4, 1, 4>", "gemm16_mfma_kernel<2, 4, 1, 4>"):
        assert "wave_image.h" in names(image_kernel), image_kernel
    for other in ("gemv16_regx_kernel<2, 4>", "gemv_nf4_kernel<2, 4>", "dequant_tiles_kernel<2>", "quantize_nf4_kernel<2>", "lora_down_kernel<2>",
                  "gemm16_wide_ring_kernel<2, 4>"):
        assert "wave_image.h" not in names(other), other
