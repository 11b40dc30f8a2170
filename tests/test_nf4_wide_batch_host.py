"""Host-side checks of the NF4 wide-batch path (no GPU): the routing of QuantData / set_small_batch_fused with both NF4 switches in
every combination, the dispatcher's cells under the restated rule of tests/nf4_wide_cases.py, the header and the build recipe."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import nf4_ref as R
import nf4_wide_cases as C
import torch_bnb_fp4.functional as F_mod
import torch_bnb_fp4.quant_data as qd_mod
from test_nf4_small_batch_host import RecordingSmallExt, _nf4_qd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RecordingWideExt(RecordingSmallExt):
    """RecordingSmallExt plus the new op."""

    def gemm_wide_nf4(self, A, B, absmax, blocksize, Bshape, bias):
        self.calls.append("gemm_wide_nf4")
        M, K = Bshape
        assert A.is_contiguous() and A.shape[-1] == K and tuple(B.shape) == (1, M * K // 2)
        w = self._w(B, absmax, M, K, blocksize)
        return torch.nn.functional.linear(A.float(), w, None if bias is None else bias.float()).to(A.dtype)


@pytest.fixture()
def rec(monkeypatch):
    r = RecordingWideExt()
    monkeypatch.setattr(F_mod, "ext", r)
    monkeypatch.setattr(qd_mod, "ext", r)
    return r


# ---- routing -----------------------------------------------------------------------------------------------------------------------------
def expected_route(rows, K, small, wide, bias=True):
    """The table of the issue: one row is the GEMV; 2..16 rows belong to the small-batch switch where K % 512 == 0 and to the wide
    switch where it is not; 17..64 rows belong to the wide switch (65..128, two passes of the kernel, measured slower than dequant +
    GEMM and are left there: profiles/nf4_wide_batch.json); everything else is dequant + GEMM."""
    b = "_bias" if bias else ""
    if rows == 1:
        return "gemv_nf4" + b
    if small and 2 <= rows <= 16 and K % 512 == 0:
        return "gemm_small_nf4"
    if wide and K % 64 == 0 and (17 <= rows <= 64 or (2 <= rows <= 16 and K % 512 != 0)):
        return "gemm_wide_nf4"
    return "qlinear_nf4" + b


@pytest.mark.parametrize("small,wide", list(itertools.product([False, True], repeat=2)))
@pytest.mark.parametrize("K", [1024, 576])
def test_both_switches_in_every_combination(rec, small, wide, K):
    M = 32
    for dtype in (torch.bfloat16, torch.float16):  # a QuantData fixes its compute dtype at the first call: one per dtype
        qd = _nf4_qd(M, K, small_batch_fused_nf4=small, wide_batch_fused_nf4=wide)
        assert qd.small_batch_fused_nf4 is small and qd.wide_batch_fused_nf4 is wide
        w = R.dequantize_f32(qd.A.numpy().ravel(), qd.absmax.numpy(), 64, M * K).reshape(M, K).astype(np.float64)
        for shape in [(2, K), (1, K), (1, 1, K), (16, K), (4, 4, K), (17, K), (3, 6, K), (64, K), (65, K), (128, K), (4, 32, K), (129, K),
                      (200, K)]:
            rows = int(np.prod(shape[:-1]))
            rec.calls.clear()
            x = torch.randn(*shape).to(dtype)
            y = qd.forward(x)
            assert rec.calls == [expected_route(rows, K, small, wide)], (shape, small, wide)
            assert tuple(y.shape) == shape[:-1] + (M,) and y.dtype == dtype
            ref = x.double().numpy() @ w.T + qd.bias.double().numpy()
            np.testing.assert_allclose(y.double().numpy(), ref, rtol=2e-2, atol=2e-2 * np.abs(ref).max())
        assert tuple(qd.forward(torch.empty(0, K).to(dtype)).shape) == (0, M)


def test_default_is_off_and_the_old_switches_alone_change_nothing_above_16_rows(rec):
    qd = _nf4_qd(32, 512, small_batch_fused=True, small_batch_fused_nf4=True)
    assert qd.wide_batch_fused_nf4 is False
    for rows in (17, 64, 128, 200):
        rec.calls.clear()
        qd.forward(torch.randn(rows, 512).to(torch.bfloat16))
        assert rec.calls == ["qlinear_nf4_bias"], rows


def test_switch_on_leaves_uncovered_inputs_where_they_were(rec):
    for kw, K, x in [(dict(), 96, torch.randn(20, 96).to(torch.bfloat16)),                 # K % 64 != 0 (blocksize 32)
                     (dict(blocksize=128), 1024, torch.randn(20, 1024).to(torch.float16)),   # blocksize != 64
                     (dict(), 1024, torch.randn(20, 1024)),                                  # f32 activations
                     (dict(), 1024, torch.randn(65, 1024).to(torch.bfloat16))]:              # more than 64 rows
        rec.calls.clear()
        if K == 96:
            kw = dict(blocksize=32)
        qd = _nf4_qd(16, K, wide_batch_fused_nf4=True, **kw)
        qd.forward(x)
        assert rec.calls == ["qlinear_nf4_bias"], (kw, K, x.dtype, x.shape)
    rec.calls.clear()
    qd = _nf4_qd(16, 1024, bias=False, wide_batch_fused_nf4=True)
    qd.forward(torch.randn(40, 1024).to(torch.float16))
    assert rec.calls == ["gemm_wide_nf4"]


def test_an_fp4_weight_ignores_the_switch(rec):
    from torch_bnb_fp4.nn import QuantState

    M, K = 16, 1024
    state = QuantState(absmax=torch.ones(M * K // 64), shape=torch.Size([M, K]), code=torch.zeros(16), blocksize=64, quant_type="fp4",
                       dtype=torch.float32)
    qd = qd_mod.QuantData(torch.zeros(M * K // 2, 1, dtype=torch.uint8), state, state.shape, use_codebook_dequant=False,
                          allow_reduced_precision_linear=True, wide_batch_fused_nf4=True)
    assert not qd.nf4
    qd.forward(torch.randn(40, K).to(torch.bfloat16))
    assert rec.calls == ["qlinear"]


def test_set_small_batch_fused_sets_the_wide_switch_only_when_asked():
    import torch_bnb_fp4 as pkg
    from torch import nn
    from torch_bnb_fp4.nn import QuantState

    def shell(qd):  # a TorchFP4Linear around a host-side QuantData (its constructor wants a weight on the GPU)
        layer = pkg.TorchFP4Linear.__new__(pkg.TorchFP4Linear)
        nn.Module.__init__(layer)
        layer.quant_data = qd
        return layer

    state = QuantState(absmax=torch.ones(32), shape=torch.Size([32, 64]), code=torch.zeros(16), blocksize=64, quant_type="fp4",
                       dtype=torch.float32)
    fp4 = qd_mod.QuantData(torch.zeros(32 * 64 // 2, 1, dtype=torch.uint8), state, state.shape)
    nf4 = _nf4_qd(32, 64)
    root = nn.Sequential(shell(nf4), nn.ReLU(), shell(fp4))
    # the calls that exist today: same counts, the new switch untouched
    assert pkg.set_small_batch_fused(root) == 1 and not nf4.wide_batch_fused_nf4
    assert pkg.set_small_batch_fused(root, True, nf4=True) == 2 and nf4.small_batch_fused_nf4 and not nf4.wide_batch_fused_nf4
    assert pkg.set_small_batch_fused(root, False, nf4=True) == 2 and not nf4.small_batch_fused_nf4
    # the new argument
    assert pkg.set_small_batch_fused(root, True, nf4_wide=True) == 2
    assert nf4.wide_batch_fused_nf4 and not nf4.small_batch_fused_nf4 and not fp4.wide_batch_fused_nf4 and fp4.small_batch_fused
    assert pkg.set_small_batch_fused(root, True, nf4=True, nf4_wide=True) == 2 and nf4.wide_batch_fused_nf4 and nf4.small_batch_fused_nf4
    assert pkg.set_small_batch_fused(root, False, nf4_wide=True) == 2 and not nf4.wide_batch_fused_nf4 and nf4.small_batch_fused_nf4


# ---- the dispatcher's cells ----------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_dispatch_cell():
    """tests/test_gpu_nf4_wide_batch.py runs C.SHAPES x C.rows_for(K): under the restated rule they reach all 16 (column tiles, row
    tiles per workgroup, blocks per wave) cells, the forwarded cell is NOT among them (test 6 of the GPU file covers it), both
    chunkings occur, and there are ragged and full last passes for both blocks-per-wave."""
    seen = {}
    for M, K in C.SHAPES:
        for B in C.rows_for(K):
            for c in C.cells(B, M, K):
                seen.setdefault(c, (B, M, K))
    assert set(seen) == C.ALL_CELLS and len(C.ALL_CELLS) == 16, sorted(C.ALL_CELLS - set(seen))
    assert C.chunks(64) == [64] and C.chunks(65) == [33, 32] and C.chunks(127) == [64, 63] and C.chunks(128) == [64, 64] and C.chunks(17) == [17]
    assert C.cells(16, 64, 512) == ["small"] and C.cells(16, 64, 576) == [(1, 1, 1)] and C.cells(17, 64, 512) == [(2, 1, 4)]
    ragged = {(4 if K % 256 == 0 else 1, C.ragged_last_pass(K)) for _, K in C.SHAPES}
    assert ragged == {(1, True), (4, True), (4, False)}  # one block per wave: K = 64, 320, 576, each short of eight units
    assert {K for _, K in C.SHAPES} >= {64, 4096, 11008, 14336}
    assert any(M < 16 for M, _ in C.SHAPES) and any(M % 16 for M, _ in C.SHAPES) and any(M % 32 and M >= 6144 for M, _ in C.SHAPES)
    assert set(C.ROWS_WIDE) == {17, 18, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 127, 128} and set(C.ROWS_SMALL) == {1, 2, 5, 16}


def test_the_kernel_source_states_the_restated_rule():
    text = open(os.path.join(REPO, "torch-bnb-fp4_amd", "csrc", "gemm_wide_nf4.hip")).read()
    assert "M >= 24 * device_cu_count()" in text
    assert "K % 256 == 0" in text
    assert "B > 64 ? (B + 1) / 2 : B" in text
    assert "B <= 16 && K % 512 == 0" in text
    assert "atomicAdd" not in text and "hipMalloc" not in text and "Synchronize" not in text


# ---- header and build recipe ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_under_abi_version_7():
    text = open(os.path.join(REPO, "include", "torch_bnb_fp4_hip.h")).read()
    assert re.search(r"#define\s+FP4_HIP_ABI_VERSION\s+7\b", text)
    m = re.search(r"FP4_HIP_API\s+int\s+fp4_hip_gemm_wide_nf4\s*\(([^;]*)\)\s*;", text)
    assert m, "fp4_hip_gemm_wide_nf4 is not declared"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["const void *x", "const uint8_t *packed", "const float *absmax", "const void *bias", "void *out", "int64_t B",
                    "int64_t M", "int64_t K", "int blocksize", "int dtype", "void *stream"]


def test_the_new_source_is_built_and_its_kernels_are_tied_to_it():
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("fp4_build_for_nf4_wide", os.path.join(REPO, "torch-bnb-fp4_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "gemm_wide_nf4.hip" in build.HIP_SOURCES and "gemm_small_nf4.hip" in build.HIP_SOURCES
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import source_digest
    finally:
        sys.path.pop(0)
    files = source_digest.sources_of("gemm_wide_nf4_kernel<2, 4, 1, 4>")
    assert files and any(f.endswith("gemm_wide_nf4.hip") for f in files) and not any(f.endswith("gemm_small_nf4.hip") for f in files)
    small = source_digest.sources_of("gemm_nf4_mfma_kernel<2, 4, 4>")
    assert any(f.endswith("gemm_small_nf4.hip") for f in small) and not any(f.endswith("gemm_wide_nf4.hip") for f in small)
    assert any(f.endswith("gemm_wide_fp4.hip") for f in source_digest.sources_of("gemm16_wide_ring_kernel<2, 4, 4>"))
    # the shared headers: rebuilt on an edit, and among the sources of the matrix-core kernels that include them - and of no other
    assert {"mfma_common.h", "nf4_mfma.h", "launchers.h"} <= set(build.HIP_HEADERS)
    names = lambda kernel: {os.path.basename(f) for f in source_digest.sources_of(kernel)}
    assert {"mfma_common.h", "nf4_mfma.h"} <= names("gemm_wide_nf4_kernel<2, 4, 1, 4>")
    for fp4_kernel in ("gemm16_wide_ring_kernel<2, 4, 4>", "gemm16_xstat_kernel<2, 4>", "splitk_reduce_kernel<2>"):
        assert "mfma_common.h" in names(fp4_kernel) and "nf4_mfma.h" not in names(fp4_kernel)
    for other in ("gemv16_regx_kernel<2, 4>", "dequant_tiles_kernel<2>"):
        assert not {"mfma_common.h", "nf4_mfma.h"} & names(other), other
