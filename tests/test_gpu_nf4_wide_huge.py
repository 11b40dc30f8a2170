"""fp4_hip_gemm_wide_nf4 past 2^32 weights: the kernel addresses the packed bytes and the scales with 64-bit offsets, so M * K >= 2^32
is served, not refused.  One weight of 2^32 + 17 K elements (a row tail past the workgroup's 32 rows included) at row counts above 16;
rows on either side of every 2^31 / 2^32-element and 2^31-byte boundary, the first and last rows and a random sample are held to the
bar of tests/test_gpu_nf4_wide_batch.py against the numpy restatement (nf4_ref.gemv_exact)."""
import numpy as np
import pytest
import torch

import nf4_ref as R
from gpu_util import HALF_ULP, dev
from test_gpu_nf4_wide_batch import BS, gemm

pytestmark = pytest.mark.gpu
K = 16384


def test_gemm_wide_nf4_beyond_2_pow_32_weights():
    M = (1 << 32) // K + 17
    assert M * K >= 2**32 and M % 32 != 0
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip("needs ~8 GiB of free device memory")
    g = torch.Generator(device=dev()).manual_seed(20260107)
    packed = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev(), generator=g)
    absmax = torch.rand(M * K // BS, device=dev(), generator=g) * 0.05 + 0.005
    marks = [0, 1, 15, 16, 31, 32, M - 18, M - 17, M - 16, M - 2, M - 1]
    marks += [e // K + d for e in (1 << 31, 1 << 32, 3 << 30, 1 << 33) for d in (-1, 0, 1) if e // K + d < M]  # element and byte offsets
    rows = np.unique(np.concatenate([np.array(marks), np.random.default_rng(5).integers(0, M, 40)]))
    idx = torch.from_numpy(rows).to(dev())
    p_rows = packed.view(M, K // 2)[idx].cpu().numpy().reshape(-1)
    a_rows = absmax.view(M, K // BS)[idx].cpu().numpy().reshape(-1)
    for dtype, B in ((torch.bfloat16, 17), (torch.float16, 80)):
        x = torch.randn(B, K, device=dev(), generator=g).to(dtype)
        bias = (torch.randn(M, device=dev(), generator=g) * 0.1).to(dtype)
        y = gemm(x, packed, absmax, M, K, bias=bias)
        assert torch.isfinite(y).all()
        got = y[:, idx].double().cpu().numpy()
        b_rows = bias[idx].double().cpu().numpy()
        for b in sorted({0, 1, 15, 16, B // 2 - 1, B // 2, B - 1}):
            exact, scale = R.gemv_exact(x[b].double().cpu().numpy(), p_rows, a_rows, len(rows), K, BS)
            exact = exact + b_rows
            tol = 1.01 * HALF_ULP[dtype] * np.abs(exact) + 1e-5 * scale + 1e-30
            err = np.abs(got[b] - exact)
            assert (err <= tol).all(), (dtype, b, int((err > tol).sum()), float((err / tol).max()), rows[int((err / tol).argmax())])
        del y
    del packed, absmax
    torch.cuda.empty_cache()
