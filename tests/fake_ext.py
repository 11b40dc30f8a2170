"""A CPU test double for ``torch_bnb_fp4_ext``: same op names and signatures, computed with the
oracle, recording which op was called.  Lets the host-side dispatch logic be tested without a GPU."""
from __future__ import annotations

import functools
import json
import os
import re

import numpy as np
import torch

from oracle import fp4_oracle as o

_NP = {torch.float16: "float16", torch.float32: "float32", torch.bfloat16: "bfloat16"}


def _to_torch(arr: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    if dtype == torch.bfloat16:
        return torch.from_numpy(arr.astype(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(arr.copy())


# ---- strict mode: the C ABI's refusals of an operand's ADDRESS and of a block size, for any CPU double ---------------------------------
# The doubles (FakeExt below and the ones local to the *_host.py files) accept any address, so a layer that hands a fused op an
# activation the C entry point would refuse passes its host test and raises on the GPU.  Strict(double) is the opt-in strict mode:
# the same double, with every op whose entry point refuses a 16-bit activation off a 16-byte boundary, or a block size it does not
# cover, raising RuntimeError as the extension does - the text recorded in tests/golden/*_entry_refusals.json with the call's own
# numbers in it.  Ops without a rule (the plain GEMVs and dequant + GEMM take any address) pass through.
# The predicate of strict_refusal() is an APPROXIMATION of nf4_check_args (csrc/nf4_call.h) and gemm_small_entry
# (csrc/gemm_small_fp4.hip), not a copy: it knows the alignment of x, the block size and K's divisibility by the block - what a layer's
# routing can get wrong - and leaves out what each entry point adds (K % 512 for gemm_small_nf4, the row limits, size bounds, the
# operands other than x).  The recorded texts pin its wording; tests/test_*_entry_refusals_host.py pin the entry points themselves.
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_DT_CODE = {torch.float16: 0, torch.float32: 1, torch.bfloat16: 2}
# op -> (kind, C entry point, index of `blocksize` among the op's arguments; Bshape follows it)
STRICT_RULES = {
    "gemm_small_fp4": ("small_fp4", "fp4_hip_gemm_small", 3), "gemm_small_fp4_fused": ("small_fp4", "fp4_hip_gemm_small_fused", 3),
    "gemv_fp4_fused": ("gemv_fp4_gated", "fp4_hip_gemv_fused", 3),
    "gemv_nf4_fused": ("nf4_gemv", "fp4_hip_gemv_fused_nf4", 3), "gemv_nf4_lora": ("nf4_gemv", "fp4_hip_gemv_lora_nf4", 3),
    "gemv_nf4_lora_multi": ("nf4_gemv", "fp4_hip_gemv_lora_multi_nf4", 3), "gemv_nf4_nested": ("nf4_gemv", "fp4_hip_gemv_nested_nf4", 7),
    "gemv_nf4_lora_nested": ("nf4_gemv", "fp4_hip_gemv_lora_nested_nf4", 7),
    "gemm_small_nf4": ("nf4_gemm", "fp4_hip_gemm_small_nf4", 3), "gemm_wide_nf4": ("nf4_gemm", "fp4_hip_gemm_wide_nf4", 3),
    "gemm_nf4_fused": ("nf4_gemm", "fp4_hip_gemm_fused_nf4", 3), "gemm_nf4_lora": ("nf4_gemm", "fp4_hip_gemm_lora_nf4", 3),
    "gemm_nf4_lora_multi": ("nf4_gemm", "fp4_hip_gemm_lora_multi_nf4", 3), "gemm_nf4_nested": ("nf4_gemm", "fp4_hip_gemm_nested_nf4", 7),
    "gemm_nf4_lora_nested": ("nf4_gemm", "fp4_hip_gemm_lora_nested_nf4", 7),
    "lora_down": ("lora_down", "fp4_hip_lora_down", None), "lora_down_multi": ("lora_down", "fp4_hip_lora_down_multi", None),
}


@functools.lru_cache(maxsize=None)
def _recorded(which: str, entry: str, case: str) -> str:
    with open(os.path.join(_GOLDEN, f"{which}_entry_refusals.json")) as f:
        return json.load(f)[entry][case][1]


def _pow2_from_32(bs: int) -> bool:
    return bs >= 32 and bs & (bs - 1) == 0


def strict_refusal(op: str, args):
    """None where the C entry point behind ``op`` takes the call, else the message it sets."""
    rule = STRICT_RULES.get(op)
    if rule is None:
        return None
    kind, entry, bs_at = rule
    x = args[0]
    aligned, dt = x.data_ptr() % 16 == 0, _DT_CODE[x.dtype]
    if kind == "lora_down":
        R, K = args[1].shape[-2], args[1].shape[-1]
        if aligned:
            return None
        return f"{entry}: Bt={x.numel() // K} R={R} K={K} is not covered (1..64 rows, a rank that is a multiple of 8 in 8..256, 16-byte aligned x and A)"
    bs, (M, K) = int(args[bs_at]), args[bs_at + 1]
    rows = x.numel() // K
    shape_ok = K % 32 == 0 and _pow2_from_32(bs) and K % bs == 0
    numbers = f"M={M} K={K} blocksize={bs} dtype={dt}"
    if kind == "small_fp4":
        if x.dtype == torch.float32:  # one f32 GEMV per row, which takes any address and any even blocksize
            return None if rows <= 8 else "fp4_hip_gemm_small: f32 activations are covered up to 8 rows; use dequant + GEMM"
        if aligned and shape_ok and (rows <= 8 and K <= 4096 or bs == 64 and K % 64 == 0):
            return None
        text = _recorded("fp4", entry, "4 rows: misaligned x")
        return re.sub(r"B=\d+ M=\d+ K=\d+ blocksize=\d+ dtype=\d+", f"B={rows} {numbers}", text)
    if kind == "gemv_fp4_gated":
        if args[bs_at + 4] != 1 or (aligned and shape_ok and x.dtype != torch.float32):  # the plain epilogue: the generic kernel
            return None
        return re.sub(r"M=\d+ K=\d+ blocksize=\d+ dtype=\d+", numbers, _recorded("fp4", entry, "gate|up, misaligned x"))
    if kind == "nf4_gemv":
        if aligned and shape_ok:
            return None
        return re.sub(r"M=\d+ K=\d+ blocksize=\d+ dtype=\d+", numbers, _recorded("nf4", entry, "misaligned x"))
    assert kind == "nf4_gemm"
    if aligned and bs == 64 and K % 64 == 0 and x.dtype != torch.float32:
        return None
    text = _recorded("nf4", "fp4_hip_gemm_nested_nf4", "misaligned x").replace("fp4_hip_gemm_nested_nf4", entry)
    return re.sub(r"B=\d+ M=\d+ K=\d+ blocksize=\d+ dtype=\d+", f"B={rows} {numbers}", text)


class Strict:
    """``Strict(double)``: the double in strict mode (see above).  Everything else - ``calls``, ``refuse_*``, ``ScalarType`` - is the
    double's own."""

    def __init__(self, double):
        object.__setattr__(self, "_double", double)

    def __getattr__(self, name):
        attr = getattr(self._double, name)
        if name not in STRICT_RULES:
            return attr

        def op(*args, **kwargs):
            message = strict_refusal(name, args)
            if message is not None:
                calls = getattr(self._double, "calls", None)
                if isinstance(calls, list):
                    calls.append(name)  # the extension was called, and refused
                raise RuntimeError(message)
            return attr(*args, **kwargs)
        return op

    def __setattr__(self, name, value):
        setattr(self._double, name, value)


class FakeExt:
    def __init__(self, real_ext):
        self.ScalarType = real_ext.ScalarType
        self._dt = {real_ext.ScalarType.float16: torch.float16, real_ext.ScalarType.float32: torch.float32,
                    real_ext.ScalarType.bfloat16: torch.bfloat16}
        self.calls = []

    def _deq(self, A, absmax, M, N, blocksize, n, dtype, table):
        out = o.dequantize(A.numpy().reshape(-1), absmax.numpy(), blocksize, n, _NP[dtype], table)
        full = torch.zeros(M * N, dtype=dtype)
        full[:n] = _to_torch(out, dtype)
        return full.view(M, N)

    def dequantize_fp4(self, A, absmax, blocksize, M, N, o_type):
        self.calls.append("dequantize_fp4")
        return self._deq(A, absmax, M, N, blocksize, M * N, self._dt[o_type], "tree")

    def dequantize_fp4_codebook(self, A, absmax, codebook, M, N, blocksize, n, dtype):
        self.calls.append("dequantize_fp4_codebook")
        return self._deq(A, absmax, M, N, blocksize, n, self._dt[dtype], "codebook")

    def _gemv(self, A, B, absmax, blocksize, dtype, Bshape, bias):
        M, K = Bshape
        assert A.is_contiguous() and A.numel() == K and A.dtype == self._dt[dtype]
        y = o.gemv_exact(A.float().numpy().reshape(-1), B.numpy().reshape(-1), absmax.numpy(), M, K, blocksize)
        out = torch.from_numpy(y).to(A.dtype)
        if bias is not None:
            out = out + bias
        return out.view(*A.shape[:-1], M).clone()

    def gemv_fp4(self, A, B, absmax, datatype, blocksize, dtype, Bshape):
        self.calls.append("gemv_fp4")
        return self._gemv(A, B, absmax, blocksize, dtype, Bshape, None)

    def gemv_fp4_bias(self, A, B, absmax, datatype, blocksize, dtype, Bshape, bias):
        self.calls.append("gemv_fp4_bias")
        return self._gemv(A, B, absmax, blocksize, dtype, Bshape, bias)

    def gemv_fp4_fused(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue):
        self.calls.append("gemv_fp4_fused")
        M, K = Bshape
        if epilogue == 1 and (A.dtype == torch.float32 or K > 16384):
            raise RuntimeError("fp4_hip_gemv_fused: the gate|up epilogue is not available for this shape")
        assert A.is_contiguous() and A.numel() == K
        y = o.gemv_exact(A.float().numpy().reshape(-1), B.numpy().reshape(-1), absmax.numpy(), M, K, blocksize)
        nb = None if bias is None else bias.float().numpy()
        nr = None if residual is None else residual.float().numpy().reshape(-1)
        if A.dtype == torch.float32:
            t = y.astype(np.float32) + (0 if nb is None else nb) + (0 if nr is None else nr)
        elif epilogue == 1:
            t = o.linear_epilogue(y, _NP[A.dtype], nb)
            t = o.silu_mul_epilogue(t[0::2], t[1::2], _NP[A.dtype], nr)
        else:
            t = o.linear_epilogue(y, _NP[A.dtype], nb, nr)
        return torch.from_numpy(np.asarray(t, np.float32)).to(A.dtype).view(*A.shape[:-1], -1)

    def gemm_small_fp4_fused(self, A, B, absmax, blocksize, Bshape, bias, residual, epilogue):
        self.calls.append("gemm_small_fp4_fused")
        M, K = Bshape
        w = o.dequantize_f32(B.numpy().reshape(-1), absmax.numpy(), blocksize, M * K).reshape(M, K).astype(np.float64)
        y = A.float().numpy().reshape(-1, K).astype(np.float64) @ w.T
        if bias is not None:
            y = y + bias.float().numpy().astype(np.float64)
        nr = None if residual is None else residual.float().numpy().reshape(y.shape[0], -1)
        if epilogue == 1:
            t = o.silu_mul_epilogue(y[:, 0::2], y[:, 1::2], _NP[A.dtype], nr)
        else:
            t = o.linear_epilogue(y, _NP[A.dtype], None, nr)
        return torch.from_numpy(np.asarray(t, np.float32)).to(A.dtype).view(*A.shape[:-1], -1)

    def gemm_small_fp4(self, A, B, absmax, blocksize, Bshape, bias):
        self.calls.append("gemm_small_fp4")
        M, K = Bshape
        w = torch.from_numpy(o.dequantize_f32(B.numpy().reshape(-1), absmax.numpy(), blocksize, M * K)).view(M, K)
        y = torch.nn.functional.linear(A.float(), w, None if bias is None else bias.float())
        return y.to(A.dtype)

    def gemv_fp4_partial(self, A, B, absmax, blocksize, Bshape):
        self.calls.append("gemv_fp4_partial")
        M, K = Bshape
        assert A.is_contiguous() and A.numel() == K
        y = o.gemv_exact(A.float().numpy().reshape(-1), B.numpy().reshape(-1), absmax.numpy(), M, K, blocksize)
        return torch.from_numpy(y).float().view(1, M)

    def _qlinear(self, name, A_in, A, absmax, M, N, blocksize, table, bias=None):
        self.calls.append(name)
        w = self._deq(A, absmax, M, N, blocksize, M * N, A_in.dtype, table)
        return torch.nn.functional.linear(A_in, w, bias)

    def qlinear(self, A_in, A, absmax, M, N, blocksize):
        return self._qlinear("qlinear", A_in, A, absmax, M, N, blocksize, "tree")

    def qlinear_bias(self, A_in, A, absmax, M, N, blocksize, bias):
        return self._qlinear("qlinear_bias", A_in, A, absmax, M, N, blocksize, "tree", bias)

    def qlinear_codebook(self, A_in, A, absmax, codebook, M, N, blocksize):
        return self._qlinear("qlinear_codebook", A_in, A, absmax, M, N, blocksize, "codebook")

    def qlinear_codebook_bias(self, A_in, A, absmax, codebook, M, N, blocksize, bias):
        return self._qlinear("qlinear_codebook_bias", A_in, A, absmax, M, N, blocksize, "codebook", bias)

    def quantize_fp4(self, W, blocksize):
        self.calls.append("quantize_fp4")
        packed, am = o.quantize_fp4(W.float().numpy().reshape(-1), blocksize)
        return torch.from_numpy(packed).view(-1, 1), torch.from_numpy(am)

    def code_table(self, name):
        return torch.from_numpy(o.table(name).copy())
