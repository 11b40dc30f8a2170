"""Test-side restatement of bitsandbytes' double-quantised (nested) absmax, independent of the code under test.

bitsandbytes is not installed where these tests run, so the rules are restated from ``QuantState.as_dict`` /
``dequantize_4bit`` / ``quantize_blockwise``:

    decode:  absmax[i] = fl32( fl32( code256[q[i]] * nested_absmax[i // g] ) + offset )         a multiply, then an add
    encode:  per group of g values  v = fl32(a - offset), m = max|v|, n = fl32(v * fl32(1 / m)),
             q = index of the entry of code256 nearest to n (exact tie: the lower index), nested_absmax = m;
             m == 0: every q is the index of the table's 0.0.

``dynamic_map`` is ``create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8)``: for i in 0..6, 2^i + 1
``torch.linspace(0.1, 1, .)`` f32 boundaries, whose pairwise means times 10^(i - 6) enter with both signs; plus 0 and 1; sorted.
"""
from __future__ import annotations

import ctypes

import numpy as np

DYNAMIC_MAP_SHA256 = "e732639a65f497b4ad684bb166a4467708255edd5207757de8b8f0c7e1fda89c"
F32 = np.float32


def dynamic_map() -> np.ndarray:
    import torch

    data = []
    for i in range(7):
        b = torch.linspace(0.1, 1, 2**i + 1)
        means = (b[:-1] + b[1:]) / 2.0
        scaled = (10 ** (i - 6)) * means
        data += scaled.tolist() + (-scaled).tolist()
    data += [0.0, 1.0]
    return np.array(sorted(data), F32)


def unnest(q, nested_absmax, code256, offset, g: int) -> np.ndarray:
    """Two f32 roundings: numpy rounds each f32 operation on its own."""
    q = np.asarray(q, np.uint8).ravel()
    code256, nested_absmax = np.asarray(code256, F32), np.asarray(nested_absmax, F32)
    t = (code256[q] * nested_absmax[np.arange(q.size) // g]).astype(F32)
    return (t + F32(offset)).astype(F32)


def unnest_fma(q, nested_absmax, code256, offset, g: int) -> np.ndarray:
    """What a fused multiply-add would give: ONE rounding of the exact code * scale + offset (exact in float64: 24 + 24 bits of
    product, and the sum of a 48-bit and a 24-bit number whose exponents are close enough for every fixture here)."""
    q = np.asarray(q, np.uint8).ravel()
    c = np.asarray(code256, F32).astype(np.float64)[q]
    m = np.asarray(nested_absmax, F32).astype(np.float64)[np.arange(q.size) // g]
    return (c * m + np.float64(F32(offset))).astype(F32)


def nest(absmax, offset, code256, g: int):
    """-> (q uint8 [nb], nested_absmax f32 [ceil(nb / g)], ties bool [nb]: the two nearest entries are equidistant)."""
    a = np.asarray(absmax, F32).ravel()
    code = np.asarray(code256, F32).astype(np.float64)
    nb = a.size
    ng = -(-nb // g)
    q = np.empty(nb, np.uint8)
    ties = np.zeros(nb, bool)
    nested = np.empty(ng, F32)
    zero_index = int(np.argmin(np.abs(code)))
    for j in range(ng):
        v = (a[j * g:(j + 1) * g] - F32(offset)).astype(F32)
        m = F32(np.max(np.abs(v)))
        nested[j] = m
        if m == 0:
            q[j * g:(j + 1) * g] = zero_index
            continue
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            inv = F32(F32(1.0) / m)
            n = (v * inv).astype(F32).astype(np.float64)
        d = np.abs(code[None, :] - n[:, None])  # exact in float64 for the entries that can be nearest
        best = np.argmin(d, axis=1)  # the first minimum: the lower index on a tie
        q[j * g:(j + 1) * g] = best
        two = np.partition(d, 1, axis=1)[:, :2]
        ties[j * g:(j + 1) * g] = two[:, 0] == two[:, 1]
    return q, nested, ties


def recipe_absmax(blocks: int = 1000, seed: int = 0) -> np.ndarray:
    """The fixture of the unnest / nest tests: the absmax of `blocks` blocks of 64 draws of 0.05 * N(0, 1)."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((blocks, 64)) * 0.05).astype(F32)
    return np.max(np.abs(w), axis=1).astype(F32)


# ---- ctypes bindings of the three entry points ---------------------------------------------------------------------------------
def lib():
    import hipabi

    l = hipabi.lib()
    if not getattr(l, "_nested_bound", False):
        vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
        l.fp4_hip_absmax_unnest.argtypes = [vp, vp, vp, f32, i32, i64, vp, vp]
        l.fp4_hip_absmax_unnest.restype = i32
        l.fp4_hip_absmax_nest.argtypes = [vp, i64, f32, vp, i32, vp, vp, vp]
        l.fp4_hip_absmax_nest.restype = i32
        l.fp4_hip_gemv_nested_nf4.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, i64, i64, i32, i32, i32, vp]
        l.fp4_hip_gemv_nested_nf4.restype = i32
        l._nested_bound = True
    return l
