"""A CPU restatement of the fused kernels' epilogue chains at EVERY value, and the pattern sets that drive them.

The kernels apply a short elementwise chain to a finished f32 row sum (csrc/gemv_common.h: store_row, store_silu_mul, store_small,
store_small_silu_mul).  The four chains, T = bf16 / fp16 (the plain ones also f32, where every rounding is the identity):

* batch-1 plain   T(T(T(sum) + bias) + res)
* batch plain     T(T(sum + bias) + res)                 (a LoRA delta has joined `sum` before)
* batch-1 gated   g = T(sum_g), g = T(g + bias[2i]) if a bias is given, the same for u; s = T(q(g)); t = T(s u); t = T(t + res[i])
* batch gated     g = T(sum_g + bias[2i]), u = T(sum_u + bias[2i + 1]); then as batch-1 gated

q is the f32 FORMULA g / (1 + exp(-g)), not true silu: e = f32(exp(-g)) (overflow gives inf), d = f32(1 + e), q = f32(g / d).  So
q(-inf) is NaN, q(g) is -0 for g < -88.72 (e overflows), q(g) = g from g = 16.64 on (e <= 2^-24: d = 1).  The device's expf is documented to 1 ulp,
so the gated chains return a SET: the chain run with e, nextafter(e, -inf) and nextafter(e, +inf) when e is finite, with e alone
otherwise (the three members are then equal).  A result agrees when it equals a member: same bits for finite values and zeros (the
sign of zero counts), same sign for infinities, NaN matches NaN (neither payload nor sign).  There is no ulp tolerance anywhere; the
host test caps the number of gate patterns whose set has more than one member, so the set cannot grow into one.

Everything is numpy on f32 arrays that hold T values; `values` / `to_bits` go between those and 16-bit patterns."""
from __future__ import annotations

import numpy as np

from oracle import fp4_oracle as o

BF16, F16, F32 = "bfloat16", "float16", "float32"
F32_ONE = np.float32(1.0)


# ---- T values <-> bit patterns, rounding ---------------------------------------------------------------------------------------------
def values(bits, dtype: str) -> np.ndarray:
    """uint16 patterns of T -> their f32 values (exact)."""
    b = np.ascontiguousarray(bits, np.uint16)
    return o.bf16_bits_to_f32(b) if dtype == BF16 else b.view(np.float16).astype(np.float32)


def to_bits(v, dtype: str) -> np.ndarray:
    """T-valued f32 -> uint16 patterns of T."""
    v = np.ascontiguousarray(v, np.float32)
    return (v.view(np.uint32) >> 16).astype(np.uint16) if dtype == BF16 else v.astype(np.float16).view(np.uint16)


def rt(v, dtype: str) -> np.ndarray:
    """f32 -> the nearest T value (RNE; overflow gives inf, NaN stays NaN), as f32.  The oracle's roundings, on f32 input."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if dtype == BF16:
            return o.bf16_bits_to_f32(o.f32_to_bf16_bits(v)).reshape(v.shape)
        return o.round_to(dtype)(v)


def _add(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float32) + np.asarray(b, np.float32)


# ---- equality --------------------------------------------------------------------------------------------------------------------------
def same(a, b) -> np.ndarray:
    """Elementwise: same f32 bits, or both NaN."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32))
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def agrees(got, want_set) -> np.ndarray:
    """got [...] against a reference set [n, ...]: equal to some member."""
    return np.any(same(np.asarray(got, np.float32)[None], want_set), axis=0)


def multi_member(want_set) -> np.ndarray:
    """Where the members of a reference set [n, ...] are not all equal."""
    return ~np.all(same(want_set[:1], want_set), axis=0)


# ---- the chains ------------------------------------------------------------------------------------------------------------------------
def exp_neg(g) -> np.ndarray:
    """f32(exp(-g)) with exp taken in float64; overflow gives inf."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.exp(-np.asarray(g, np.float64)).astype(np.float32)


def exp_set(g) -> np.ndarray:
    """[3, ...]: e, nextafter(e, -inf), nextafter(e, +inf) where e is finite; e three times where it is inf or NaN."""
    e = exp_neg(g)
    fin = np.isfinite(e)
    with np.errstate(over="ignore", invalid="ignore"):
        lo = np.where(fin, np.nextafter(e, np.float32(-np.inf)), e)
        hi = np.where(fin, np.nextafter(e, np.float32(np.inf)), e)
    return np.stack([e, lo, hi]).astype(np.float32)


def formula(g, e) -> np.ndarray:
    """q = f32(g / f32(1 + e))."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        d = (F32_ONE + np.asarray(e, np.float32)).astype(np.float32)
        return (np.asarray(g, np.float32) / d).astype(np.float32)


def silu_set(g, dtype: str) -> np.ndarray:
    """[3, ...]: s = T(q(g)) under the three exps.  g holds T values."""
    g = np.asarray(g, np.float32)
    return np.stack([rt(formula(g, e), dtype) for e in exp_set(g)])


def gated(g, u, dtype: str, residual=None) -> np.ndarray:
    """[3, ...]: T(T(s u) + res) for T-valued gate and up rows (what the plain entry point returns for them)."""
    g, u = np.asarray(g, np.float32), np.asarray(u, np.float32)
    out = []
    for s in silu_set(g, dtype):
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            t = rt(s * u, dtype)
        if residual is not None:
            t = rt(_add(t, residual), dtype)
        out.append(t)
    return np.stack(out)


def operand_batch1(total, bias, dtype: str) -> np.ndarray:
    """A gate or up row of the batch-1 kernels: T(T(sum) + bias)."""
    t = rt(total, dtype)
    return t if bias is None else rt(_add(t, bias), dtype)


def operand_batch(total, bias, dtype: str) -> np.ndarray:
    """A gate or up row of the 2..64-row kernels: T(sum + bias), the bias joining the f32 sum."""
    return rt(total if bias is None else _add(total, bias), dtype)


def gated_batch1(sum_g, sum_u, dtype: str, bias_g=None, bias_u=None, residual=None) -> np.ndarray:
    return gated(operand_batch1(sum_g, bias_g, dtype), operand_batch1(sum_u, bias_u, dtype), dtype, residual)


def gated_batch(sum_g, sum_u, dtype: str, bias_g=None, bias_u=None, residual=None) -> np.ndarray:
    return gated(operand_batch(sum_g, bias_g, dtype), operand_batch(sum_u, bias_u, dtype), dtype, residual)


def plain_batch1(total, dtype: str, bias=None, residual=None) -> np.ndarray:
    """T(T(T(sum) + bias) + res); with f32, plain f32 adds in that order."""
    t = operand_batch1(total, bias, dtype)
    return t if residual is None else rt(_add(t, residual), dtype)


def plain_batch(total, dtype: str, bias=None, residual=None) -> np.ndarray:
    """T(T(sum + bias) + res)."""
    t = operand_batch(total, bias, dtype)
    return t if residual is None else rt(_add(t, residual), dtype)


# ---- pattern sets ----------------------------------------------------------------------------------------------------------------------
FORMAT = {BF16: dict(exp_bits=8, man_bits=7), F16: dict(exp_bits=5, man_bits=10)}
E_OVERFLOW = 88.72283905206835  # ln(f32 max): exp(-g) overflows below -this
# 1 + e rounds to 1 for every e <= 2^-24 (the tie goes to even), i.e. from g = 24 ln 2 = 16.64 on; 25 ln 2 = 17.33 lies a binade of e
# further in, where a 1-ulp error of exp cannot reach the tie any more.  The T neighbours of both are in E_T.
D_IS_ONE = (24 * np.log(2.0), 25 * np.log(2.0))


def inf_bits(dtype: str) -> int:
    return 0x7F80 if dtype == BF16 else 0x7C00


def max_bits(dtype: str) -> int:
    return inf_bits(dtype) - 1


def ulp_of_one(dtype: str) -> float:
    return 2.0 ** -FORMAT[dtype]["man_bits"]


def neighbours(x: float, dtype: str):
    """The two T patterns around x: the largest value <= x and the smallest >= x."""
    allb = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    with np.errstate(invalid="ignore"):
        v = values(allb, dtype).astype(np.float64)
    fin = np.isfinite(v)
    below = allb[fin & (v <= x)]
    above = allb[fin & (v >= x)]
    return int(below[np.argmax(v[fin & (v <= x)])]), int(above[np.argmin(v[fin & (v >= x)])])


def edge_patterns(dtype: str) -> np.ndarray:
    """E_T: every exponent x mantissa {0, 1, half, all ones} x both signs (zeros, the subnormal edges, max, +-inf and two NaNs per
    sign among them), the T neighbours of -88.72 and of both ends of the `1 + e == 1` edge, of 0 and of max."""
    m = FORMAT[dtype]["man_bits"]
    pats = set()
    for ex in range(1 << FORMAT[dtype]["exp_bits"]):
        for man in (0, 1, 1 << (m - 1), (1 << m) - 1):
            for sign in (0, 0x8000):
                pats.add(sign | (ex << m) | man)
    for x in (-E_OVERFLOW, E_OVERFLOW) + D_IS_ONE + tuple(-d for d in D_IS_ONE):
        pats.update(neighbours(x, dtype))
    for b in (1, 2, max_bits(dtype), max_bits(dtype) - 1):
        pats.update((b, b | 0x8000))
    return np.array(sorted(pats), np.uint16)


def finite(bits, dtype: str) -> np.ndarray:
    bits = np.asarray(bits, np.uint16)
    return bits[(bits & 0x7FFF) < inf_bits(dtype)]


def up_patterns(dtype: str) -> np.ndarray:
    """U: +-0, +-1, the smallest normal, a negative subnormal, +-max, +-inf, NaN, 1/3, -2.5."""
    m, mx, inf = FORMAT[dtype]["man_bits"], max_bits(dtype), inf_bits(dtype)
    one, third, m25 = (int(to_bits(rt(np.float32([x]), dtype), dtype)[0]) for x in (1.0, 1.0 / 3.0, -2.5))
    return np.array([0, 0x8000, one, one | 0x8000, 1 << m, 0x8003, mx, mx | 0x8000, inf, inf | 0x8000, inf | (1 << (m - 1)), third, m25], np.uint16)


def residual_patterns(dtype: str) -> np.ndarray:
    """R without `none`: +-0, max, +inf."""
    return np.array([0, 0x8000, max_bits(dtype), inf_bits(dtype)], np.uint16)


def residual_prime_patterns(dtype: str) -> np.ndarray:
    """R' = U and +-max (which U holds already): the residuals of the plain chain."""
    return up_patterns(dtype)


def bias_subset(dtype: str) -> np.ndarray:
    """16 patterns of E_T for the sum-driven gated runs: zeros, units, a tie-maker, subnormals, max, inf and NaN."""
    m, mx, inf = FORMAT[dtype]["man_bits"], max_bits(dtype), inf_bits(dtype)
    one = int(to_bits(np.float32([1.0]), dtype)[0])
    return np.array([0, 0x8000, one, one | 0x8000, one | 1, 1, 0x8001, 1 << m, (1 << m) | 0x8000, mx, mx | 0x8000, inf, inf | 0x8000,
                     inf | (1 << (m - 1)), neighbours(-E_OVERFLOW, dtype)[0], neighbours(D_IS_ONE[0], dtype)[1]], np.uint16)


# ---- sum-driven operands ---------------------------------------------------------------------------------------------------------------
def sum_row_scales(dtype: str) -> np.ndarray:
    """f32 block scales that are NOT T values, one sum class each (under a unit activation and a +-1 code): two ties of opposite
    parity around 1, a value that rounds down to max and one that overflows T, and magnitudes whose negative rounds to -0."""
    u = ulp_of_one(dtype)
    mx = float(values([max_bits(dtype)], dtype)[0])
    tiny = 2.0**-140 if dtype == BF16 else 2.0**-26
    return np.array([1 + u / 2, 1 + 3 * u / 2, mx * (1 + u / 8), mx * (1 + u / 2) if dtype == BF16 else 1.0e5, tiny], np.float32)


def activation_scales(dtype: str) -> np.ndarray:
    """T values a batch row's one-hot entry takes; each turns the rows' sums into another class: unchanged, +0, the tie-makers
    1 + ulp and 1 - ulp/2 (an odd mantissa times a scale with mantissa bits of its own), down towards the subnormals, up past max."""
    u = ulp_of_one(dtype)
    return np.array([1.0, 0.0, 1 + u, 1 - u / 2, -1.0, 2.0**-7, 1.5 * 2.0**7], np.float32)
