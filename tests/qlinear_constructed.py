"""Constructed operands for the dequant + GEMM path (`qlinear*`: csrc/torch_ext.cpp, qlinear_impl) whose result is known bit for bit,
whatever the GEMM's blocking, split-K or summation order - proved on the CPU by tests/test_qlinear_constructed_host.py, run on the
GPU by tests/test_gpu_qlinear_exact.py.

Every expectation starts from the ORACLE's dequantised weight in the activation dtype T (``weight_T``: oracle.fp4_oracle.dequantize
for the tree and codebook tables, nf4_ref.dequantize_f32 rounded RNE to T for NF4), indexed by flat element, so blocks that straddle
rows ((300, 1000) with blocksize 64) need no special case.

* one-hot rows (``one_hot_expected``): activation row b is v at k_b and zero elsewhere; y[b][r] = T(fl32(W_T[r][k_b] * v)), every
  other term an exact zero.  Over ``byte_cycle_weight`` with ``flat_scales`` (tests/fp4_constructed.py).
* bias alone (``zero_code_weight``, ``full_precision_bias``): every weight code is the format's zero, so y[b][r] is bias[r], whose
  values need every significand bit of T, differ between all columns and are never zero.
* exact sums (``exact_sum_*``): 24 codes of +-1.0 per weight row under block scales in {1, 2, 4}, integer activations in -2..2 and
  an integer bias in -32..32: every product and every partial sum, in any order, is an integer of magnitude <= 224 < 256, exact in
  f32, fp16 and bf16, whether the bias joins before the rounding or after it.

One thing no construction fixes is the SIGN of an exact zero: a sum of terms that are all +-0 is +0 or -0 depending on what the
accumulator started from and which term came last.  ``bits`` therefore maps -0 to +0 (``canonical_zero``) before it compares; every
other value is compared by its bit pattern.

``routed`` asserts through the extension's route counters (``qlinear_gemm_stats``) which GEMM served the calls made inside it."""
from __future__ import annotations

import contextlib

import numpy as np

import nf4_ref as R
from fp4_constructed import ONE_HOT_VALUES, byte_cycle_weight, one_hot_batches, one_hot_positions, one_hot_rows, placement_scales  # noqa: F401
from nf4_constructed import tabled_statistics  # noqa: F401
from oracle import fp4_oracle as o

BS = 64
WEIGHT_SHAPES = [(320, 192), (300, 1000), (257, 4160)]  # every byte value at a fixed k; blocks straddle rows, odd sizes; > 1 pass over K
NESTED_SHAPES = [(320, 192), (257, 4160)]
DTYPES = ["float32", "float16", "bfloat16"]
FORMATS = ["tree", "codebook", "nf4"]
ZERO_CODE = {"tree": 0, "codebook": 0, "nf4": 7}
PLUS_ONE = {"tree": 3, "codebook": 3, "nf4": 15}
MINUS_ONE = {"tree": 11, "codebook": 11, "nf4": 0}
TERMS = 24  # non-zero codes per weight row of the exact sums
SIGNIFICAND_BITS = {"float32": 24, "float16": 11, "bfloat16": 8}


def row_shapes(K: int) -> list:
    """The activation shapes of the GPU tests: 2-D, 3-D, across the 64- and 128-row thresholds of the fused kernels, and 1-D."""
    return [(2, K), (1, 5, K), (65, K), (129, K), (3, 100, K), (K,)]


def n_blocks(M: int, K: int, bs: int = BS) -> int:
    return -(-M * K // bs)


def _check(M: int, K: int, bs: int):
    if M < 1 or K < 2 or bs < 2 or bs % 2 or (M * K) % 2:
        raise ValueError(f"M={M} K={K} bs={bs}: need M >= 1, K >= 2, an even blocksize and an even number of weights")


# ---- values of T ------------------------------------------------------------------------------------------------------------------
def round_T(f32: np.ndarray, dtype: str) -> np.ndarray:
    """float32 values -> float64 values of their RNE rounding to ``dtype`` (one rounding, by bit arithmetic for bf16)."""
    f = np.ascontiguousarray(f32, np.float32)
    if dtype == "float32":
        return f.astype(np.float64)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return f.astype(np.float16).astype(np.float64)
    if dtype == "bfloat16":
        return o.bf16_bits_to_f32(o.f32_to_bf16_bits(f)).astype(np.float64).reshape(f.shape)
    raise ValueError(dtype)


def canonical_zero(a: np.ndarray) -> np.ndarray:
    return np.where(a == 0, np.zeros_like(a), a)


def bits(values: np.ndarray, dtype: str) -> np.ndarray:
    """Bit patterns in ``dtype`` of float values that are REPRESENTABLE in it (raises otherwise), -0 mapped to +0."""
    v = np.asarray(values, np.float64)
    back = round_T(v.astype(np.float32), dtype)
    if not np.array_equal(back, v):
        raise ValueError(f"values are not representable in {dtype}")
    f = canonical_zero(v).astype(np.float32)
    if dtype == "float32":
        return f.view(np.uint32)
    if dtype == "float16":
        return f.astype(np.float16).view(np.uint16)
    return o.f32_to_bf16_bits(f).reshape(f.shape)


def weight_T(packed: np.ndarray, absmax: np.ndarray, M: int, K: int, fmt: str, dtype: str, bs: int = BS) -> np.ndarray:
    """float64[M, K]: the values of the oracle's dequantised weight in ``dtype`` - what both GEMM routes multiply."""
    n = M * K
    if fmt == "nf4":
        return round_T(R.dequantize_f32(packed, absmax, bs, n), dtype).reshape(M, K)
    if fmt not in ("tree", "codebook"):
        raise ValueError(f"unknown format {fmt!r}")
    w = o.dequantize(packed, absmax, bs, n, dtype, fmt)
    if dtype == "bfloat16":
        w = o.bf16_bits_to_f32(w)
    return w.astype(np.float64).reshape(M, K)


# ---- one-hot rows -------------------------------------------------------------------------------------------------------------------
def flat_scales(M: int, K: int, bs: int = BS) -> np.ndarray:
    """float32[ceil(M K / bs)]: placement_scales(M, K) where blocks stay inside rows; where they straddle rows, the same 13 powers of
    two by FLAT block index f, 2^((3 f) % 13 - 3): blocks f and f + 1 differ, and so do the blocks a column meets in neighbouring
    rows, which lie K // bs or K // bs + 1 apart (tests/test_qlinear_constructed_host.py asserts both for the shapes used)."""
    _check(M, K, bs)
    if K % bs == 0:
        return placement_scales(M, K, bs)
    return placement_scales(n_blocks(M, K, bs), bs, bs)


def one_hot_expected(w_T: np.ndarray, pos: np.ndarray, val: np.ndarray, dtype: str) -> np.ndarray:
    """float64[B, M]: T(fl32(W_T[r][k_b] * v_b)) for the one-hot rows (pos[b], val[b]); both factors are f32 values, the product is
    rounded once to f32 and once to T."""
    pos, val = np.asarray(pos, np.int64).reshape(-1), np.asarray(val, np.float64).reshape(-1)
    if pos.shape != val.shape or pos.size == 0 or pos.min() < 0 or pos.max() >= w_T.shape[1]:
        raise ValueError("one-hot rows: positions and values must match and lie inside the row")
    w32, v32 = w_T[:, pos].T.astype(np.float32), val.astype(np.float32)
    if not (np.array_equal(w32.astype(np.float64), w_T[:, pos].T) and np.array_equal(v32.astype(np.float64), val)):
        raise ValueError("one-hot rows: the weight and the values must be f32 numbers")
    return round_T(w32 * v32[:, None], dtype)


# ---- bias alone -----------------------------------------------------------------------------------------------------------------------
def zero_code_weight(M: int, K: int, fmt: str, bs: int = BS):
    """(packed, absmax): every nibble the format's zero code (FP4 0, NF4 7) under flat_scales."""
    _check(M, K, bs)
    z = ZERO_CODE[fmt]
    return np.full(M * K // 2, (z << 4) | z, np.uint8), flat_scales(M, K, bs)


def full_precision_bias(M: int, dtype: str) -> np.ndarray:
    """float64[M] of T values: (-1)^r * (1 + m_r / 2^(p-1)) * 2^(r % 7 - 3) with an ODD m_r = 2 ((37 r + 11) % 2^(p-2)) + 1, p the
    significand width of T (24 / 11 / 8).  The last significand bit is set, so no narrower format holds the value; m_r runs over
    2^(p-2) >= 64 values and the exponent over 7, so the first 448 columns all differ; both signs occur and no value is zero."""
    if M < 1 or M > 448:
        raise ValueError(f"M={M}: the bias values are shown to be distinct for 1..448 columns")
    p = SIGNIFICAND_BITS[dtype]
    r = np.arange(M, dtype=np.int64)
    m = 2 * ((37 * r + 11) % (1 << (p - 2))) + 1
    return np.where(r % 2 == 0, 1.0, -1.0) * np.ldexp(1.0 + m / float(1 << (p - 1)), (r % 7 - 3).astype(np.int32))


def arbitrary_rows(shape, dtype: str, seed: int = 0) -> np.ndarray:
    """float64[shape] of finite T values of mixed sign and magnitude (N(0, 1) * 2^(-4..4), rounded to T)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * np.ldexp(1.0, rng.integers(-4, 5, size=shape))
    return round_T(x.astype(np.float32), dtype)


# ---- exact sums ----------------------------------------------------------------------------------------------------------------------
def exact_sum_positions(M: int, K: int) -> np.ndarray:
    """int64[M, 24]: the k of the non-zero codes of row r, (7 r + 173 i) % K: distinct within a row where gcd(173, K) = 1 or
    K / gcd >= 24 (checked), spread over the whole row."""
    r, i = np.arange(M, dtype=np.int64)[:, None], np.arange(TERMS, dtype=np.int64)[None, :]
    pos = (7 * r + 173 * i) % K
    if K < TERMS or any(len(set(row.tolist())) != TERMS for row in pos[:min(M, 8)]):
        raise ValueError(f"K={K}: the {TERMS} positions of a row collide")
    return pos


def exact_sum_scales(M: int, K: int, bs: int = BS) -> np.ndarray:
    """float32[ceil(M K / bs)] in {1, 2, 4}.  Blocks inside rows: 2^((r + a j) % 3), a = 1 or 2, which differs between neighbouring blocks AND
    neighbouring rows.  Blocks that straddle rows: 2^(f % 3) by flat block index - neighbouring blocks differ; a column's blocks in
    neighbouring rows lie d = K // bs or d + 1 apart, BOTH for every block, and three values cannot differ at distances 1, d and
    d + 1 at once (c(f + 1), c(f + d + 1) and c(f) are pairwise neighbours, so are c(f + d), c(f + d + 1) and c(f): hence
    c(f + d) = c(f + 1), period d - 1, and with c(f), c(f + 1), c(f + 2) all different also period 3 - a constant unless 3 divides
    d - 1).  There the scales differ between rows at the distance that is no multiple of 3."""
    _check(M, K, bs)
    if K % bs == 0:
        r, j = np.arange(M, dtype=np.int64)[:, None], np.arange(K // bs, dtype=np.int64)[None, :]
        a = 2 if (K // bs) % 3 == 2 else 1  # so that the last block of a row and the first of the next differ too
        e = (r + a * j) % 3
    else:
        e = np.arange(n_blocks(M, K, bs), dtype=np.int64) % 3
    return np.ldexp(np.float32(1.0), e.astype(np.int32).reshape(-1)).astype(np.float32)


def exact_sum_weight(M: int, K: int, fmt: str, bs: int = BS):
    """(packed, absmax): 24 codes of +-1.0 per row at exact_sum_positions, the sign (-1)^(r + i) (neighbours in i and in r differ),
    every other code the zero code; exact_sum_scales."""
    _check(M, K, bs)
    pos = exact_sum_positions(M, K)
    nib = np.full((M, K), ZERO_CODE[fmt], np.uint8)
    r, i = np.arange(M)[:, None], np.arange(TERMS)[None, :]
    nib[r, pos] = np.where((r + i) % 2 == 0, PLUS_ONE[fmt], MINUS_ONE[fmt]).astype(np.uint8)
    nib = nib.reshape(-1)
    return ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8), exact_sum_scales(M, K, bs)


def exact_sum_rows(shape) -> np.ndarray:
    """float64[shape]: integers in -2..2, ((3 b + 7 k + b k) % 5) - 2 over the flattened rows b."""
    K = shape[-1]
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    b, k = np.arange(rows, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    return (((3 * b + 7 * k + b * k) % 5) - 2).astype(np.float64).reshape(shape)


def exact_sum_bias(M: int) -> np.ndarray:
    """float64[M]: integers in -32..32, ((7 r + 3) % 65) - 32."""
    return (((7 * np.arange(M, dtype=np.int64) + 3) % 65) - 32).astype(np.float64)


def exact_sum_bound(w_T: np.ndarray, x: np.ndarray, bias) -> float:
    """The largest magnitude any partial sum can reach: non-zeros per row x max |w| x max |x| + max |bias|."""
    nz = int((w_T != 0).sum(axis=1).max())
    return nz * float(np.abs(w_T).max()) * float(np.abs(x).max()) + (0.0 if bias is None else float(np.abs(bias).max()))


def product(w_T: np.ndarray, x: np.ndarray, bias=None) -> np.ndarray:
    """float64 x @ W_T^T (+ bias) over the flattened rows: [rows, M]."""
    y = np.asarray(x, np.float64).reshape(-1, w_T.shape[1]) @ w_T.T
    return y if bias is None else y + np.asarray(bias, np.float64)


# ---- the route counters -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def routed(ext, route: str, calls=None):
    """Asserts on exit that every qlinear* call made inside went through ``route`` ('direct' = hipBLASLt through the cached plan,
    'aten' = at::linear): that counter advanced (by ``calls`` where given) and the other one stood still."""
    if route not in ("direct", "aten"):
        raise ValueError(route)
    other = "aten" if route == "direct" else "direct"
    before = dict(ext.qlinear_gemm_stats())
    yield
    after = dict(ext.qlinear_gemm_stats())
    took, strayed = after[route] - before[route], after[other] - before[other]
    assert strayed == 0, f"{strayed} call(s) took the {other} route where {route} was expected"
    assert took > 0 if calls is None else took == calls, f"{took} call(s) on the {route} route, expected {'some' if calls is None else calls}"
