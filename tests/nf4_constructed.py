"""Constructed NF4 operands whose GEMV / GEMM / adapter result has a closed form (the NF4 side of tests/fp4_constructed.py, whose
generic pieces - the byte-cycle weight, the placement scales, the one-hot positions, the bar and the guard helpers - are used as they
are: nothing in them depends on the code table).

* ``closed_form_nf4``: one-hot activations over the byte-cycle weight give ONE product  CODE[nibble(r, k)] * absmax[r][k // bs] * x
  per output, with nf4_ref.CODE; the nibble is the plain table index (NF4 has no sign bit).  The smallest non-zero |output| is
  0.0796 * 2^-3 * 0.75, a normal fp16 number; the largest 1.0 * 2^9 * 3.
* ``gemv_f32_restatement``: what the batch-1 f32 kernel leaves of a one-hot row: fl32(fl32(code * x) * absmax).  Every other term of
  the row is an exact zero and the scale is a power of two, so fl32(code * x) is the row's only rounding.
* ``nested_statistics``: double-quantised statistics (uint8 code per block, f32 scale per 256 blocks, a CUSTOM 256-entry table, an
  offset) whose expansion fl32(fl32(code256 * nested) + offset) is exact and differs between neighbouring blocks and groups.
* ``lora_b`` / ``lora_a``: adapter matrices of small dyadic entries, exact in bf16 and fp16, that differ between neighbouring rows
  and columns; with a one-hot t (or x) the adapter term (the down projection) is one exact product.

Every builder raises ValueError on a shape it was not made for; none quietly returns something else."""
from __future__ import annotations

import numpy as np

import nf4_ref as R
from fp4_constructed import (F16_MIN_NORMAL, ONE_HOT_VALUES, bar, byte_cycle_weight, guard_elems, guarded, guards_intact,  # noqa: F401
                             nibble, one_hot_batches, one_hot_positions, one_hot_rows, one_hot_value, placement_scales, refill, untouched)

# One (M, K) per dispatch cell (ks, G, iters) of the batch-1 kernel: the row-tail entry of nf4_ref.GEMV_CELL_CASES, or the cell's other
# entry where that is smaller and also leaves a partial last pass ((512, 8224) for (1023, 32768)).  tests/test_nf4_constructed_host.py
# shows that the twelve reach the twelve cells and that each has a partial last pass.
GEMV_PLACEMENT_CASES = [(1023, 992), (4097, 800), (8193, 736), (2047, 1056), (2049, 1600), (4097, 1088), (1023, 2080), (1025, 3104),
                        (2049, 4064), (512, 8224), (1025, 8224), (4097, 4128)]

NESTED_GROUP = 256  # blocks per nested scale: what fp4_hip_gemv_nested_nf4 covers
NESTED_OFFSETS = (0.0, 0.25)


def _check_shape(M: int, K: int, bs: int):
    if M < 1 or K < 2 or K % 2 or bs < 2 or K % bs:
        raise ValueError(f"M={M} K={K} bs={bs}: need M >= 1, an even K >= 2 and a blocksize that divides K (blocks must not straddle rows)")


def _check_one_hot(K: int, pos, val):
    pos, val = np.asarray(pos), np.asarray(val)
    if pos.shape != val.shape or pos.size == 0 or pos.min() < 0 or pos.max() >= K:
        raise ValueError(f"one-hot rows: positions {pos.shape} / values {val.shape} must match and lie in [0, {K})")


def closed_form_nf4(M: int, K: int, pos, val, bs: int = 64, absmax=None) -> np.ndarray:
    """float64[..., M]: CODE[nibble(r, k)] * absmax[r][k // bs] * x for the one-hot rows (pos, val) over byte_cycle_weight(M, K).
    ``absmax`` (float32[M * K / bs]) defaults to placement_scales(M, K, bs)."""
    _check_shape(M, K, bs)
    _check_one_hot(K, pos, val)
    am = placement_scales(M, K, bs) if absmax is None else np.asarray(absmax)
    if am.size != M * K // bs:
        raise ValueError(f"absmax has {am.size} entries, the weight {M * K // bs} blocks")
    r = np.arange(M, dtype=np.int64)
    k = np.asarray(pos, np.int64)[..., None]
    code = R.CODE.astype(np.float64)[nibble(r, k)]
    return code * am.reshape(M, K // bs).astype(np.float64)[r, k // bs] * np.asarray(val, np.float64)[..., None]


def gemv_f32_restatement(M: int, K: int, pos, val, bs: int = 64, absmax=None) -> np.ndarray:
    """float32[..., M]: fl32(fl32(code * x) * absmax), the f32 steps of the batch-1 kernel on a one-hot row."""
    _check_shape(M, K, bs)
    _check_one_hot(K, pos, val)
    am = (placement_scales(M, K, bs) if absmax is None else np.asarray(absmax, np.float32)).reshape(M, K // bs)
    r = np.arange(M, dtype=np.int64)
    k = np.asarray(pos, np.int64)[..., None]
    t = (R.CODE[nibble(r, k)] * np.asarray(val, np.float32)[..., None]).astype(np.float32)
    return (t * am[r, k // bs]).astype(np.float32)


# ---- nested (double-quantised) placement statistics ---------------------------------------------------------------------------------
def nested_code256() -> np.ndarray:
    """float32[256]: code256[q] = (16 + (q >> 4)) / 16 * 2^((q & 15) - 8): 256 distinct values, each exact in 5 bits."""
    q = np.arange(256)
    return np.ldexp((16 + (q >> 4)) / 16.0, (q & 15) - 8).astype(np.float32)


def nested_statistics(nb: int, offset: float):
    """(absmax_u8 uint8[nb], nested_absmax float32[ceil(nb / 256)], code256 float32[256], offset) with absmax_u8[i] = (7 i + 3) % 256
    and nested_absmax[g] = 2^(g % 5).  7 is a unit mod 256 and the table has no repeated value, so neighbouring blocks differ; the
    scales of neighbouring groups differ by a factor of 2 (16 at the wrap), which no table ratio inside a group undoes by accident
    for blocks i and i + 256 (their codes differ by 7 * 256 % 256 = 0: the same code under a different scale)."""
    if nb < 1:
        raise ValueError(f"nb={nb}: need at least one block")
    if offset not in NESTED_OFFSETS:
        raise ValueError(f"offset={offset}: the expansion is shown to be exact for {NESTED_OFFSETS} only")
    q = ((7 * np.arange(nb, dtype=np.int64) + 3) % 256).astype(np.uint8)
    nested = np.ldexp(np.float32(1.0), (np.arange(-(-nb // NESTED_GROUP)) % 5).astype(np.int32)).astype(np.float32)
    return q, nested, nested_code256(), float(offset)


def nested_expanded(nb: int, offset: float) -> np.ndarray:
    """float64[nb]: code256[q[i]] * nested[i // 256] + offset in float64 - what the f32 expansion must equal, exactly."""
    q, nested, code, offset = nested_statistics(nb, offset)
    return code.astype(np.float64)[q] * nested.astype(np.float64)[np.arange(nb) // NESTED_GROUP] + offset


def tabled_statistics(absmax: np.ndarray):
    """Any absmax of at most 256 distinct values as nested statistics that expand to it bit for bit: the distinct values are the
    table (so a 0 or an Inf scale is a table entry that is 0 or Inf), every group scale is 1 and the offset 0."""
    a = np.asarray(absmax, np.float32).ravel()
    values, q = np.unique(a, return_inverse=True)
    if values.size > 256 or np.isnan(values).any():
        raise ValueError(f"{values.size} distinct scales (or a NaN): a 256-entry table cannot hold them")
    code = np.ones(256, np.float32)
    code[:values.size] = values
    return q.astype(np.uint8), np.ones(-(-a.size // NESTED_GROUP), np.float32), code, 0.0


# ---- LoRA placement ---------------------------------------------------------------------------------------------------------------------
def _check_rank(Rr: int):
    if Rr < 8 or Rr > 256 or Rr % 8:
        raise ValueError(f"R={Rr}: the adapter entry points take a multiple of 8 in 8..256")


def lora_b(M: int, Rr: int) -> np.ndarray:
    """float32[M, R]: lora_B[r][j] = ((3 r + 5 j) % 61 - 30) / 32."""
    _check_rank(Rr)
    if M < 1:
        raise ValueError(f"M={M}")
    r, j = np.arange(M, dtype=np.int64)[:, None], np.arange(Rr, dtype=np.int64)[None, :]
    return (((3 * r + 5 * j) % 61 - 30) / 32.0).astype(np.float32)


def lora_a(Rr: int, K: int) -> np.ndarray:
    """float32[R, K]: A[j][k] = ((5 j + 3 k) % 61 - 30) / 32."""
    _check_rank(Rr)
    if K < 8 or K % 8:
        raise ValueError(f"K={K}: the down projection takes a multiple of 8")
    j, k = np.arange(Rr, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    return (((5 * j + 3 * k) % 61 - 30) / 32.0).astype(np.float32)


def down_scale(Rr: int) -> np.ndarray:
    """float32[R]: scale[j] = +-2^(j % 4), the sign alternating every third row (so that it does not follow j % 4)."""
    _check_rank(Rr)
    j = np.arange(Rr)
    return (np.where(j % 3 == 0, -1.0, 1.0) * 2.0 ** (j % 4)).astype(np.float32)


def down_positions(K: int) -> list:
    """one_hot_positions(K) plus the ends of the first 8192-element pass and of the row's last 8-element unit."""
    if K < 8 or K % 8:
        raise ValueError(f"K={K}: the down projection takes a multiple of 8")
    return sorted({k for k in set(one_hot_positions(K)) | {8191, 8192, K - 8, K - 1} if 0 <= k < K})


def deal(positions, rows: int):
    """Positions dealt over launches of `rows` one-hot rows, as one_hot_batches does: (pos int64[L, rows], val float64[L, rows])."""
    if rows < 1 or not len(positions):
        raise ValueError(f"rows={rows}, {len(positions)} positions")
    P = list(positions)
    L = -(-len(P) // rows)
    pos = np.array([[P[(l * rows + b) % len(P)] for b in range(rows)] for l in range(L)], dtype=np.int64)
    val = np.array([[one_hot_value(b, int(pos[l, b])) for b in range(rows)] for l in range(L)], dtype=np.float64)
    return pos, val
