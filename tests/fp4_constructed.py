"""Constructed FP4 operands whose GEMV / GEMM result has a closed form, and guard regions around kernel outputs.

Random weights hide a misplaced nibble behind the rounding of a sum over K terms.  Here every activation row is ONE-HOT, so an
output is a single product  code[nibble(r, k)] * absmax[r][k // bs] * x[k]  and a wrong byte, nibble, row, block or activation index
changes it by a factor no rounding explains:

* ``byte_cycle_weight``: packed byte (r + k // 2) % 256 - for a fixed k, 256 consecutive rows run through every byte value at that
  position (both nibbles, both signs, every magnitude);
* ``placement_scales``: absmax[r][j] = 2^(((3 r + 5 j) % 13) - 3) - neighbouring rows and neighbouring blocks always differ (3 and 5
  are units mod 13), every product is exact, and the smallest non-zero |output| (1/192 * 2^-3 * 0.75) is a normal fp16 number;
* ``one_hot_positions``: every k of the first block (all lanes / bytes / nibbles of a packed dword group), then the edges of the
  128 / 256 / 512 / 1024-wide slices the kernels split a row into, the middle of the row and its last block.

Everything here is numpy; torch is only imported by the guard helpers (which take the device as an argument, so that the host test
can prove them on CPU tensors)."""
from __future__ import annotations

import numpy as np

from oracle import fp4_oracle as o

ONE_HOT_VALUES = (1.0, -1.5, 0.75, 3.0)  # exact in bf16, fp16 and f32
SENTINEL16, SENTINEL32, SENTINEL8 = 0x7BCD, 0x7BCD7BCD, 0xA5  # finite in every format; no test output equals them by accident
HALF_ULP = {"bfloat16": 2.0**-8, "float16": 2.0**-11, "float32": 0.0}
F16_MIN_NORMAL = 2.0**-14


def byte_cycle_weight(M: int, K: int) -> np.ndarray:
    """uint8[M * K / 2]: byte k // 2 of weight row r is (r + k // 2) % 256."""
    r = np.arange(M, dtype=np.int64)[:, None]
    j = np.arange(K // 2, dtype=np.int64)[None, :]
    return ((r + j) % 256).astype(np.uint8).reshape(-1)


def nibble(r, k):
    """The 4-bit code of weight (r, k) under byte_cycle_weight: the HIGH nibble of the byte holds the even k."""
    byte = (np.asarray(r, np.int64) + np.asarray(k, np.int64) // 2) % 256
    return np.where(np.asarray(k) % 2 == 0, byte >> 4, byte & 15).astype(np.int64)


def placement_scales(M: int, K: int, bs: int = 64) -> np.ndarray:
    """float32[M * K / bs]: absmax[r][j] = 2^(((3 r + 5 j) % 13) - 3), i.e. 2^-3 .. 2^9."""
    r = np.arange(M, dtype=np.int64)[:, None]
    j = np.arange(K // bs, dtype=np.int64)[None, :]
    return np.ldexp(np.float32(1.0), ((3 * r + 5 * j) % 13 - 3).astype(np.int32)).astype(np.float32).reshape(-1)


def one_hot_positions(K: int) -> list:
    edges = {64, 65, 127, 128, 255, 256, 511, 512, 1023, 1024, K // 2 - 1, K // 2, K - 65, K - 64, K - 2, K - 1}
    return sorted({k for k in set(range(64)) | edges if 0 <= k < K})


def one_hot_value(b: int, k: int) -> float:
    return ONE_HOT_VALUES[(b + k) % 4]


def one_hot_batches(K: int, B: int):
    """The positions of one_hot_positions(K) dealt over launches of B rows: (pos int64[L, B], val float64[L, B]); the last launch
    wraps around to the first positions."""
    P = one_hot_positions(K)
    L = -(-len(P) // B)
    pos = np.array([[P[(l * B + b) % len(P)] for b in range(B)] for l in range(L)], dtype=np.int64)
    val = np.array([[one_hot_value(b, int(pos[l, b])) for b in range(B)] for l in range(L)], dtype=np.float64)
    return pos, val


def one_hot_rows(pos: np.ndarray, val: np.ndarray, K: int) -> np.ndarray:
    """float32[..., K] with val at pos and zeros elsewhere."""
    x = np.zeros(pos.shape + (K,), np.float32)
    np.put_along_axis(x, pos[..., None], val[..., None].astype(np.float32), axis=-1)
    return x


def closed_form(M: int, K: int, pos: np.ndarray, val: np.ndarray, bs: int = 64) -> np.ndarray:
    """float64[..., M]: code[nibble(r, k)] * absmax[r][k // bs] * x for the one-hot rows (pos, val), with the oracle's f32 code
    values (CODE_PARAM, oracle.fp4_oracle.CODEBOOK_TABLE).  Exact: every factor but the code is a small dyadic number."""
    r = np.arange(M, dtype=np.int64)
    k = np.asarray(pos, np.int64)[..., None]
    code = o.CODEBOOK_TABLE.astype(np.float64)[nibble(r, k)]
    am = placement_scales(M, K, bs).reshape(M, K // bs).astype(np.float64)
    return code * am[r, k // bs] * np.asarray(val, np.float64)[..., None]


def kernel_restatement(M: int, K: int, pos: np.ndarray, val: np.ndarray, dtype: str, bs: int = 64) -> np.ndarray:
    """What the 16-bit kernels compute for a one-hot row, in f32 steps: ((12 code * x) * absmax) * f32(1/12), rounded once to
    ``dtype``.  12 code is the exact magnitude set {0, 1/16, 8, 12, 4, 6, 2, 3} (oracle.fp4_oracle.C12_MAG), not 12 x CODE_PARAM."""
    r = np.arange(M, dtype=np.int64)
    k = np.asarray(pos, np.int64)[..., None]
    nib = nibble(r, k)
    c12 = np.where(nib & 8, -o.C12_MAG[nib & 7], o.C12_MAG[nib & 7]).astype(np.float32)
    am = placement_scales(M, K, bs).reshape(M, K // bs)
    t = (c12 * np.asarray(val, np.float32)[..., None]).astype(np.float32)
    t = (t * am[r, k // bs]).astype(np.float32)
    t = (t * np.float32(1.0 / 12.0)).astype(np.float32)
    return o.round_to(dtype)(t).astype(np.float64)


def bar(exact: np.ndarray, scale: np.ndarray, dtype: str) -> np.ndarray:
    """The project's GEMV bar (tests/gpu_util.assert_within_bar): 1.01 ulp_T(y*)/2 + 1e-5 sum |x w|."""
    return HALF_ULP[dtype] * 1.01 * np.abs(exact) + 1e-5 * scale + 1e-30


# ---- guard regions -------------------------------------------------------------------------------------------------------------------
def guard_elems(M: int) -> int:
    """Guard size in elements on either side of an output of rows of length M: at least 4096 and two rows, a multiple of 16 so
    that the guarded view keeps the buffer's 16-byte alignment."""
    return (max(4096, 2 * M) + 15) // 16 * 16


def _sentinel(dtype):
    import torch

    size = torch.empty(0, dtype=dtype).element_size()
    return {1: (torch.uint8, SENTINEL8), 2: (torch.int16, SENTINEL16), 4: (torch.int32, SENTINEL32)}[size]


def guarded(n: int, dtype, guard: int, device):
    """A sentinel-filled buffer holding `n` elements of `dtype` between two guards of `guard` elements: (buffer, the view a kernel
    writes)."""
    import torch

    raw, fill = _sentinel(dtype)
    buf = torch.full((n + 2 * guard,), fill, dtype=raw, device=device)
    buf = buf if raw == dtype else buf.view(dtype)
    return buf, buf[guard:guard + n]


def refill(buf):
    raw, fill = _sentinel(buf.dtype)
    (buf if raw == buf.dtype else buf.view(raw)).fill_(fill)


def untouched(buf, lo: int = 0, hi=None) -> bool:
    raw, fill = _sentinel(buf.dtype)
    return bool(((buf if raw == buf.dtype else buf.view(raw))[lo:hi] == fill).all())


def guards_intact(buf, n: int, guard: int) -> bool:
    return untouched(buf, 0, guard) and untouched(buf, guard + n, None)
