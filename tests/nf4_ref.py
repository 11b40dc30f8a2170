"""Test-side restatement of bitsandbytes' NF4 format (numpy), independent of the kernels, plus ctypes bindings of the NF4 entry
points of include/torch_bnb_fp4_hip.h.

bitsandbytes is not installed where these tests run, so its published constants are the spec:
* CODE_DECIMAL - ``get_4bit_type('nf4')`` / the literals of ``dDequantizeNF4``; the f32 table is their f32 rounding.
* THRESHOLD_DECIMAL - the literals of ``dQuantizeNF4``'s decision tree: the midpoints of neighbouring codes.
Quantiser: absmax = max|w| per block, x = w * (1/absmax) in f32, nibble = #{i : x > T[i]} (strict), even element in the high
nibble.  An odd length is padded with one 0.0 in the last block, ranked like any other element: the spare low nibble of the last
byte is rank(0 * (1/absmax)) = 7 for a finite non-zero or an infinite scale, 0 for a zero or NaN one (bitsandbytes' blockwise
quantiser zero-fills its last block and stores ceil(n/2) bytes of what it ranked).  Dequant: out = RN_T(f32(code[nibble]) * absmax).
"""
from __future__ import annotations

import ctypes

import numpy as np

CODE_DECIMAL = [
    -1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
    -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
    0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0,
]
THRESHOLD_DECIMAL = [
    -0.8480964004993439, -0.6106329262256622, -0.4599952697753906, -0.33967943489551544, -0.23460740596055984,
    -0.13791173323988914, -0.045525018125772476, 0.03979014977812767, 0.1202552504837513, 0.2035212516784668,
    0.2920137718319893, 0.3893125355243683, 0.5016634166240692, 0.6427869200706482, 0.8614784181118011,
]

CODE = np.array(CODE_DECIMAL, np.float32)


def midpoint_thresholds() -> np.ndarray:
    """T[i] = f32 rounding of the float64 midpoint of code[i] and code[i+1]."""
    c = CODE.astype(np.float64)
    return ((c[:-1] + c[1:]) / 2).astype(np.float32)


THRESHOLDS = midpoint_thresholds()


def rank(x: np.ndarray) -> np.ndarray:
    """nibble = #{i : x > T[i]} for f32 x (NaN -> 0)."""
    x = np.asarray(x, np.float32)
    # #{T < x} for sorted T is searchsorted(side="left"); numpy sorts NaN last, the compares make it 0
    r = np.searchsorted(THRESHOLDS, x, side="left").astype(np.uint8)
    return np.where(np.isnan(x), np.uint8(0), r)


def rank_tree(x: np.ndarray) -> np.ndarray:
    """bitsandbytes' dQuantizeNF4 decision tree, compare for compare (on the f32 thresholds)."""
    x = np.asarray(x, np.float32).ravel()
    T = THRESHOLDS
    out = np.empty(x.size, np.uint8)
    for j, v in enumerate(x.tolist()):
        v = np.float32(v)
        if v > T[7]:
            if v > T[11]:
                if v > T[13]:
                    out[j] = 15 if v > T[14] else 14
                else:
                    out[j] = 13 if v > T[12] else 12
            else:
                if v > T[9]:
                    out[j] = 11 if v > T[10] else 10
                else:
                    out[j] = 9 if v > T[8] else 8
        else:
            if v > T[3]:
                if v > T[5]:
                    out[j] = 7 if v > T[6] else 6
                else:
                    out[j] = 5 if v > T[4] else 4
            else:
                if v > T[1]:
                    out[j] = 3 if v > T[2] else 2
                else:
                    out[j] = 1 if v > T[0] else 0
    return out


def quantize(w: np.ndarray, blocksize: int):
    """f32 weights -> (packed uint8[ceil(n/2)], absmax f32[ceil(n/bs)])."""
    w = np.asarray(w, np.float32).ravel()
    n = w.size
    nb = -(-n // blocksize)
    pad = np.zeros(nb * blocksize, np.float32)
    pad[:n] = w
    blocks = pad.reshape(nb, blocksize)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        absmax = np.max(np.abs(blocks), axis=1).astype(np.float32)
        inv = (np.float32(1.0) / absmax).astype(np.float32)
        x = (blocks * inv[:, None]).astype(np.float32).ravel()[: n + n % 2]  # odd n: the zero pad of the last block is ranked too
    nib = rank(x)
    packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8)
    return packed, absmax


def gemv_cell(M: int, K: int):
    """(ks, G, iters) of the fast NF4 GEMV kernel for an (M, K) it takes: the rule of dispatch_nf4 (csrc/gemv_nf4.hip:185-200).
    A workgroup covers 2 * (4 / ks) * iters rows and one pass G * 32 * ks chunks of 32 weights."""
    C = K >> 5
    ks = 1 if C <= 32 else (2 if C <= 64 else 4)
    G = 1 if C <= 128 else 2
    iters = 1
    while iters < 4 and M // (2 * (4 // ks) * iters * 2) >= 256:
        iters *= 2
    return ks, G, iters


def rows_per_workgroup(ks: int, iters: int) -> int:
    return 2 * (4 // ks) * iters


# (M, K) cases of tests/test_gpu_nf4_gemv.py: each of the 12 cells twice, once with M a multiple of its rows per workgroup and once
# with a row tail; K with partial last passes (C not a multiple of G * 32 * ks) and several passes (K > 8192)
GEMV_CELL_CASES = [
    (64, 1024), (1023, 992),        # ks 1, G 1, iters 1
    (4096, 1024), (4097, 800),      # ks 1, G 1, iters 2
    (8192, 512), (8193, 736),       # ks 1, G 1, iters 4
    (256, 2048), (2047, 1056),      # ks 2, G 1, iters 1
    (2048, 2048), (2049, 1600),     # ks 2, G 1, iters 2
    (4096, 2048), (4097, 1088),     # ks 2, G 1, iters 4
    (512, 4096), (1023, 2080),      # ks 4, G 1, iters 1
    (1024, 4096), (1025, 3104),     # ks 4, G 1, iters 2
    (2048, 4096), (2049, 4064),     # ks 4, G 1, iters 4
    (512, 8224), (1023, 32768),     # ks 4, G 2, iters 1
    (1024, 14336), (1025, 8224),    # ks 4, G 2, iters 2
    (2048, 32768), (4097, 4128),    # ks 4, G 2, iters 4
]


def unpack(packed: np.ndarray, n: int) -> np.ndarray:
    p = np.asarray(packed, np.uint8).ravel()
    nib = np.empty(p.size * 2, np.uint8)
    nib[0::2] = p >> 4
    nib[1::2] = p & 15
    return nib[:n]


def dequantize_f32(packed: np.ndarray, absmax: np.ndarray, blocksize: int, n: int) -> np.ndarray:
    """f32(code[nibble]) * absmax, one f32 multiply (round this to T for a T output)."""
    nib = unpack(packed, n)
    am = np.asarray(absmax, np.float32)[np.arange(n) // blocksize]
    with np.errstate(invalid="ignore", over="ignore"):
        return (CODE[nib] * am).astype(np.float32)


def gemv_exact(x: np.ndarray, packed: np.ndarray, absmax: np.ndarray, M: int, K: int, blocksize: int):
    """float64 answer of x @ dequant(W)^T and the bar's scale term sum |x w|."""
    w = dequantize_f32(packed, absmax, blocksize, M * K).astype(np.float64).reshape(M, K)
    x64 = np.asarray(x, np.float64)
    return w @ x64, np.abs(w) @ np.abs(x64)


# ---- ctypes bindings of the NF4 entry points (tests/hipabi.py binds the FP4 ones) ----------------------------------------------
TABLE_NF4 = 2


def lib():
    import hipabi

    l = hipabi.lib()
    if not getattr(l, "_nf4_bound", False):
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        l.fp4_hip_gemv_nf4.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]
        l.fp4_hip_gemv_nf4.restype = i32
        l.fp4_hip_quantize_blockwise_nf4.argtypes = [vp, i32, vp, vp, i64, i32, vp]
        l.fp4_hip_quantize_blockwise_nf4.restype = i32
        l._nf4_bound = True
    return l


def code_table() -> np.ndarray:
    out = np.zeros(16, np.float32)
    rc = lib().fp4_hip_code_table(TABLE_NF4, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def gemv(x, packed, absmax, M: int, K: int, blocksize: int, bias=None, out=None):
    import hipabi
    import torch

    if out is None:
        out = torch.empty(M, dtype=x.dtype, device=x.device)
    rc = lib().fp4_hip_gemv_nf4(hipabi._ptr(x), hipabi._ptr(packed), hipabi._ptr(absmax), hipabi._ptr(bias), hipabi._ptr(out), M, K,
                                blocksize, hipabi.DT[x.dtype], hipabi._stream())
    assert rc == 0, (rc, hipabi.last_error())
    return out


def quantize_dev(w, blocksize: int):
    import hipabi
    import torch

    n = w.numel()
    packed = torch.empty((n + 1) // 2, dtype=torch.uint8, device=w.device)
    absmax = torch.empty(-(-n // blocksize), dtype=torch.float32, device=w.device)
    rc = lib().fp4_hip_quantize_blockwise_nf4(hipabi._ptr(w), hipabi.DT[w.dtype], hipabi._ptr(packed), hipabi._ptr(absmax), n, blocksize,
                                              hipabi._stream())
    assert rc == 0, (rc, hipabi.last_error())
    return packed, absmax
