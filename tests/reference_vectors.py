"""Reader of tests/golden/reference_vectors.npz: what the reference's own kernels, run on the CPU (oracle/ref_cpu.py), computed for a
fixed list of inputs.  numpy only; used by the host and the GPU tests alike.  Layout: tests/golden/make_reference_vectors.py."""
from __future__ import annotations

import functools
import hashlib
import os
from dataclasses import dataclass

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.npz")
DTYPES = ("float32", "float16", "bfloat16")
KERNELS = ("tree", "codebook")
FLAVOURS = ("separate", "contracted")
SLICE = 256  # elements of a long case's output that the file keeps beside its digest
_QUIET_NAN = {"float32": 0x7FC00000, "float16": 0x7E00, "bfloat16": 0x7FC0}
_EXP_MANT = {"float32": (0x7F800000, 0x007FFFFF), "float16": (0x7C00, 0x03FF), "bfloat16": (0x7F80, 0x007F)}


@functools.lru_cache(maxsize=1)
def arrays() -> dict:
    return dict(np.load(PATH, allow_pickle=False))


def bits_of(values: np.ndarray, dtype: str) -> np.ndarray:
    """Bit patterns of an array that holds `dtype`: float32 / float16 arrays are viewed, bfloat16 travels as uint16 already."""
    a = np.ascontiguousarray(values)
    if dtype == "bfloat16":
        assert a.dtype == np.uint16
        return a
    assert a.dtype == {"float32": np.float32, "float16": np.float16}[dtype], a.dtype
    return a.view(np.uint32 if dtype == "float32" else np.uint16)


def values_of(bits: np.ndarray, dtype: str) -> np.ndarray:
    """float64 values of bit patterns."""
    b = np.ascontiguousarray(bits)
    if dtype == "float32":
        return b.view(np.float32).astype(np.float64)
    if dtype == "float16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def is_nan_bits(bits: np.ndarray, dtype: str) -> np.ndarray:
    e, m = _EXP_MANT[dtype]
    return ((bits & e) == e) & ((bits & m) != 0)


def digest(bits: np.ndarray, dtype: str) -> np.ndarray:
    """uint8[32]: SHA-256 of the little-endian bit patterns with every NaN replaced by the format's canonical quiet NaN, so that two
    outputs have the same digest exactly when `mismatches` finds none (NaN by class, everything else by bits)."""
    b = np.ascontiguousarray(bits)
    b = np.where(is_nan_bits(b, dtype), b.dtype.type(_QUIET_NAN[dtype]), b).astype(b.dtype.newbyteorder("<"))
    return np.frombuffer(hashlib.sha256(b.tobytes()).digest(), np.uint8).copy()


def mismatches(got_bits: np.ndarray, want_bits: np.ndarray, dtype: str) -> np.ndarray:
    """Indices where two outputs differ: equal bits, or NaN on both sides whatever the payload (NVIDIA's payloads are not in the
    reference's text; everything else, signed zeros and infinities included, is compared by bits)."""
    assert got_bits.shape == want_bits.shape and got_bits.dtype == want_bits.dtype, (got_bits.shape, want_bits.shape, got_bits.dtype)
    same = (got_bits == want_bits) | (is_nan_bits(got_bits, dtype) & is_nan_bits(want_bits, dtype))
    return np.flatnonzero(~same)


def assert_same(got_bits, want_bits, dtype: str, what) -> None:
    bad = mismatches(got_bits, want_bits, dtype)
    assert bad.size == 0, (what, f"{bad.size} of {want_bits.size} differ, first at {int(bad[0])}: "
                                 f"got {int(got_bits[bad[0]]):#x}, recorded {int(want_bits[bad[0]]):#x}")


@dataclass(frozen=True)
class DequantCase:
    name: str
    n: int
    blocksize: int
    packed: np.ndarray
    absmax: np.ndarray
    _out: int

    def recorded(self, kernel: str, dtype: str) -> np.ndarray:
        """Output bit patterns of the reference's `kernel` ("tree" / "codebook") kernel for `dtype`."""
        a = arrays()
        sl = slice(self._out, self._out + self.n)
        tree = a[f"dq_tree_{dtype}"][sl]
        return tree if kernel == "tree" else tree ^ a[f"dq_codebook_xor_tree_{dtype}"][sl]


@dataclass(frozen=True)
class BigDequantCase:
    """A dequant case kept as digests: the recorded output is known through its SHA-256 (NaN canonical) and a 256-element slice."""
    name: str
    n: int
    blocksize: int
    packed: np.ndarray
    absmax: np.ndarray
    slice_at: int
    _index: int

    def recorded_digest(self, kernel: str, dtype: str) -> np.ndarray:
        return arrays()[f"dqbig_sha_{kernel}_{dtype}"][self._index]

    def recorded_slice(self, kernel: str, dtype: str) -> np.ndarray:
        return arrays()[f"dqbig_slice_{kernel}_{dtype}"][self._index * SLICE:(self._index + 1) * SLICE]

    def assert_same(self, got_bits: np.ndarray, kernel: str, dtype: str, what) -> None:
        """The slice first (it says where and what), then the whole output through its digest."""
        assert got_bits.shape == (self.n,)
        assert_same(got_bits[self.slice_at:self.slice_at + SLICE], self.recorded_slice(kernel, dtype), dtype, (what, "slice"))
        assert np.array_equal(digest(got_bits, dtype), self.recorded_digest(kernel, dtype)), (what, "SHA-256 of the whole output differs")


@dataclass(frozen=True)
class GemvCase:
    name: str
    M: int
    K: int
    blocksize: int
    packed: np.ndarray
    absmax: np.ndarray
    plain: bool  # ordinary finite numbers throughout: the cases the error statistic runs over
    _x: int
    _out: int

    def x_bits(self, dtype: str) -> np.ndarray:
        return arrays()[f"gv_x_{dtype}"][self._x:self._x + self.K]

    def x(self, dtype: str) -> np.ndarray:
        """The activation as the kernel reads it (already rounded to `dtype`), as float64."""
        return values_of(self.x_bits(dtype), dtype)

    def recorded(self, dtype: str, flavour: str) -> np.ndarray:
        return arrays()[f"gv_out_{dtype}_{flavour}"][self._out:self._out + self.M]


@functools.lru_cache(maxsize=1)
def dequant_cases() -> tuple:
    a = arrays()
    am = a["dq_absmax_bits"].view(np.float32)
    out = []
    for name, (n, bs, po, ao, oo) in zip(a["dq_names"], a["dq_meta"].tolist()):
        out.append(DequantCase(str(name), n, bs, a["dq_packed"][po:po + (n + 1) // 2], am[ao:ao + -(-n // bs)], oo))
    return tuple(out)


@functools.lru_cache(maxsize=1)
def big_dequant_cases() -> tuple:
    a = arrays()
    am = a["dqbig_absmax_bits"].view(np.float32)
    out = []
    for i, (name, (n, bs, po, ao, at)) in enumerate(zip(a["dqbig_names"], a["dqbig_meta"].tolist())):
        out.append(BigDequantCase(str(name), n, bs, a["dqbig_packed"][po:po + (n + 1) // 2], am[ao:ao + -(-n // bs)], at, i))
    return tuple(out)


@functools.lru_cache(maxsize=1)
def gemv_cases() -> tuple:
    a = arrays()
    am = a["gv_absmax_bits"].view(np.float32)
    out = []
    for name, (M, K, bs, xo, po, ao, oo, plain) in zip(a["gv_names"], a["gv_meta"].tolist()):
        out.append(GemvCase(str(name), M, K, bs, a["gv_packed"][po:po + M * K // 2], am[ao:ao + -(-M * K // bs)], bool(plain), xo, oo))
    return tuple(out)
