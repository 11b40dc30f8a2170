"""Generates tests/golden/reference_vectors.npz: inputs, and what the REFERENCE'S OWN KERNELS computed for them.

The outputs come from oracle/_ref/libref_cpu*.so, i.e. from the reference's kernel text compiled for the CPU by oracle/ref_cpu.py
(one OS thread per CUDA thread) - not from the numpy or C restatement.  The file holds data only: operand bytes, scales, activations
and output bit patterns.  Run from the repo root after oracle/ref_cpu.py has built the libraries (it needs a reference checkout):

    python -m oracle.ref_cpu <reference checkout> && python tests/golden/make_reference_vectors.py

Layout (tests/reference_vectors.py reads it): every group is a few flat arrays plus a meta table of offsets, because a zip member
per case would cost more than the data.  All floating-point values are stored as bit patterns (uint16 / uint32).

  dq_names[c], dq_meta[c] = (n, blocksize, offset into dq_packed, offset into dq_absmax, offset into the outputs)
  dq_packed, dq_absmax_bits, dq_tree_<float32|float16|bfloat16>, dq_codebook_xor_tree_<dtype>: the codebook kernel's output bits
      XOR the tree kernel's (the two agree except at the codes whose table entries differ, so this member is nearly all zeros and
      the file stays under its size limit without dropping a case)
  dqbig_names[c], dqbig_meta[c] = (n, blocksize, offset into dqbig_packed, into dqbig_absmax_bits, first element of the slice):
      cases too long to keep whole.  dqbig_sha_<kernel>_<dtype>[c] is the SHA-256 of the output's little-endian bit patterns with
      every NaN replaced by the format's canonical quiet NaN (tests/reference_vectors.digest), dqbig_slice_<kernel>_<dtype> holds
      256 output elements per case
  gv_names[c], gv_meta[c] = (M, K, blocksize, offset into gv_x_*, into gv_packed, into gv_absmax_bits, into gv_out_*, plain)
  gv_packed, gv_absmax_bits, gv_x_<dtype>, gv_out_<dtype>_<separate|contracted>
  code_param_dequant, code_param_gemv: CODE_PARAM of the two .cu files as their compiler rounds the literals
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_vectors.npz")
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DTYPES = ("float32", "float16", "bfloat16")
KERNELS = ("tree", "codebook")
FLAVOURS = {"separate": False, "contracted": True}

# ---- dequant ---------------------------------------------------------------------------------------------------------------------
# odd n, a partial last thread (16 elements), a partial last tile (1024) and more than one tile
LENGTHS = (1, 2, 15, 16, 17, 1023, 1024, 1025, 2050, 3333)
# 40: blocksize % 16 != 0, where "one absmax per thread of 16 elements" (the reference's rule) and "element // blocksize" differ
BLOCKSIZES = (32, 40, 64, 128, 256, 4096)
FLT_MAX = np.finfo(np.float32).max
EDGE_SCALES = np.array([0.0, 1e-41, FLT_MAX, np.inf, np.nan, -0.75], np.float32)  # +0, subnormal, FLT_MAX, +Inf, NaN, negative


def ordinary_scales(count: int, seed: int) -> np.ndarray:
    """(1 + f) * 2^e with e running through 40 binades, 2^-25 .. 2^14."""
    rng = np.random.default_rng(seed)
    e = ((7 * np.arange(count) + seed) % 40 - 25).astype(np.int32)
    return np.ldexp((1.0 + rng.random(count)).astype(np.float32), e).astype(np.float32)


def grid_scales(count: int, seed: int) -> np.ndarray:
    """Ordinary scales with every fifth block (3, 8, 13, ...) taken from the edge list in turn."""
    am = ordinary_scales(count, seed)
    at = np.arange(3, count, 5)
    am[at] = EDGE_SCALES[(at // 5) % EDGE_SCALES.size]
    return am


def dequant_cases():
    """(name, n, blocksize, packed uint8[(n+1)//2], absmax float32[ceil(n / blocksize)])"""
    cases = []
    for n in LENGTHS:
        packed = np.random.default_rng(1000 + n).integers(0, 256, (n + 1) // 2, dtype=np.uint8)
        for bs in BLOCKSIZES:
            cases.append((f"grid n={n} bs={bs}", n, bs, packed, grid_scales(-(-n // bs), n + bs)))
    for bs in BLOCKSIZES:
        # every byte value in an even-numbered absmax block and again in an odd-numbered one: with h bytes per block, block b holds
        # the h values starting at (b // 2) * h, so blocks 2i and 2i + 1 hold the same bytes under different scales
        h = bs // 2
        nbytes = -(-max(512, 2 * h) // (2 * h)) * 2 * h
        j = np.arange(nbytes)
        packed = ((j // h // 2) * h + j % h) % 256
        for parity in (0, 1):
            assert set(packed[(j // h) % 2 == parity].tolist()) == set(range(256)), (bs, parity)
        cases.append((f"bytes bs={bs}", 2 * nbytes, bs, packed.astype(np.uint8), ordinary_scales(-(-2 * nbytes // bs), bs)))
    for bs in (32, 64):
        # every edge scale meets every nibble code, in both nibble positions; ragged end
        n = 8 * bs + 3
        j = np.arange((n + 1) // 2)
        hi, lo = j % 16, (j // 16 + 5 * j + 3) % 16
        am = ordinary_scales(9, bs)
        am[1:7] = EDGE_SCALES
        cases.append((f"edges bs={bs}", n, bs, ((hi << 4) | lo).astype(np.uint8), am))
    # the sixteen codes in order under a scale of exactly 1.0: the f32 outputs ARE each kernel's table (the tree kernel's literals
    # exist nowhere else)
    codes = ((np.arange(0, 16, 2) << 4) | np.arange(1, 16, 2)).astype(np.uint8)
    cases.append(("codes at scale 1", 16, 64, codes, np.ones(1, np.float32)))
    return cases


# Long enough for a whole tile of every geometry the HIP dequant can be set to (up to 16 loads per lane: 16384 elements of f32 output,
# 32768 of 16-bit output), with a ragged, odd-length tail behind the last tile; edge scales as in the grid.  Kept as digests.
BIG_N = 32768 + 16384 + 77
BIG_SLICE_AT = 32768 - 128  # 256 elements across the end of the first 32768-element tile
BIG_BLOCKSIZES = (32, 64)


def big_dequant_cases():
    """(name, n, blocksize, packed, absmax, first element of the slice)"""
    cases = []
    for bs in BIG_BLOCKSIZES:
        packed = np.random.default_rng(5000 + bs).integers(0, 256, (BIG_N + 1) // 2, dtype=np.uint8)
        cases.append((f"big n={BIG_N} bs={bs}", BIG_N, bs, packed, grid_scales(-(-BIG_N // bs), BIG_N + bs), BIG_SLICE_AT))
    return cases


# ---- GEMV --------------------------------------------------------------------------------------------------------------------------
# (M, K, blocksize): the smallest K (one lane live), K a chunk or two over a 1024 step, M on both sides of the 4 rows a workgroup
# takes, blocksize > K so that rows share a scale
SHAPES = ((5, 32, 64), (6, 96, 32), (7, 1024, 64), (6, 1056, 64), (3, 2080, 128), (2, 4096, 64), (9, 3104, 4096),
          (4, 32, 32), (1, 64, 64), (13, 992, 32))
SPECIAL_SHAPE = (7, 1024, 64)


def to_bits(x: np.ndarray, dtype: str) -> np.ndarray:
    """float32 values -> bit patterns of `dtype`, round to nearest even (numpy's IEEE conversion for fp16; for bf16 the integer
    identity bits + 0x7FFF + lsb, written out here so that the fixture's inputs do not depend on the code under test)."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "float32":
        return x.view(np.uint32).copy()
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16).copy()
    u = x.view(np.uint32).astype(np.uint64)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), out).astype(np.uint16)


def gemv_cases():
    """(name, M, K, blocksize, x float32[K] before rounding to T, packed, absmax, plain) - `plain` marks the cases whose outputs are
    ordinary finite numbers in every dtype (the ones the error statistic runs over)."""
    cases = []
    for M, K, bs in SHAPES:
        rng = np.random.default_rng(100003 * M + K)
        packed = rng.integers(0, 256, M * K // 2, dtype=np.uint8)
        am = rng.uniform(0.005, 0.055, -(-M * K // bs)).astype(np.float32)
        cases.append((f"plain {M}x{K} bs={bs}", M, K, bs, rng.standard_normal(K).astype(np.float32), packed, am, 1))
    M, K, bs = SPECIAL_SHAPE
    rng = np.random.default_rng(77)
    packed = rng.integers(0, 256, M * K // 2, dtype=np.uint8)
    am = rng.uniform(0.005, 0.055, M * K // bs).astype(np.float32)
    x = rng.standard_normal(K).astype(np.float32)
    # fp16-subnormal activations (multiples of 2^-24 below 2^-14) under scales of 2^16, so that the outputs are normal numbers
    sub = (rng.integers(16, 513, K) * rng.choice([-1.0, 1.0], K) * 2.0**-24).astype(np.float32)
    cases.append(("f16-subnormal x", M, K, bs, sub, packed, np.full(M * K // bs, 2.0**16, np.float32), 0))
    xi = x.copy()
    xi[K - 3] = np.inf
    cases.append(("inf in x", M, K, bs, xi, packed, am, 0))
    an = am.copy()
    an.reshape(M, -1)[5, 3] = np.nan
    cases.append(("nan scale row 5", M, K, bs, x, packed, an, 0))
    # the half accumulator overflows: each lane's 32 elements begin with +1.0 * 6e4 twice (6e4 + 6e4 > 65504) and take it back with
    # -1.0 * 6e4 twice, so the exact sum is that of the remaining 28 ordinary terms
    nib = np.stack([packed >> 4, packed & 15], axis=1).reshape(M, K)
    nib[:, 0::32], nib[:, 1::32], nib[:, 2::32], nib[:, 3::32] = 3, 3, 11, 11  # codes +1.0, +1.0, -1.0, -1.0
    flat = nib.reshape(-1)
    po = ((flat[0::2] << 4) | flat[1::2]).astype(np.uint8)
    xo = x.copy()
    xo[0::32] = xo[1::32] = xo[2::32] = xo[3::32] = 6.0e4
    cases.append(("f16 accumulator overflow", M, K, bs, xo, po, np.ones(M * K // bs, np.float32), 0))
    return cases


def generate() -> dict:
    from oracle import ref_cpu

    out = {"code_param_dequant": ref_cpu.code_param(0).view(np.uint32), "code_param_gemv": ref_cpu.code_param(1).view(np.uint32)}
    names, meta, packed_all, am_all = [], [], [], []
    outs = {(k, d): [] for k in KERNELS for d in DTYPES}
    po = ao = oo = 0
    for name, n, bs, packed, am in dequant_cases():
        names.append(name)
        meta.append((n, bs, po, ao, oo))
        packed_all.append(packed)
        am_all.append(am)
        for k in KERNELS:
            for d in DTYPES:
                r = ref_cpu.dequantize(k, packed, am, bs, n, d)
                outs[k, d].append(r.view(np.uint32 if d == "float32" else np.uint16))
        po, ao, oo = po + packed.size, ao + am.size, oo + n
    out["dq_names"], out["dq_meta"] = np.array(names), np.array(meta, np.int64)
    out["dq_packed"], out["dq_absmax_bits"] = np.concatenate(packed_all), np.concatenate(am_all).view(np.uint32)
    for d in DTYPES:
        tree, codebook = np.concatenate(outs["tree", d]), np.concatenate(outs["codebook", d])
        out[f"dq_tree_{d}"], out[f"dq_codebook_xor_tree_{d}"] = tree, codebook ^ tree

    from reference_vectors import SLICE, digest

    names, meta, packed_all, am_all = [], [], [], []
    shas, slices = {(k, d): [] for k in KERNELS for d in DTYPES}, {(k, d): [] for k in KERNELS for d in DTYPES}
    po = ao = 0
    for name, n, bs, packed, am, at in big_dequant_cases():
        names.append(name)
        meta.append((n, bs, po, ao, at))
        packed_all.append(packed)
        am_all.append(am)
        for k in KERNELS:
            for d in DTYPES:
                r = ref_cpu.dequantize(k, packed, am, bs, n, d).view(np.uint32 if d == "float32" else np.uint16)
                shas[k, d].append(digest(r, d))
                slices[k, d].append(r[at:at + SLICE])
        po, ao = po + packed.size, ao + am.size
    out["dqbig_names"], out["dqbig_meta"] = np.array(names), np.array(meta, np.int64)
    out["dqbig_packed"], out["dqbig_absmax_bits"] = np.concatenate(packed_all), np.concatenate(am_all).view(np.uint32)
    for k in KERNELS:
        for d in DTYPES:
            out[f"dqbig_sha_{k}_{d}"], out[f"dqbig_slice_{k}_{d}"] = np.stack(shas[k, d]), np.concatenate(slices[k, d])

    names, meta, packed_all, am_all = [], [], [], []
    xs = {d: [] for d in DTYPES}
    outs = {(d, f): [] for d in DTYPES for f in FLAVOURS}
    xo = po = ao = oo = 0
    for name, M, K, bs, x, packed, am, plain in gemv_cases():
        names.append(name)
        meta.append((M, K, bs, xo, po, ao, oo, plain))
        packed_all.append(packed)
        am_all.append(am)
        for d in DTYPES:
            xb = to_bits(x, d)
            xs[d].append(xb)
            for f, fused in FLAVOURS.items():
                r = ref_cpu.gemv(xb.view(np.float32) if d == "float32" else xb.view(np.float16) if d == "float16" else xb,
                                 packed, am, M, K, bs, d, fused)
                outs[d, f].append(r.view(np.uint32 if d == "float32" else np.uint16))
        xo, po, ao, oo = xo + K, po + packed.size, ao + am.size, oo + M
    out["gv_names"], out["gv_meta"] = np.array(names), np.array(meta, np.int64)
    out["gv_packed"], out["gv_absmax_bits"] = np.concatenate(packed_all), np.concatenate(am_all).view(np.uint32)
    for d in DTYPES:
        out[f"gv_x_{d}"] = np.concatenate(xs[d])
        for f in FLAVOURS:
            out[f"gv_out_{d}_{f}"] = np.concatenate(outs[d, f])
    return out


if __name__ == "__main__":
    from oracle import ref_cpu

    if not ref_cpu.available():
        sys.exit("build oracle/_ref first: python -m oracle.ref_cpu <reference checkout>")
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print("wrote", os.path.relpath(OUT), os.path.getsize(OUT), "bytes,", len(arrays), "arrays,",
          len(arrays["dq_names"]), "dequant cases,", len(arrays["gv_names"]), "GEMV cases")
