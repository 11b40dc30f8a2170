"""The HIP kernels against what the reference's own kernels computed (tests/golden/reference_vectors.npz).

The vectors were recorded from the reference's kernel text run on the CPU (oracle/ref_cpu.py); this file reads only the committed
fixture.  Dequant is held to the recorded outputs bit for bit (NaN by class) in every tile geometry; the GEMV keeps the project's
two bars of tests/test_gpu_gemv.py, with the reference side of the second one now the recorded kernel outputs instead of an
emulation.  Every case is a few thousand elements at most.
"""
import numpy as np
import pytest
import torch

import fp4_constructed as fc
import hipabi
import reference_vectors as rv
from gpu_util import assert_within_bar, bits, dev, to_dev
from oracle import fp4_oracle as o

pytestmark = pytest.mark.gpu
TORCH_DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
TABLE = {"tree": hipabi.TABLE_TREE, "codebook": hipabi.TABLE_CODEBOOK}
# fp4_hip_set_variant("dequant", loads per lane | streaming << 8): every pair the sweep hook takes, built or not, and the heuristic
DEQUANT_VARIANTS = [-1] + [loads | (nt << 8) for nt in (0, 1) for loads in (1, 2, 4, 8, 16)]


def tile_elems(variant: int, dtype: str) -> int:
    """Elements per workgroup of the tile kernel under a setting: 256 threads x loads x (4 f32 | 8 16-bit values per load).  The
    heuristic (-1) ends at one load per lane for every n below 1024 tiles, i.e. for every recorded case.  Shorter inputs, and
    the tail behind the last whole tile, go to the generic kernel."""
    loads = 1 if variant < 0 else variant & 0xFF
    return 256 * loads * (4 if dtype == "float32" else 8)


def is_built(variant: int, dtype: str) -> bool:
    """f32 output: every geometry.  16-bit output: 1, 2, 4 loads either way and 8 loads with plain stores; the others are refused
    (never computed) as soon as a whole tile fits into n."""
    loads, streaming = (1, 0) if variant < 0 else (variant & 0xFF, variant >> 8)
    return dtype == "float32" or loads <= 4 or (loads == 8 and not streaming)


@pytest.fixture(scope="module")
def dequant_operands():
    return [(c, to_dev(c.packed), to_dev(c.absmax)) for c in rv.dequant_cases() + rv.big_dequant_cases()]


@pytest.mark.parametrize("variant", DEQUANT_VARIANTS)
def test_dequant_equals_the_reference_kernels_bit_for_bit(dequant_operands, variant):
    """fp4_hip_dequantize_blockwise with the tree table against the reference's tree kernel and with the codebook table against its
    codebook kernel, to f32 / f16 / bf16, at every recorded case: ragged ends on either side of a thread's 16 elements and of a
    1024-element tile, blocksize 40 (where the reference's once-per-thread scale lookup is not element // blocksize), every byte
    value under two scales, scales of 0, a subnormal, FLT_MAX, Inf, NaN and a negative number; and the two long cases (whole output
    by SHA-256, NaN canonical, plus a slice), which hold three whole tiles of 16384 elements or one of 32768, edge scales inside
    them, and an odd tail.  Outputs are written between sentinel guards.

    A setting only means something where a whole tile fits: per dtype the test requires that the tile kernel of the setting ran on
    a case with edge scales and a tail behind the last tile, or - for a geometry that is not built - that the call was refused with
    the output untouched.  Which of the two happens is asserted for every single call."""
    tile_runs, refusals = dict.fromkeys(rv.DTYPES, 0), dict.fromkeys(rv.DTYPES, 0)
    try:
        hipabi.set_variant("dequant", variant)
        for c, P, A in dequant_operands:
            for dtype in rv.DTYPES:
                guard = fc.guard_elems(c.n)
                buf, out = fc.guarded(c.n, TORCH_DT[dtype], guard, dev())
                reaches_tiles = c.n >= tile_elems(variant, dtype) and c.blocksize in (32, 64, 128, 256, 4096)  # (40: generic kernel)
                for kernel in rv.KERNELS:
                    fc.refill(buf)
                    rc = hipabi.lib().fp4_hip_dequantize_blockwise(P.data_ptr(), A.data_ptr(), out.data_ptr(), c.blocksize, c.n,
                                                                   hipabi.DT[TORCH_DT[dtype]], TABLE[kernel], hipabi.AUTO, hipabi._stream())
                    what = (c.name, kernel, dtype, variant)
                    if reaches_tiles and not is_built(variant, dtype):
                        assert rc == hipabi.ERR_INVALID and "unknown kernel variant" in hipabi.last_error(), (what, rc, hipabi.last_error())
                        assert fc.untouched(buf), (what, "a refused call wrote")
                        refusals[dtype] += 1
                        continue
                    assert rc == hipabi.OK, (what, rc, hipabi.last_error())
                    if isinstance(c, rv.BigDequantCase):
                        c.assert_same(bits(out), kernel, dtype, what)
                        tile_runs[dtype] += reaches_tiles and c.n % tile_elems(variant, dtype) != 0
                    else:
                        rv.assert_same(bits(out), c.recorded(kernel, dtype), dtype, what)
                    assert fc.guards_intact(buf, c.n, guard), what
    finally:
        hipabi.set_variant("dequant", -1)
    for dtype in rv.DTYPES:
        if is_built(variant, dtype):
            assert tile_runs[dtype] == 2 * len(rv.big_dequant_cases()) and refusals[dtype] == 0, (dtype, tile_runs, refusals)
        else:
            assert refusals[dtype] == 2 * len(rv.big_dequant_cases()) and tile_runs[dtype] == 0, (dtype, tile_runs, refusals)


def gemv_operands(c, dtype):
    raw = c.x_bits(dtype)
    x_t = torch.from_numpy(raw.view(np.int32 if dtype == "float32" else np.int16).copy()).view(TORCH_DT[dtype]).to(dev())
    with np.errstate(all="ignore"):
        w = o.dequantize_f32(c.packed, c.absmax, c.blocksize, c.M * c.K).astype(np.float64).reshape(c.M, c.K)
        xv = c.x(dtype)
        exact, scale = o.gemv_exact(xv, c.packed, c.absmax, c.M, c.K, c.blocksize), np.abs(w) @ np.abs(xv)
    return x_t, exact, scale


@pytest.fixture(scope="module")
def gemv_results():
    """{(case name, dtype): (case, y, float64 product, sum |x w|)}: one launch per recorded case and dtype, shared by the tests."""
    out = {}
    for c in rv.gemv_cases():
        P, A = to_dev(c.packed), to_dev(c.absmax)
        for dtype in rv.DTYPES:
            x_t, exact, scale = gemv_operands(c, dtype)
            guard = fc.guard_elems(c.M)
            buf, y = fc.guarded(c.M, TORCH_DT[dtype], guard, dev())
            hipabi.gemv(x_t, P, A, c.M, c.K, c.blocksize, out=y)
            assert fc.guards_intact(buf, c.M, guard), (c.name, dtype)
            out[c.name, dtype] = (c, y.clone(), exact, scale)
    return out


FINITE_CASES = [c.name for c in rv.gemv_cases() if c.plain] + ["f16-subnormal x", "f16 accumulator overflow"]


@pytest.mark.parametrize("dtype", rv.DTYPES)
def test_gemv_meets_the_bar_at_every_recorded_case(gemv_results, dtype):
    """Bar 1 of tests/test_gpu_gemv.py against the float64 product (oracle.gemv_exact's arithmetic) on the reference's own shapes:
    one live lane (K = 32), K one and two chunks past a 1024 step, M on both sides of a workgroup's four rows, scales shared
    between rows (blocksize > K); fp16-subnormal activations; and the input on which the reference's half accumulator overflows
    (6e4 + 6e4), where an f32 accumulator must still give the exact sum's rounding."""
    for name in FINITE_CASES:
        c, y, exact, scale = gemv_results[name, dtype]
        assert np.isfinite(exact).all() and np.abs(exact).max() < 6.0e4, name
        assert_within_bar(y, exact, scale, TORCH_DT[dtype])


@pytest.mark.parametrize("dtype", rv.DTYPES)
def test_gemv_is_no_worse_than_the_reference_kernels_outputs(gemv_results, dtype):
    """Bar 2 of tests/test_gpu_gemv.py (mean |error| against the float64 product no larger than the reference's, margin 1.05) with
    the reference side taken from the recorded outputs of its own kernel (separate roundings).

    fp16 / bf16: per case, as in that file.  The reference accumulates each lane's 32 products in T and this kernel in f32, so the
    statistic has to hold at every shape, one live lane (K = 32) and a single row (M = 1) included.
    f32: both sides accumulate in f32 and differ only in the order of the additions, so a mean over the 1 to 13 rows of one case
    is decided by individual roundings; the statistic runs over the 56 rows of the ten plain cases together.  (A regression of the
    f32 kernel at a small K is bar 1's to catch: half an ulp is 0 for f32, so that bar is 1e-5 sum |x w| at every row.)"""
    mine, theirs = [], []
    for name in FINITE_CASES[:10]:
        c, y, exact, scale = gemv_results[name, dtype]
        ref = rv.values_of(c.recorded(dtype, "separate"), dtype)
        mine.append(np.abs(y.double().cpu().numpy() - exact))
        theirs.append(np.abs(ref - exact))
        print(f"{name} {dtype}: mean |err| {mine[-1].mean():.3e}, reference kernel {theirs[-1].mean():.3e}; "
              f"over sum |x w|: {(mine[-1] / scale).mean():.3e}, {(theirs[-1] / scale).mean():.3e}")
        if dtype != "float32":
            assert mine[-1].mean() <= theirs[-1].mean() * 1.05 + 1e-12, (name, mine[-1].mean(), theirs[-1].mean())
    err, ref_err = np.concatenate(mine), np.concatenate(theirs)
    assert err.size == 56
    print(f"all {err.size} rows {dtype}: mean |err| {err.mean():.3e}, reference kernel {ref_err.mean():.3e}")
    assert err.mean() <= ref_err.mean() * 1.05 + 1e-12, (err.mean(), ref_err.mean())


@pytest.mark.parametrize("dtype", rv.DTYPES)
def test_gemv_non_finite_inputs_spoil_their_own_rows_only(gemv_results, dtype):
    """What tests/test_gpu_fp4_constructed.py asserts for such inputs: an infinite activation spoils every row it meets, a NaN scale
    its own row, and every other row is at the bar.  (No equality with the reference here: it, too, returns non-finite rows.)"""
    c, y, _, _ = gemv_results["inf in x", dtype]
    assert not np.isfinite(y.double().cpu().numpy()).any()
    assert not np.isfinite(rv.values_of(c.recorded(dtype, "separate"), dtype)).any()
    c, y, exact, scale = gemv_results["nan scale row 5", dtype]
    got = y.double().cpu().numpy()
    keep = [r for r in range(c.M) if r != 5]
    assert not np.isfinite(got[5]) and np.isfinite(got[keep]).all()
    assert_within_bar(y[keep], exact[keep], scale[keep], TORCH_DT[dtype])
