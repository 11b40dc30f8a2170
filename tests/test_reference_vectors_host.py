"""The oracle against what the reference's own kernels computed (tests/golden/reference_vectors.npz), without a GPU.

The vectors were recorded from the reference's kernel text compiled for the CPU (oracle/ref_cpu.py, tests/golden/
make_reference_vectors.py).  The first group of tests reads only the committed file and never skips: the numpy oracle and the C
oracle must reproduce every recorded dequant output bit for bit, the GEMV emulation every recorded GEMV output in both contraction
modes, and the two code tables the recorded CODE_PARAMs.  NaN is compared by class (tests/reference_vectors.mismatches).  The
second group needs oracle/_ref (built by __graft_entry__.build() when a reference checkout is at hand): regenerating the vectors
reproduces the committed file, and the sanitized stand-alone self-check of the CPU build exits 0.
"""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import reference_vectors as rv
from oracle import c_oracle, fp4_oracle as o, ref_cpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_bits(values_f32: np.ndarray, dtype: str) -> np.ndarray:
    """Bit patterns of float32 values that are already values of `dtype` (what gemv_reference_emulated returns)."""
    v = np.ascontiguousarray(values_f32, np.float32)
    if dtype == "float32":
        return v.view(np.uint32)
    if dtype == "float16":
        return v.astype(np.float16).view(np.uint16)
    assert ((v.view(np.uint32) & 0xFFFF) == 0)[~np.isnan(v)].all()
    return (v.view(np.uint32) >> 16).astype(np.uint16)


# ---- from the committed file alone ---------------------------------------------------------------------------------------------------
def test_the_case_list_is_the_one_the_vectors_were_asked_for():
    """Lengths x blocksizes x kernels x dtypes, every byte value at both block parities, the edge scales; the ten GEMV shapes and the
    four special activations / scales - so that a regenerated file with fewer cases cannot pass for this one."""
    dq = rv.dequant_cases()
    grid = {(c.n, c.blocksize) for c in dq if c.name.startswith("grid")}
    assert grid == {(n, bs) for n in (1, 2, 15, 16, 17, 1023, 1024, 1025, 2050, 3333) for bs in (32, 40, 64, 128, 256, 4096)}
    for bs in (32, 40, 64, 128, 256, 4096):
        (c,) = [c for c in dq if c.name == f"bytes bs={bs}"]
        block_of_byte = np.arange(c.packed.size) // (bs // 2)
        for parity in (0, 1):
            assert np.unique(c.packed[block_of_byte % 2 == parity]).size == 256
    every = np.concatenate([c.absmax for c in dq])
    assert (every == 0).any() and np.isinf(every).any() and np.isnan(every).any() and (every < 0).any() and (every == np.finfo(np.float32).max).any()
    assert ((every > 0) & (every < np.finfo(np.float32).tiny)).any()
    ordinary = every[np.isfinite(every) & (every > 1e-30) & (every < 1e30)]
    assert np.unique(np.floor(np.log2(ordinary))).size >= 40
    # the long cases: a whole 32768-element tile (the largest geometry the HIP dequant can be set to) and a ragged odd tail, with
    # every edge scale among their blocks
    big = rv.big_dequant_cases()
    assert [(c.n, c.blocksize) for c in big] == [(32768 + 16384 + 77, 32), (32768 + 16384 + 77, 64)]
    for c in big:
        assert np.isnan(c.absmax).any() and np.isinf(c.absmax).any() and (c.absmax == 0).any() and (c.absmax < 0).any()
        assert c.slice_at < 32768 < c.slice_at + rv.SLICE
    gv = rv.gemv_cases()
    assert [(c.M, c.K, c.blocksize) for c in gv if c.plain] == [(5, 32, 64), (6, 96, 32), (7, 1024, 64), (6, 1056, 64), (3, 2080, 128),
                                                               (2, 4096, 64), (9, 3104, 4096), (4, 32, 32), (1, 64, 64), (13, 992, 32)]
    special = {c.name: c for c in gv if not c.plain}
    assert sorted(special) == ["f16 accumulator overflow", "f16-subnormal x", "inf in x", "nan scale row 5"]
    sub = np.abs(special["f16-subnormal x"].x("float16"))
    assert sub.max() < 2.0**-14 and sub.min() >= 2.0**-20
    assert np.isinf(special["inf in x"].x("float16")).sum() == 1 and np.isnan(special["nan scale row 5"].absmax.reshape(7, -1)[5]).sum() == 1
    over = special["f16 accumulator overflow"]
    assert not np.isfinite(rv.values_of(over.recorded("float16", "separate"), "float16")).any()
    assert np.isfinite(rv.values_of(over.recorded("bfloat16", "separate"), "bfloat16")).all()


@pytest.mark.parametrize("dtype", rv.DTYPES)
@pytest.mark.parametrize("kernel", rv.KERNELS)
def test_both_oracles_equal_every_recorded_dequant_output(kernel, dtype):
    for c in rv.dequant_cases():
        want = c.recorded(kernel, dtype)
        with np.errstate(all="ignore"):
            got = o.dequantize(c.packed, c.absmax, c.blocksize, c.n, dtype, kernel)
        rv.assert_same(rv.bits_of(got, dtype), want, dtype, ("numpy oracle", c.name))
        got_c = c_oracle.dequantize(c.packed, c.absmax, c.blocksize, c.n, dtype, kernel)
        rv.assert_same(rv.bits_of(got_c, dtype), want, dtype, ("C oracle", c.name))
    for c in rv.big_dequant_cases():  # kept as SHA-256 + slice
        with np.errstate(all="ignore"):
            got = o.dequantize(c.packed, c.absmax, c.blocksize, c.n, dtype, kernel)
        c.assert_same(rv.bits_of(got, dtype), kernel, dtype, ("numpy oracle", c.name))
        c.assert_same(rv.bits_of(c_oracle.dequantize(c.packed, c.absmax, c.blocksize, c.n, dtype, kernel), dtype), kernel, dtype, ("C oracle", c.name))


@pytest.mark.parametrize("flavour", rv.FLAVOURS)
@pytest.mark.parametrize("dtype", rv.DTYPES)
def test_gemv_emulation_equals_every_recorded_gemv_output(dtype, flavour):
    for c in rv.gemv_cases():
        with np.errstate(all="ignore"):
            got = o.gemv_reference_emulated(c.x(dtype), c.packed, c.absmax, c.M, c.K, c.blocksize, dtype, fused=flavour == "contracted")
        rv.assert_same(oracle_bits(got, dtype), c.recorded(dtype, flavour), dtype, (c.name, flavour))


def test_digest_is_blind_to_nan_payloads_and_to_nothing_else():
    for dtype, np_t in (("float32", np.uint32), ("float16", np.uint16), ("bfloat16", np.uint16)):
        e, m = rv._EXP_MANT[dtype]
        a = np.array([0, 1, e, e | 1, e | m, 0x8000 if np_t is np.uint16 else 0x80000000], np_t)
        b = a.copy()
        b[3], b[4] = e | 2, e | 1 | (a[5])  # other payloads, one with the sign set
        assert np.array_equal(rv.digest(a, dtype), rv.digest(b, dtype)) and rv.mismatches(a, b, dtype).size == 0
        for i in (0, 1, 2, 5):
            c = a.copy()
            c[i] ^= 1 if i != 2 else np_t(a[5])  # one bit elsewhere: +0 -> tiny, tiny -> 0, +Inf -> -Inf, -0 -> -tiny
            assert not np.array_equal(rv.digest(a, dtype), rv.digest(c, dtype)) and rv.mismatches(a, c, dtype).size == 1


def test_the_two_flavours_differ_somewhere():
    """Otherwise the contracted build recorded nothing the separate one did not."""
    for dtype in rv.DTYPES:
        assert any(rv.mismatches(c.recorded(dtype, "separate"), c.recorded(dtype, "contracted"), dtype).size for c in rv.gemv_cases()), dtype


def test_code_tables_equal_both_recorded_code_params():
    a = rv.arrays()
    assert np.array_equal(a["code_param_dequant"], a["code_param_gemv"])  # the GEMV file's copy is the dequant file's
    assert np.array_equal(o.table(o.TABLE_CODEBOOK).view(np.uint32), a["code_param_dequant"])
    assert np.array_equal(c_oracle.table("codebook").view(np.uint32), a["code_param_dequant"])
    # the tree kernel keeps no table in memory: its literals are its f32 outputs for the sixteen codes under a scale of exactly 1.0
    (c,) = [c for c in rv.dequant_cases() if c.name == "codes at scale 1"]
    assert np.array_equal(o.unpack_nibbles(c.packed), np.arange(16)) and c.absmax.tolist() == [1.0]
    assert np.array_equal(c.recorded("codebook", "float32"), a["code_param_dequant"])
    assert np.array_equal(c.recorded("tree", "float32"), o.table(o.TABLE_TREE).view(np.uint32))
    assert np.array_equal(c.recorded("tree", "float32"), c_oracle.table("tree").view(np.uint32))


# ---- with oracle/_ref built --------------------------------------------------------------------------------------------------------------
needs_ref = pytest.mark.skipif(not ref_cpu.available(), reason=ref_cpu.missing())


@needs_ref
def test_regenerating_reproduces_the_committed_file():
    spec = importlib.util.spec_from_file_location("make_reference_vectors", os.path.join(REPO, "tests", "golden", "make_reference_vectors.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh, committed = gen.generate(), rv.arrays()
    assert sorted(fresh) == sorted(committed)
    for key in sorted(committed):
        assert fresh[key].dtype == committed[key].dtype and np.array_equal(fresh[key], committed[key]), key


def test_recipe_refuses_text_without_the_expected_launch_sites():
    for name in ref_cpu.FILES:
        with pytest.raises(ref_cpu.ReferenceChanged):
            ref_cpu.cut_kernel_text(name, "__global__ void some_other_kernel() {}\n")


@pytest.mark.skipif(ref_cpu.find_reference() is None, reason="no reference checkout ($FP4_REFERENCE_DIR, or `reference` next to the repository)")
def test_recipe_cuts_pure_kernel_text_and_notices_a_changed_launch():
    """The launch geometry restated in oracle/ref_cpu/ref_entry.cpp is checked against the reference's launchers at every build:
    the text as it is passes, and a changed block size, grid size, blocksize halving or leading dimension fails the build."""
    ref = ref_cpu.find_reference()
    text = {name: open(os.path.join(ref, "csrc", name + ".cu")).read() for name in ref_cpu.FILES}
    for name in ref_cpu.FILES:
        kept = ref_cpu.cut_kernel_text(name, text[name])
        assert text[name].startswith(kept) and "<<<" not in kept and "torch::" not in kept and "__global__" in kept
    for name, old, new in [("dequant_fp4_optimized", "<<<blocks, 64>>>", "<<<blocks, 128>>>"), ("dequant_fp4_optimized", "CDIV(n, 1024)", "CDIV(n, 512)"),
                           ("dequant_fp4_optimized", "(blocksize / 2)", "(blocksize)"), ("dequant_fp4_optimized", "<T, 512, 64, 8>", "<T, 256, 64, 4>"),
                           ("gemv_fp4_optimized", "<<<num_blocks, 128>>>", "<<<num_blocks, 256>>>"), ("gemv_fp4_optimized", "CDIV(m, 4)", "CDIV(m, 8)"),
                           ("gemv_fp4_optimized", "CDIV(A.sizes()[1], 2)", "A.sizes()[1]")]:
        assert old in text[name]
        with pytest.raises(ref_cpu.ReferenceChanged):
            ref_cpu.cut_kernel_text(name, text[name].replace(old, new, 1))


@needs_ref
def test_sanitized_selfcheck_of_the_cpu_build_exits_clean():
    """oracle/ref_cpu/selfcheck.cpp, compiled with the kernels under AddressSanitizer + UBSan, as programs of their own (both
    flavours side by side): operands of exactly the documented sizes, every entry point, every shape of the case list."""
    procs = [subprocess.Popen([p], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for p in ref_cpu.SELFCHECKS.values()]
    for p in procs:
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0 and "selfcheck ok" in out, out[-3000:]
