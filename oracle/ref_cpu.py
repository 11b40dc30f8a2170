"""Builds and loads the reference's own kernels as CPU code.  TEST INFRASTRUCTURE ONLY.

The reference's two kernel files (csrc/dequant_fp4_optimized.cu, csrc/gemv_fp4_optimized.cu) are cut before their first host
launcher and compiled, unedited, as C++20 against the shim of oracle/ref_cpu/ (one OS thread per CUDA thread).  Everything that
holds reference text or is compiled from it goes to oracle/_ref/, which git ignores:

    oracle/_ref/*.cut.inc              the kernel text, byte for byte
    oracle/_ref/libref_cpu.so          every 16-bit `a * b` and `+=` rounded separately, float kernel with -ffp-contract=off
    oracle/_ref/libref_cpu_fused.so    the per-lane `local_C += a * b` as one multiply-add (-DREF_CONTRACT_FMA -ffp-contract=fast -mfma)
    oracle/_ref/selfcheck[_fused]      oracle/ref_cpu/selfcheck.cpp under AddressSanitizer + UBSan, a program of its own

A reference checkout is looked for in $FP4_REFERENCE_DIR, then in a directory `reference` next to this repository.  Without one
nothing can be built; the committed vectors of tests/golden/reference_vectors.npz (recorded from these libraries) still serve every
test that needs the reference's results.

    python -m oracle.ref_cpu [<reference checkout>]
"""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC_DIR = os.path.join(_HERE, "ref_cpu")
OUT_DIR = os.path.join(_HERE, "_ref")
FILES = ("dequant_fp4_optimized", "gemv_fp4_optimized")  # ref_code_param's which_file is the index into this
LIBS = {False: os.path.join(OUT_DIR, "libref_cpu.so"), True: os.path.join(OUT_DIR, "libref_cpu_fused.so")}
SELFCHECKS = {False: os.path.join(OUT_DIR, "selfcheck"), True: os.path.join(OUT_DIR, "selfcheck_fused")}

F16, F32, BF16 = 0, 1, 2
_DT = {"float16": F16, "float32": F32, "bfloat16": BF16}
_KERNEL = {"codebook": 0, "tree": 1}
_NPDT = {"float16": np.float16, "float32": np.float32, "bfloat16": np.uint16}  # bf16 travels as bit patterns

# the first host function of each file: everything before it is kernels, tables and device helpers
_CUT_AT = {
    "dequant_fp4_optimized": "template <typename T>\nvoid launch_dequantize_blockwise_kernel_fp4(",
    "gemv_fp4_optimized": "template <typename T, typename T_REDUCE>\nvoid gemv_4bit_inference_launch(",
}
# (regular expression, how often it must occur) over each WHOLE file: the launch geometry that ref_entry.cpp restates
_LAUNCH_SITES = {
    "dequant_fp4_optimized": [
        (r"<<<", 4),
        (r"<T, 512, 64, 8><<<blocks, 64>>>", 1),
        (r"<(?:float|nv_half|nv_bfloat16), 512, 64, 8><<<blocks, 64>>>", 3),
        (r"const int blocks = CDIV\(n, 1024\);", 2),
        (r"\(const int\)\(blocksize / 2\),?\s*\(const int\)n\s*\);", 4),
        (r"#define CDIV\(x, y\) \(\(\(x\) \+ \(y\)-1\) / \(y\)\)", 1),
    ],
    "gemv_fp4_optimized": [
        (r"<<<", 2),
        (r"<T, 128, T_REDUCE><<<num_blocks, 128>>>", 1),
        (r"<float, 128, float>\s*<<<num_blocks, 128>>>", 1),
        (r">>>\(m, n, k, A, B, absmax, CODE_PARAM, out, lda, ldb, ldc, blocksize\);", 2),
        (r"int num_blocks = CDIV\(m, 4\);", 2),
        (r"int n = 1;", 1), (r"int m = Bshape\[0\];", 1), (r"int k = Bshape\[1\];", 1),
        (r"int ldb = CDIV\(A\.sizes\(\)\[1\], 2\);", 1),
        (r"#define CDIV\(x, y\) \(\(\(x\) \+ \(y\)-1\) / \(y\)\)", 1),
    ],
}


class ReferenceChanged(RuntimeError):
    """The reference's text no longer has the shape this recipe was written for."""


def find_reference(explicit: str | None = None) -> str | None:
    for cand in (explicit, os.environ.get("FP4_REFERENCE_DIR"), os.path.join(os.path.dirname(os.path.dirname(_HERE)), "reference")):
        if cand and all(os.path.isfile(os.path.join(cand, "csrc", f + ".cu")) for f in FILES):
            return os.path.abspath(cand)
    return None


def cut_kernel_text(name: str, text: str) -> str:
    """The part of a reference file that holds its kernels, unedited; raises if the launch sites changed."""
    for pattern, count in _LAUNCH_SITES[name]:
        found = len(re.findall(pattern, text))
        if found != count:
            raise ReferenceChanged(f"{name}.cu: /{pattern}/ occurs {found} times, expected {count}: the launch geometry in "
                                   "oracle/ref_cpu/ref_entry.cpp may no longer be the reference's")
    at = text.find(_CUT_AT[name])
    if at < 0:
        raise ReferenceChanged(f"{name}.cu: first host launcher not found")
    kept = text[:at]
    if "<<<" in kept or "torch::" in kept or "__global__" not in kept:
        raise ReferenceChanged(f"{name}.cu: the text before the first launcher is not pure kernel text any more")
    return kept


def _cxx() -> str:
    """A C++20 host compiler with <barrier> and the sanitizer runtimes: $FP4_REF_CXX, else g++, else clang++."""
    for cand in (os.environ.get("FP4_REF_CXX"), "g++", "clang++"):
        if cand and shutil.which(cand):
            return cand
    raise RuntimeError("no host C++ compiler found")


def _run(cmd) -> str:
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode:
        raise RuntimeError("command failed: " + " ".join(cmd) + "\n" + p.stdout[-4000:])
    return p.stdout


def _flags(fused: bool):
    common = ["-std=c++20", "-O2", "-fPIC", "-pthread", "-w", f"-I{SRC_DIR}", f"-I{os.path.join(SRC_DIR, 'include')}", f"-I{OUT_DIR}"]
    return common + (["-DREF_CONTRACT_FMA", "-ffp-contract=fast", "-mfma"] if fused else ["-ffp-contract=off"])


def _fma_count(fused: bool) -> int:
    """Single-precision fused multiply-adds, scalar or vectorised, in the code generated for a flavour (read from the assembly).
    The only float multiply feeding a float add in the whole translation unit is the float kernel's `local_C += local_A[k] * local_B[k]`."""
    asm = _run([_cxx(), *_flags(fused), "-S", "-o", "-", os.path.join(SRC_DIR, "ref_entry.cpp")])
    return len(re.findall(r"\bvfn?m(?:add|sub)\d*[sp]s\b", asm))


def build(reference: str | None = None, force: bool = False) -> list[str] | None:
    """Cuts the kernel text out of the reference checkout and compiles both library flavours and the sanitized self-checks.
    Returns the paths built, or None when no reference checkout is found."""
    ref = find_reference(reference)
    if ref is None:
        return None
    os.makedirs(OUT_DIR, exist_ok=True)
    newest = 0.0
    for name in FILES:
        kept = cut_kernel_text(name, open(os.path.join(ref, "csrc", name + ".cu")).read())
        inc = os.path.join(OUT_DIR, name + ".cut.inc")
        if not os.path.exists(inc) or open(inc).read() != kept:
            with open(inc, "w") as f:
                f.write(kept)
        newest = max(newest, os.path.getmtime(inc))
    for root, _, files in os.walk(SRC_DIR):
        newest = max([newest] + [os.path.getmtime(os.path.join(root, f)) for f in files])
    newest = max(newest, os.path.getmtime(os.path.abspath(__file__)))
    targets = list(LIBS.values()) + list(SELFCHECKS.values())
    if not force and all(os.path.exists(t) and os.path.getmtime(t) >= newest for t in targets):
        return targets
    entry, selfcheck = os.path.join(SRC_DIR, "ref_entry.cpp"), os.path.join(SRC_DIR, "selfcheck.cpp")
    for fused in (False, True):
        _run([_cxx(), *_flags(fused), "-shared", "-o", LIBS[fused], entry])
        _run([_cxx(), *_flags(fused), "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=undefined", "-o", SELFCHECKS[fused], selfcheck, entry])
    # the two flavours must differ where they claim to: no fused multiply-add in the separate build, some in the contracted one
    separate, contracted = _fma_count(False), _fma_count(True)
    if separate != 0 or contracted == 0:
        raise RuntimeError(f"float GEMV kernel: {separate} FMAs in the separate flavour, {contracted} in the contracted one")
    return targets


def cpu_has_fma() -> bool:
    """The contracted flavour is compiled with -mfma; a CPU without the instruction can build it but not run it."""
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def runnable(fused: bool) -> bool:
    return os.path.exists(LIBS[fused]) and os.path.exists(SELFCHECKS[fused]) and (not fused or cpu_has_fma())


def available() -> bool:
    """Both flavours are built and this CPU can run them."""
    return runnable(False) and runnable(True)


def missing() -> str:
    """Why `available()` is false (for skip reasons)."""
    repo = os.path.dirname(_HERE)
    gone = [os.path.relpath(p, repo) for p in (*LIBS.values(), *SELFCHECKS.values()) if not os.path.exists(p)]
    if gone:
        return "not built (no reference checkout at build time): " + ", ".join(gone)
    return "" if cpu_has_fma() else "this CPU has no FMA, which the contracted flavour (-mfma) needs"


_libs: dict = {}


def lib(fused: bool = False):
    if fused not in _libs:
        if fused and not cpu_has_fma():
            raise RuntimeError("the contracted flavour needs a CPU with FMA (check available() first)")
        l = ctypes.CDLL(LIBS[fused])
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        l.ref_flavour.argtypes, l.ref_flavour.restype = [], i32
        l.ref_code_param.argtypes, l.ref_code_param.restype = [i32, vp], i32
        l.ref_dequant.argtypes, l.ref_dequant.restype = [i32, i32, vp, vp, vp, i32, i32], i32
        l.ref_gemv.argtypes, l.ref_gemv.restype = [i32, vp, vp, vp, vp, i32, i32, i32], i32
        assert l.ref_flavour() == int(fused)
        _libs[fused] = l
    return _libs[fused]


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def code_param(which_file: int) -> np.ndarray:
    """float32[16]: CODE_PARAM of FILES[which_file] as the host compiler rounds its decimal literals."""
    out = np.empty(16, np.float32)
    assert lib().ref_code_param(which_file, _p(out)) == 0
    return out


def dequantize(kernel: str, packed, absmax, blocksize: int, n: int, dtype: str) -> np.ndarray:
    """The reference's tree / codebook dequant kernel; float32 / float16 arrays, uint16 bit patterns for bfloat16."""
    packed = np.ascontiguousarray(packed, np.uint8).reshape(-1)
    absmax = np.ascontiguousarray(absmax, np.float32).reshape(-1)
    assert packed.size >= (n + 1) // 2 and absmax.size >= -(-n // blocksize)
    out = np.empty(n, _NPDT[dtype])
    assert lib().ref_dequant(_KERNEL[kernel], _DT[dtype], _p(packed), _p(absmax), _p(out), blocksize, n) == 0
    return out


def gemv(x, packed, absmax, M: int, K: int, blocksize: int, dtype: str, fused: bool = False) -> np.ndarray:
    """The reference's GEMV kernel for `dtype`; x and the result are arrays of the dtype (uint16 bit patterns for bfloat16)."""
    x = np.ascontiguousarray(x, _NPDT[dtype]).reshape(-1)
    packed = np.ascontiguousarray(packed, np.uint8).reshape(-1)
    absmax = np.ascontiguousarray(absmax, np.float32).reshape(-1)
    assert x.size == K and packed.size >= M * K // 2 and absmax.size >= -(-M * K // blocksize)
    out = np.empty(M, _NPDT[dtype])
    assert lib(fused).ref_gemv(_DT[dtype], _p(x), _p(packed), _p(absmax), _p(out), M, K, blocksize) == 0
    return out


if __name__ == "__main__":
    built = build(sys.argv[1] if len(sys.argv) > 1 else None, force=True)
    if built is None:
        sys.exit("no reference checkout found (argument, $FP4_REFERENCE_DIR, or ../reference)")
    for path in built:
        print("built", os.path.relpath(path))
