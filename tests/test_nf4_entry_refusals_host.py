"""Every refusal of the nine NF4 decode entry points that tests/test_nf4_mfma_args_host.py does not pin (the six GEMV forms of
csrc/gemv_nf4.hip and the adapter-stack and nested forms of csrc/gemm_wide_nf4.hip), through the C ABI and without a GPU: every call
below is refused, or found empty, before any HIP call.

Each refusal is compared with the status and the WHOLE fp4_hip_last_error() text.  The expectations (tests/golden/nf4_entry_refusals.json)
were recorded from the library as it was when every entry point passed its operands to its entry function as a row of positional
arguments and every form had a block of its own there: one descriptor and one path per entry function have to reproduce all of them
byte for byte, and - the calls with two mistakes at once - in the same ORDER.  `python tests/test_nf4_entry_refusals_host.py` prints
the table of the library it finds as JSON; it is how the fixture was made and it is not how to make a test pass."""
import ctypes
import json
import os

import pytest

import hipabi

OK, INVALID, UNSUPPORTED = hipabi.OK, hipabi.ERR_INVALID, hipabi.ERR_UNSUPPORTED
F16, F32, BF16 = hipabi.F16, hipabi.F32, hipabi.BF16
NONE, GATED = hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS
D = 0x1000  # a 16-byte aligned non-null "pointer": nothing below dereferences it
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nf4_entry_refusals.json")

#          entry point                       gemv,  fused, adapter, stack, nested
ENTRIES = {"fp4_hip_gemv_nf4":             (True,  False, False,   False, False),
           "fp4_hip_gemv_fused_nf4":       (True,  True,  False,   False, False),
           "fp4_hip_gemv_lora_nf4":        (True,  True,  True,    False, False),
           "fp4_hip_gemv_lora_multi_nf4":  (True,  True,  True,    True,  False),
           "fp4_hip_gemv_nested_nf4":      (True,  True,  False,   False, True),
           "fp4_hip_gemv_lora_nested_nf4": (True,  True,  True,    False, True),
           "fp4_hip_gemm_lora_multi_nf4":  (False, True,  True,    True,  False),
           "fp4_hip_gemm_nested_nf4":      (False, True,  False,   False, True),
           "fp4_hip_gemm_lora_nested_nf4": (False, True,  True,    False, True)}


def _signature(entry, v):
    """[(ctype, value)] of one call in the header's argument order; `v` maps argument names to values."""
    gemv, fused, adapter, stack, nested = ENTRIES[entry]
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    a = [(vp, v["x"]), (vp, v["packed"]), (vp, v["absmax"])]
    if nested:
        a += [(vp, v["nested_absmax"]), (vp, v["code256"]), (f32, 0.25), (i32, v["nested_blocksize"])]
    a += [(vp, None)]  # bias
    if fused:
        a += [(vp, None)]  # residual
    if stack:
        a += [(vp, v["lora_B"]), (vp, v["ids"]), (i64, v["n_adapters"]), (vp, v["t"]), (i64, v["R"])]
    elif adapter:
        a += [(vp, v["lora_B"]), (vp, v["t"]), (i64, v["R"])]
    a += [(vp, v["out"])]
    if not gemv:
        a += [(i64, v["B"])]
    a += [(i64, v["M"]), (i64, v["K"]), (i32, v["blocksize"]), (i32, v["dtype"])]
    if fused:
        a += [(i32, v["epilogue"])]
    return a + [(vp, None)]  # stream


def call(entry, **override):
    """One call of `entry` with a valid, covered argument list except for what the caller overrides (an argument the entry point
    does not take is dropped)."""
    v = dict(x=D, packed=D, absmax=D, out=D, B=4, M=64, K=1024 if ENTRIES[entry][0] else 512, blocksize=64, dtype=BF16, epilogue=NONE,
             lora_B=D, t=D, R=8, ids=D, n_adapters=2, nested_absmax=D, code256=D, nested_blocksize=256)
    assert set(override) <= set(v), override
    v.update(override)
    sig = _signature(entry, v)
    f = getattr(hipabi.lib(), entry)
    f.argtypes, f.restype = [t for t, _ in sig], ctypes.c_int
    return f(*[val for _, val in sig])


def refusals(entry):
    """[(label, keyword arguments of `call`)]: every way the entry point's path refuses, then calls with two mistakes at once."""
    gemv, fused, adapter, stack, nested = ENTRIES[entry]
    if gemv:
        cases = [("negative M", dict(M=-1)),
                 ("negative K", dict(K=-2)),
                 ("odd K", dict(K=1023)),
                 ("blocksize 1", dict(blocksize=1)),
                 ("odd blocksize", dict(blocksize=33)),
                 ("unknown dtype", dict(dtype=9)),
                 ("null x", dict(x=None)),
                 ("null packed", dict(packed=None)),
                 ("null absmax", dict(absmax=None)),
                 ("null out", dict(out=None)),
                 ("M too large", dict(M=(1 << 30) + 2)),
                 ("K too large", dict(K=(1 << 30) + 32)),
                 ("unknown dtype, negative M", dict(dtype=9, M=-1)),
                 ("null x, M too large", dict(x=None, M=(1 << 30) + 2))]
        if fused:  # the plain GEMV runs these on the generic kernel
            cases += [("K = 0", dict(K=0)),
                      ("irregular K", dict(K=1040)),
                      ("blocksize 16", dict(blocksize=16)),
                      ("blocksize 48", dict(blocksize=48)),
                      ("blocksize does not divide K", dict(K=1056, blocksize=64)),
                      ("misaligned x", dict(x=D + 8)),
                      ("misaligned packed", dict(packed=D + 4)),
                      ("gate|up with f32", dict(dtype=F32, epilogue=GATED)),
                      ("odd M, gate|up, f32", dict(M=63, dtype=F32, epilogue=GATED)),
                      ("irregular K, null x", dict(K=1040, x=None))]
    else:
        rows = 64 if adapter else 128
        cases = [("negative B", dict(B=-1)),
                 ("negative M", dict(M=-1)),
                 ("K = 0", dict(K=0)),
                 ("blocksize 0", dict(blocksize=0)),
                 ("blocksize 32", dict(blocksize=32)),
                 ("one row too many", dict(B=rows + 1)),
                 ("K off the multiple", dict(K=96)),
                 ("f32", dict(dtype=F32)),
                 ("misaligned x", dict(x=D + 8)),
                 ("misaligned packed", dict(packed=D + 4)),
                 ("M too large", dict(M=(1 << 30) + 2)),
                 ("K too large", dict(K=(1 << 24) + 64)),
                 ("null x", dict(x=None)),
                 ("null packed", dict(packed=None)),
                 ("null absmax", dict(absmax=None)),
                 ("null out", dict(out=None)),
                 ("negative B, f32", dict(B=-1, dtype=F32)),
                 ("f32, null x", dict(dtype=F32, x=None)),
                 ("odd M gate|up, blocksize 32", dict(M=63, epilogue=GATED, blocksize=32))]
    if fused:
        cases += [("odd M, gate|up", dict(M=63, epilogue=GATED)),
                  ("unknown epilogue", dict(epilogue=7)),
                  ("negative epilogue", dict(epilogue=-1)),
                  ("unknown epilogue, negative M", dict(epilogue=7, M=-1)),
                  ("unknown epilogue, M = 0", dict(epilogue=7, M=0))]
    if adapter:
        other_k = 2048 if gemv else 576  # the other side of the hand-over / another K split: the adapter is checked before either
        cases += [("negative R", dict(R=-8)),
                  ("R = 0", dict(R=0)),
                  ("R = 12", dict(R=12)),
                  ("R = 264", dict(R=264)),
                  ("null lora_B", dict(lora_B=None)),
                  ("null t", dict(t=None)),
                  ("misaligned lora_B", dict(lora_B=D + 8)),
                  ("misaligned t", dict(t=D + 4)),
                  ("negative R, null x", dict(R=-8, x=None)),
                  ("negative R, M = 0", dict(R=-8, M=0)),
                  ("R = 12, null x", dict(R=12, x=None)),
                  ("R = 12, null lora_B", dict(R=12, lora_B=None)),
                  ("R = 12, another K", dict(R=12, K=other_k)),
                  ("R = 12, odd M gate|up", dict(R=12, M=63, epilogue=GATED)),
                  ("uncovered K, R = 12", dict(K=1040 if gemv else 96, R=12)),
                  ("unknown epilogue, negative R", dict(epilogue=7, R=-8))]
        if not gemv:
            cases += [("R = 12, 20 rows", dict(R=12, B=20)),
                      ("R = 12, one row too many", dict(R=12, B=65))]
    if stack:
        cases += [("n_adapters = 0", dict(n_adapters=0)),
                  ("negative n_adapters", dict(n_adapters=-3)),
                  ("null ids", dict(ids=None)),
                  ("n_adapters = 0, R = 12", dict(n_adapters=0, R=12)),
                  ("n_adapters = 0, negative R", dict(n_adapters=0, R=-8)),
                  ("n_adapters = 0, null lora_B", dict(n_adapters=0, lora_B=None)),
                  ("n_adapters = 0, null x", dict(n_adapters=0, x=None)),
                  ("n_adapters = 0, uncovered K", dict(n_adapters=0, K=1040 if gemv else 96)),
                  ("null ids, misaligned t", dict(ids=None, t=D + 4))]
    if nested:
        cases += [("nested_blocksize 0", dict(nested_blocksize=0)),
                  ("negative nested_blocksize", dict(nested_blocksize=-256)),
                  ("nested_blocksize 128", dict(nested_blocksize=128)),
                  ("null nested_absmax", dict(nested_absmax=None)),
                  ("null table", dict(code256=None)),
                  ("unknown epilogue, nested_blocksize 0", dict(epilogue=7, nested_blocksize=0)),
                  ("nested_blocksize 0, null table", dict(nested_blocksize=0, code256=None)),
                  ("nested_blocksize 128, null table", dict(nested_blocksize=128, code256=None)),
                  ("nested_blocksize 128, negative M", dict(nested_blocksize=128, M=-1)),
                  ("nested_blocksize 128, M = 0", dict(nested_blocksize=128, M=0)),
                  ("null table, negative M", dict(code256=None, M=-1)),
                  ("null table, K = 0", dict(code256=None, K=0)),
                  ("null table, null x", dict(code256=None, x=None)),
                  ("null table, uncovered K", dict(code256=None, K=1040 if gemv else 96))]
        if adapter:
            cases += [("nested_blocksize 128, R = 12", dict(nested_blocksize=128, R=12)),
                      ("null table, negative R", dict(code256=None, R=-8))]
        if not gemv:
            cases += [("null table, negative B", dict(code256=None, B=-1)),
                      ("null table, B = 0, blocksize 32", dict(code256=None, B=0, blocksize=32))]
    return cases


NULLS = dict(x=None, packed=None, absmax=None, out=None, lora_B=None, t=None, ids=None, nested_absmax=None, code256=None)


def empties(entry):
    """[(label, keyword arguments of `call`)]: empty problems, which are OK whatever the pointers are - where the path says so."""
    gemv, fused, adapter, stack, nested = ENTRIES[entry]
    cases = [("M = 0", dict(M=0, **NULLS))]
    if fused:
        cases += [("M = 0, gate|up", dict(M=0, epilogue=GATED, **NULLS))]
    if gemv:
        cases += [("M = 0, K = 0", dict(M=0, K=0, **NULLS))]
        if fused:
            cases += [("M = 0, irregular K", dict(M=0, K=1040, **NULLS))]
    else:
        cases += [("B = 0", dict(B=0, **NULLS)), ("B = 0, M = 0", dict(B=0, M=0, **NULLS))]
    if adapter:
        cases += [("M = 0, R = 12", dict(M=0, R=12, **NULLS))]
    if stack:
        cases += [("M = 0, n_adapters = 0", dict(M=0, n_adapters=0, **NULLS))]
    return cases


def table():
    """{entry: {label: [status, message]}} of the library that is loaded; an empty problem leaves the message of the refusal before."""
    out = {}
    for entry in ENTRIES:
        rows = out[entry] = {}
        for label, kw in refusals(entry):
            rc = call(entry, **kw)
            rows[label] = [rc, hipabi.last_error()]
        for label, kw in empties(entry):
            assert call(entry, M=-1) == INVALID
            before = hipabi.last_error()
            rc = call(entry, **kw)
            rows["empty: " + label] = [rc, "" if hipabi.last_error() == before else hipabi.last_error()]
    return out


@pytest.fixture(scope="module")
def expected():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_refusals_and_empty_problems_only_and_one_row_per_case(expected):
    assert list(expected) == list(ENTRIES)
    for entry in ENTRIES:
        labels = [label for label, _ in refusals(entry)] + ["empty: " + label for label, _ in empties(entry)]
        assert len(set(labels)) == len(labels), entry
        assert labels == list(expected[entry]), "a case without a recorded message, or the other way round"
        for label, (rc, msg) in expected[entry].items():
            if label.startswith("empty: "):
                assert (rc, msg) == (OK, ""), (entry, label)
            else:  # never a call that would launch
                assert rc in (INVALID, UNSUPPORTED) and msg.startswith(entry + ": "), (entry, label)


def test_the_cases_cover_what_each_path_can_refuse(expected):
    """Each distinct message shape the sources can produce for an entry point occurs in its rows at least once."""
    shapes = {"need M,K >= 0": lambda f: f[0], "need B, M >= 0": lambda f: not f[0], "unsupported dtype": lambda f: f[0],
              "needs an even row count": lambda f: f[1], "null pointer": lambda f: True, "too large": lambda f: f[0],
              "the fused epilogue is not available": lambda f: f[0] and f[1], "is not covered (1..": lambda f: not f[0],
              "unknown epilogue": lambda f: f[1], "(need R >= 0)": lambda f: f[0] and f[2], "the adapter term is not available": lambda f: f[2],
              "need at least one adapter": lambda f: f[3], "need a positive group size": lambda f: f[4], "reads groups of 256 blocks": lambda f: f[4]}
    for entry, feats in ENTRIES.items():
        msgs = [m for _, m in expected[entry].values()]
        for shape, applies in shapes.items():
            assert any(shape in m for m in msgs) == bool(applies(feats)), (entry, shape)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_refusal_has_its_status_and_its_whole_message(entry, expected):
    for label, kw in refusals(entry):
        rc = call(entry, **kw)
        assert [rc, hipabi.last_error()] == expected[entry][label], (entry, label)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_an_empty_problem_is_ok_whatever_the_pointers_are_and_leaves_the_message(entry, expected):
    for label, kw in empties(entry):
        assert call(entry, M=-1) == INVALID
        before = hipabi.last_error()
        assert before == expected[entry]["negative M"][1]
        assert call(entry, **kw) == OK, (entry, label)
        assert hipabi.last_error() == before, (entry, label)


if __name__ == "__main__":
    print(json.dumps(table(), indent=1))
