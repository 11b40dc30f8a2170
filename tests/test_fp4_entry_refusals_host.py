"""Every refusal of the six FP4 decode entry points (the GEMV of csrc/gemv_fp4.hip: plain, fused, partial; the small-batch GEMM of
csrc/gemm_small_fp4.hip: plain, fused, with a workspace) and what fp4_hip_gemm_small_ws_bytes answers without asking the device,
through the C ABI and without a GPU: every call below is refused, or found empty, before any HIP call.

Each refusal is compared with the status and the WHOLE fp4_hip_last_error() text.  The expectations (tests/golden/fp4_entry_refusals.json)
were recorded from the library as it was when every host function of these files passed its operands as a row of positional arguments:
one descriptor (csrc/fp4_call.h) has to reproduce all of them byte for byte, and - the calls with two mistakes at once - in the same
ORDER.  The messages keep their quirks: the fused entry points report as fp4_hip_gemv / fp4_hip_gemm_small, except for the odd row
count under the gate|up epilogue; the f32 small-batch rows forward the GEMV's text; above 16 rows the message names the row count of
the first even chunk, which pins the chunk split.  `python tests/test_fp4_entry_refusals_host.py` prints the table of the library it
finds as JSON; it is how the fixture was made and it is not how to make a test pass.

Left out on purpose: every shape a kernel covers (K == 0 with M > 0 on the plain and partial GEMV is a valid launch), and every
_ws / _ws_bytes call that would ask the device for its CU count (33..64 rows or 65..128 halved, blocksize 64, K % 64 == 0, K >= 8192,
a 16-bit dtype).

The one behaviour that is NOT a record of the earlier library is at the end: a workspace with a weight of another blocksize than 64."""
import ctypes
import json
import os

import pytest

import hipabi

OK, INVALID, UNSUPPORTED = hipabi.OK, hipabi.ERR_INVALID, hipabi.ERR_UNSUPPORTED
F16, F32, BF16 = hipabi.F16, hipabi.F32, hipabi.BF16
NONE, GATED = hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS
D = 0x1000  # a 16-byte aligned non-null "pointer": nothing below dereferences it
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp4_entry_refusals.json")
WS_BYTES = "fp4_hip_gemm_small_ws_bytes"

#          entry point                   gemv,  fused, ws     (fused: takes a residual and an epilogue; ws: and a workspace)
ENTRIES = {"fp4_hip_gemv":             (True,  False, False),
           "fp4_hip_gemv_fused":       (True,  True,  False),
           "fp4_hip_gemv_partial":     (True,  False, False),
           "fp4_hip_gemm_small":       (False, False, False),
           "fp4_hip_gemm_small_fused": (False, True,  False),
           "fp4_hip_gemm_small_ws":    (False, True,  True)}


def _signature(entry, v):
    """[(ctype, value)] of one call in the header's argument order; `v` maps argument names to values."""
    gemv, fused, ws = ENTRIES[entry]
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    a = [(vp, v["x"]), (vp, v["packed"]), (vp, v["absmax"])]
    if entry != "fp4_hip_gemv_partial":
        a += [(vp, None)]  # bias
    if fused:
        a += [(vp, None)]  # residual
    a += [(vp, v["out"])]
    if not gemv:
        a += [(i64, v["B"])]
    a += [(i64, v["M"]), (i64, v["K"]), (i32, v["blocksize"]), (i32, v["dtype"])]
    if fused:
        a += [(i32, v["epilogue"])]
    if ws:
        a += [(vp, v["workspace"]), (i64, v["workspace_bytes"])]
    return a + [(vp, None)]  # stream


def call(entry, **override):
    """One call of `entry` with a valid, covered argument list except for what the caller overrides (an argument the entry point
    does not take is dropped)."""
    v = dict(x=D, packed=D, absmax=D, out=D, B=4, M=64, K=1024 if ENTRIES[entry][0] else 512, blocksize=64, dtype=BF16, epilogue=NONE,
             workspace=None, workspace_bytes=0)
    assert set(override) <= set(v), override
    v.update(override)
    sig = _signature(entry, v)
    f = getattr(hipabi.lib(), entry)
    f.argtypes, f.restype = [t for t, _ in sig], ctypes.c_int
    return f(*[val for _, val in sig])


def ws_bytes(B=40, M=64, K=8192, blocksize=64, dtype=BF16):
    f = getattr(hipabi.lib(), WS_BYTES)
    f.argtypes, f.restype = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int], ctypes.c_int64
    return f(B, M, K, blocksize, dtype)


BIG = (1 << 30) + 2
WS = dict(workspace=D, workspace_bytes=1 << 20)


def refusals(entry):
    """[(label, keyword arguments of `call`)]: every way the entry point's path refuses, then calls with two mistakes at once."""
    gemv, fused, ws = ENTRIES[entry]
    if gemv:
        cases = [("negative M", dict(M=-1)),
                 ("negative K", dict(K=-2)),
                 ("odd K", dict(K=1023)),
                 ("blocksize 0", dict(blocksize=0)),
                 ("blocksize 1", dict(blocksize=1)),
                 ("blocksize 33", dict(blocksize=33)),
                 ("negative blocksize", dict(blocksize=-64)),
                 ("unknown dtype", dict(dtype=9)),
                 ("negative dtype", dict(dtype=-1)),
                 ("null out", dict(out=None)),
                 ("null x", dict(x=None)),
                 ("null packed", dict(packed=None)),
                 ("null absmax", dict(absmax=None)),
                 ("null out, K = 0", dict(out=None, K=0)),
                 ("M too large", dict(M=BIG)),
                 ("K too large", dict(K=(1 << 30) + 32)),
                 ("unknown dtype, negative M", dict(dtype=9, M=-1)),
                 ("unknown dtype, M = 0", dict(dtype=9, M=0)),
                 ("unknown dtype, null x", dict(dtype=9, x=None)),
                 ("null x, M too large", dict(x=None, M=BIG)),
                 ("odd K, blocksize 33", dict(K=1023, blocksize=33))]
        if fused:
            g = dict(epilogue=GATED)
            cases += [("unknown epilogue", dict(epilogue=7)),
                      ("negative epilogue", dict(epilogue=-1)),
                      ("unknown epilogue, negative M", dict(epilogue=7, M=-1)),
                      ("unknown epilogue, M = 0", dict(epilogue=7, M=0)),
                      ("gate|up, odd M", dict(M=63, **g)),
                      ("unknown dtype, gate|up odd M", dict(dtype=9, M=63, **g)),
                      ("gate|up odd M, null x", dict(M=63, x=None, **g)),
                      ("gate|up, null out", dict(out=None, **g)),
                      ("gate|up, M too large", dict(M=BIG, **g)),
                      ("gate|up, f32", dict(dtype=F32, **g)),
                      ("gate|up, K = 0", dict(K=0, **g)),
                      ("gate|up, K = 1040", dict(K=1040, **g)),
                      ("gate|up, blocksize 16", dict(blocksize=16, **g)),
                      ("gate|up, blocksize 48", dict(blocksize=48, **g)),
                      ("gate|up, blocksize does not divide K", dict(K=1056, **g)),
                      ("gate|up, misaligned x", dict(x=D + 8, **g)),
                      ("gate|up, misaligned packed", dict(packed=D + 4, **g)),
                      ("gate|up, K = 32768", dict(K=32768, **g)),
                      ("gate|up, K = 32768, f16", dict(K=32768, dtype=F16, **g)),
                      ("gate|up, K beyond the LDS", dict(K=1 << 20, **g)),
                      ("gate|up, f32, null x", dict(dtype=F32, x=None, **g))]
        return cases
    cases = [("B = -1", dict(B=-1)),
             ("B = 129", dict(B=129)),
             ("negative M", dict(M=-1)),
             ("K = 0", dict(K=0)),
             ("negative K", dict(K=-512)),
             ("B = 129, f32", dict(B=129, dtype=F32)),
             ("K = 0, null x", dict(K=0, x=None)),
             ("f32, 9 rows", dict(dtype=F32, B=9)),
             ("f32, null x", dict(dtype=F32, x=None)),
             ("f32, null out", dict(dtype=F32, out=None)),
             ("f32, odd K", dict(dtype=F32, K=511)),
             ("f32, 8 rows, blocksize 33", dict(dtype=F32, B=8, blocksize=33)),
             ("f32, null packed", dict(dtype=F32, packed=None)),
             ("f32, M too large", dict(dtype=F32, M=BIG)),
             ("f32, 9 rows, null x", dict(dtype=F32, B=9, x=None)),
             ("4 rows: null x", dict(x=None)),
             ("4 rows: null packed", dict(packed=None)),
             ("4 rows: null absmax", dict(absmax=None)),
             ("4 rows: null out", dict(out=None)),
             ("4 rows: unknown dtype", dict(dtype=9)),
             ("4 rows: blocksize 16", dict(blocksize=16)),
             ("4 rows: blocksize 48", dict(blocksize=48)),
             ("4 rows: blocksize 0", dict(blocksize=0)),
             ("4 rows: K = 1040", dict(K=1040)),
             ("4 rows: blocksize does not divide K", dict(K=1056)),
             ("4 rows: misaligned x", dict(x=D + 8)),
             ("4 rows: misaligned packed", dict(packed=D + 4)),
             ("4 rows: M too large", dict(M=BIG)),
             ("4 rows: K too large", dict(K=(1 << 24) + 512)),
             ("4 rows: null x, unknown dtype", dict(x=None, dtype=9)),
             ("1 row: blocksize 16", dict(B=1, blocksize=16)),
             ("16 rows: blocksize 32", dict(B=16, blocksize=32)),
             ("12 rows, blocksize 128", dict(B=12, blocksize=128)),
             ("9 rows, K = 96", dict(B=9, K=96)),
             ("8 rows, blocksize 128, K = 32768", dict(B=8, blocksize=128, K=32768)),
             ("17 rows, blocksize 32", dict(B=17, blocksize=32)),
             ("40 rows, blocksize 32", dict(B=40, blocksize=32)),
             ("64 rows, blocksize 32", dict(B=64, blocksize=32)),
             ("65 rows, blocksize 32", dict(B=65, blocksize=32)),
             ("128 rows, blocksize 32", dict(B=128, blocksize=32)),
             ("33 rows, blocksize 128", dict(B=33, blocksize=128)),
             ("17 rows: unknown dtype", dict(B=17, dtype=9)),
             ("17 rows: K = 96, blocksize 64", dict(B=17, K=96)),
             ("17 rows: null out", dict(B=17, out=None)),
             ("17 rows: null x", dict(B=17, x=None)),
             ("17 rows: misaligned x", dict(B=17, x=D + 8)),
             ("40 rows: M too large", dict(B=40, M=BIG)),
             ("128 rows: null absmax", dict(B=128, absmax=None)),
             ("65 rows: unknown dtype, null x", dict(B=65, dtype=9, x=None))]
    if fused:
        g = dict(epilogue=GATED)
        cases += [("unknown epilogue", dict(epilogue=7)),
                  ("negative epilogue", dict(epilogue=-1)),
                  ("unknown epilogue, B = -1", dict(epilogue=7, B=-1)),
                  ("unknown epilogue, B = 0", dict(epilogue=7, B=0)),
                  ("gate|up, odd M", dict(M=63, **g)),
                  ("gate|up odd M, B = 0", dict(M=63, B=0, **g)),
                  ("gate|up odd M, K = 0", dict(M=63, K=0, **g)),
                  ("gate|up odd M, 40 rows", dict(M=63, B=40, **g)),
                  ("gate|up, f32", dict(dtype=F32, **g)),
                  ("gate|up, f32, odd M", dict(dtype=F32, M=63, **g)),
                  ("gate|up, 4 rows, blocksize 16", dict(blocksize=16, **g)),
                  ("gate|up, 40 rows, blocksize 32", dict(B=40, blocksize=32, **g)),
                  ("gate|up, 65 rows, null out", dict(B=65, out=None, **g))]
    if ws:  # a workspace given: the split-K path turns every one of these down before it asks the device (K < 8192), then as above
        cases += [("workspace: 40 rows, blocksize 32", dict(B=40, blocksize=32, **WS)),
                  ("workspace: 65 rows, blocksize 32", dict(B=65, blocksize=32, **WS)),
                  ("workspace: 128 rows, blocksize 32", dict(B=128, blocksize=32, **WS)),
                  ("workspace: 127 rows, blocksize 128", dict(B=127, blocksize=128, **WS)),
                  ("workspace: 65 rows, K = 96", dict(B=65, K=96, **WS)),
                  ("workspace: 65 rows, null out", dict(B=65, out=None, **WS)),
                  ("workspace: 65 rows, null x", dict(B=65, x=None, **WS)),
                  ("workspace: 65 rows, unknown dtype", dict(B=65, dtype=9, **WS)),
                  ("workspace: 40 rows, null absmax", dict(B=40, absmax=None, **WS)),
                  ("workspace: 40 rows, gate|up odd M", dict(B=40, M=63, epilogue=GATED, **WS)),
                  ("workspace: 128 rows, gate|up odd M", dict(B=128, M=63, epilogue=GATED, **WS)),
                  ("workspace: unknown epilogue", dict(B=40, epilogue=7, **WS)),
                  ("workspace: B = 129", dict(B=129, **WS)),
                  ("workspace: 4 rows, blocksize 16", dict(blocksize=16, **WS)),
                  ("workspace: f32, 9 rows", dict(dtype=F32, B=9, **WS))]
    return cases


NULLS = dict(x=None, packed=None, absmax=None, out=None)


def empties(entry):
    """[(label, keyword arguments of `call`)]: empty problems, which are OK whatever the pointers are - where the path says so."""
    gemv, fused, ws = ENTRIES[entry]
    cases = [("M = 0", dict(M=0, **NULLS))]
    if fused:
        cases += [("M = 0, gate|up", dict(M=0, epilogue=GATED, **NULLS))]
    if gemv:
        cases += [("M = 0, K = 0", dict(M=0, K=0, **NULLS)),
                  ("M = 0, f32, blocksize 2", dict(M=0, dtype=F32, blocksize=2, **NULLS))]
    else:
        cases += [("B = 0", dict(B=0, **NULLS)),
                  ("B = 0, M = 0", dict(B=0, M=0, **NULLS)),
                  ("B = 0, unknown dtype, blocksize 0", dict(B=0, dtype=9, blocksize=0, **NULLS)),
                  ("M = 0, unknown dtype", dict(M=0, dtype=9, **NULLS)),
                  ("M = 0, f32", dict(M=0, dtype=F32, **NULLS)),
                  ("M = 0, 17 rows", dict(M=0, B=17, **NULLS)),
                  ("M = 0, 65 rows", dict(M=0, B=65, **NULLS)),
                  ("M = 0, 128 rows, blocksize 32", dict(M=0, B=128, blocksize=32, **NULLS))]
    if ws:
        cases += [("workspace: M = 0, 65 rows", dict(M=0, B=65, **NULLS, **WS)),
                  ("workspace: M = 0, 40 rows", dict(M=0, B=40, **NULLS, **WS)),
                  ("workspace: B = 0", dict(B=0, **NULLS, **WS))]
    return cases


def ws_bytes_cases():
    """[(label, keyword arguments of `ws_bytes`)]: the shapes the split-K path is not for, each answered before the CU count is read."""
    return [("32 rows", dict(B=32)),
            ("129 rows", dict(B=129)),
            ("B = 0", dict(B=0)),
            ("B = -40", dict(B=-40)),
            ("blocksize 32", dict(blocksize=32)),
            ("blocksize 128", dict(blocksize=128)),
            ("K = 8160", dict(K=8160)),
            ("K = 4096", dict(K=4096)),
            ("f32", dict(dtype=F32)),
            ("unknown dtype", dict(dtype=9)),
            ("65 rows, blocksize 32", dict(B=65, blocksize=32)),
            ("128 rows, K = 4096", dict(B=128, K=4096))]


def _message_after(entry, kw):
    """(status, message) of an empty problem: "" where the call left the message of the refusal before it alone."""
    assert call(entry, M=-1) == INVALID
    before = hipabi.last_error()
    rc = call(entry, **kw)
    return rc, "" if hipabi.last_error() == before else hipabi.last_error()


def table():
    """{entry: {label: [status, message]}} of the library that is loaded, and {label: bytes} for fp4_hip_gemm_small_ws_bytes."""
    out = {}
    for entry in ENTRIES:
        rows = out[entry] = {}
        for label, kw in refusals(entry):
            rc = call(entry, **kw)
            rows[label] = [rc, hipabi.last_error()]
        for label, kw in empties(entry):
            rows["empty: " + label] = list(_message_after(entry, kw))
    out[WS_BYTES] = {label: ws_bytes(**kw) for label, kw in ws_bytes_cases()}
    return out


@pytest.fixture(scope="module")
def expected():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_refusals_and_empty_problems_only_and_one_row_per_case(expected):
    assert list(expected) == list(ENTRIES) + [WS_BYTES]
    for entry in ENTRIES:
        labels = [label for label, _ in refusals(entry)] + ["empty: " + label for label, _ in empties(entry)]
        assert len(set(labels)) == len(labels), entry
        assert labels == list(expected[entry]), "a case without a recorded message, or the other way round"
        for label, (rc, msg) in expected[entry].items():
            if label.startswith("empty: "):
                assert (rc, msg) == (OK, ""), (entry, label)
            else:  # never a call that would launch; the reporting name is the family's, not always the entry point's
                assert rc in (INVALID, UNSUPPORTED) and msg.startswith(("fp4_hip_gemv", "fp4_hip_gemm_small")), (entry, label)
    assert [label for label, _ in ws_bytes_cases()] == list(expected[WS_BYTES])
    assert set(expected[WS_BYTES].values()) == {0}


def test_the_cases_cover_what_each_path_can_refuse(expected):
    """Each distinct message shape the sources can produce before a launch occurs in the rows of the entry points it applies to."""
    shapes = {"need M,K >= 0": lambda f: True,  # the small-batch f32 rows forward it
              "unsupported dtype": lambda f: f[0],
              "fp4_hip_gemv_fused: the gate|up epilogue needs an even row count": lambda f: f[0] and f[1],
              "fp4_hip_gemm_small_fused: the gate|up epilogue needs an even row count": lambda f: not f[0] and f[1],
              "fp4_hip_gemv: null pointer": lambda f: True,
              "fp4_hip_gemm_small: null pointer": lambda f: not f[0],
              "too large": lambda f: True,
              "the gate|up epilogue is not available": lambda f: f[0] and f[1],
              "need 0 <= B <= 128": lambda f: not f[0],
              "f32 activations are covered up to 8 rows": lambda f: not f[0],
              "more than 16 rows need a 16-bit dtype": lambda f: not f[0],
              "is not covered; use dequant + GEMM": lambda f: not f[0],
              "unknown epilogue": lambda f: f[1]}
    for entry, feats in ENTRIES.items():
        msgs = [m for _, m in expected[entry].values()]
        for shape, applies in shapes.items():
            assert any(shape in m for m in msgs) == bool(applies(feats)), (entry, shape)
    # the unknown epilogue is reported under the entry point's own name, the three of them apart
    for entry, feats in ENTRIES.items():
        if feats[1]:
            assert expected[entry]["unknown epilogue"] == [INVALID, entry + ": unknown epilogue 7"]


def test_the_first_chunk_of_more_than_16_rows_has_the_recorded_row_count(expected):
    """17, 40, 64, 65 and 128 rows go as even chunks of at most 16 (above 64 rows: two halves first): 9, 14, 16, 11 and 16 rows."""
    for entry, feats in ENTRIES.items():
        if not feats[0]:
            for rows, first in ((17, 9), (40, 14), (64, 16), (65, 11), (128, 16)):
                assert "shape B=%d M=64 K=512 blocksize=32" % first in expected[entry]["%d rows, blocksize 32" % rows][1]
    ws = expected["fp4_hip_gemm_small_ws"]
    for rows, first in ((40, 14), (65, 11), (128, 16)):
        assert "shape B=%d M=64 K=512 blocksize=32" % first in ws["workspace: %d rows, blocksize 32" % rows][1]
    assert "shape B=16 M=64 K=512 blocksize=128" in ws["workspace: 127 rows, blocksize 128"][1]  # 64 + 63, then 4 x 16


def test_a_null_workspace_is_the_fused_entry_point(expected):
    fused, ws = expected["fp4_hip_gemm_small_fused"], expected["fp4_hip_gemm_small_ws"]
    for label, row in fused.items():
        assert ws[label] == [row[0], row[1].replace("fp4_hip_gemm_small_fused: unknown", "fp4_hip_gemm_small_ws: unknown")], label


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_refusal_has_its_status_and_its_whole_message(entry, expected):
    for label, kw in refusals(entry):
        rc = call(entry, **kw)
        assert [rc, hipabi.last_error()] == expected[entry][label], (entry, label)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_an_empty_problem_is_ok_whatever_the_pointers_are_and_leaves_the_message(entry, expected):
    for label, kw in empties(entry):
        assert _message_after(entry, kw) == (OK, ""), (entry, label)
    assert hipabi.last_error() == expected[entry]["negative M"][1]


def test_the_workspace_query_answers_zero_where_the_split_k_path_is_not_for_the_shape(expected):
    for label, kw in ws_bytes_cases():
        assert ws_bytes(**kw) == expected[WS_BYTES][label], label


@pytest.mark.parametrize("blocksize", [128, 32])
def test_a_workspace_with_another_blocksize_than_64_is_the_fused_entry_point(blocksize):
    """Not a record of the earlier library: there the split-K path sized and indexed a given workspace for blocksize 64 whatever the
    weight's was (33..64 rows, M below 24 per CU, K >= 8192) and answered FP4_OK with the wrong scales.  Now it turns the call down
    before it asks the device anything, and the call is fp4_hip_gemm_small_fused: three chunks of 11 rows that no kernel covers."""
    B, M, K = 33, 16, 8192
    kw = dict(B=B, M=M, K=K, blocksize=blocksize)
    assert call("fp4_hip_gemm_small_ws", workspace=D, workspace_bytes=B * M * 16 * 4, **kw) == UNSUPPORTED
    msg = hipabi.last_error()
    assert msg == ("fp4_hip_gemm_small: shape B=11 M=16 K=8192 blocksize=%d dtype=%d is not covered; use dequant + GEMM" % (blocksize, BF16))
    assert call("fp4_hip_gemm_small_fused", **kw) == UNSUPPORTED and hipabi.last_error() == msg
    assert ws_bytes(B=B, M=M, K=K, blocksize=blocksize) == 0


if __name__ == "__main__":
    print(json.dumps(table(), indent=1))
