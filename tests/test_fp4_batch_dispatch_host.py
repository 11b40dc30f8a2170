"""Host-side checks of tests/fp4_batch_cases.py (no GPU): the restated dispatcher of fp4_hip_gemm_small / _fused / _ws against the
text of the three kernel files, the reach of the cases tests/test_gpu_fp4_batch_dispatch.py runs, and the forcing settings."""
import itertools
import os

import pytest

import fp4_batch_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "torch-bnb-fp4_amd", "csrc")
CUS = 256  # compute units of an MI355X: the reach is proven for the whole card


def _cells_of_cases(cus):
    seen = {}
    for B, M, K, ws in C.CASES(cus):
        for c in C.cells(B, M, K, cus, ws):
            seen.setdefault(C.reach_key(c), (B, M, K, ws))
    return seen


def test_the_restatement_returns_exactly_the_listed_cells():
    """The restated dispatcher over a grid - every row count, the rows around every threshold and between them, every class of
    K / 512 and the ragged K - returns the cells of all_cells() and no other: the list the reach is measured against is complete."""
    ms = set()
    for t in (2048, 4096, 8192, 16384, 8 * CUS, 16 * CUS, 20 * CUS, 24 * CUS, 48 * CUS, 96 * CUS):
        ms |= {t - 1, t, t + 1}
    ms |= {1, 15, 16, 17, 300, 3000, 7000, 10000, 14336, 20000, 28672, 40000}
    ks = [64, 512, 576, 1024, 1536, 2048, 2560, 4096, 5120, 8192, 11008, 12288, 13824, 14336, 16384]
    seen = set()
    for B, M, K, ws in itertools.product(range(1, 129), sorted(ms), ks, (False, True)):
        for c in C.cells(B, M, K, CUS, ws):
            assert c is not None, (B, M, K, ws)
            seen.add(C.reach_key(c))
    assert seen == C.all_cells(), (sorted(seen - C.all_cells()), sorted(C.all_cells() - seen))


def test_cases_reach_every_dispatch_cell():
    seen = _cells_of_cases(CUS)
    assert set(seen) == C.all_cells(), (sorted(C.all_cells() - set(seen)), sorted(set(seen) - C.all_cells()))
    # the chunked calls: 100 rows are two one-pass launches of 50; with the one-pass path declined 17..64 rows go in 16-row launches
    assert C.chunks(100, 64) == [50, 50] and C.chunks(65, 64) == [33, 32] and C.chunks(128, 64) == [64, 64]
    assert C.chunks(17, 16) == [9, 8] and C.chunks(33, 16) == [11, 11, 11] and C.chunks(64, 16) == [16] * 4
    assert C.cells(100, 48 * CUS, 4096, CUS) == [("wide", 4, 3)] * 2
    off = C.hooks(gemm_wide=0)
    assert C.cells(32, 14336, 4096, CUS, h=off) == [("persist", 0)] * 2 and C.cells(64, 14336, 4096, CUS, h=off) == [("persist", 0)] * 4
    assert C.cells(17, 4096, 4096, CUS, h=off) == [("mfma", 1, 4, 0), ("mfma", 1, 4, 8)]
    assert C.cells(100, 24 * CUS - 1, 8192, CUS, True) == [("splitk", 4, 3)] * 2
    # the shapes the decode bench times are among the cases, at every row count it times
    for M in (14336, 28672):
        assert {B for B, m, K, ws in C.CASES(CUS) if (m, K, ws) == (M, 4096, False)} >= {2, 8, 16, 32, 64}
    # T - 1 is never a multiple of 16: the lower side of every threshold has a ragged last tile
    assert all(C.rows_of(t.lo, CUS) % 16 or C.rows_of(t.hi, CUS) % 16 for t in C.THRESHOLDS)
    # the largest weight is 96 MiB packed
    assert max(M * K // 2 for _, M, K, _ in C.CASES(CUS)) == 96 << 20


@pytest.mark.parametrize("t", C.THRESHOLDS, ids=[t.name for t in C.THRESHOLDS])
def test_both_sides_of_every_threshold_land_in_different_cells(t):
    ws = t is C.WS_THRESHOLD
    for B in t.Bs:
        lo = C.cells(B, C.rows_of(t.lo, CUS), t.K, CUS, ws)
        hi = C.cells(B, C.rows_of(t.hi, CUS), t.K, CUS, ws)
        assert len(lo) == len(hi) == 1 and lo != hi, (t.name, B, lo, hi)
        # a pair is exempt from the route test exactly where the two kernels share one K partition and summation order
        assert (C.exempt(lo[0], hi[0]) is not None) == (C.k_partition(lo[0]) == C.k_partition(hi[0])), (t.name, B, lo, hi)


def test_the_exempt_list_names_no_pair_whose_k_slicing_differs():
    cells = sorted(C.all_cells(), key=str)
    for a, b in itertools.combinations(cells, 2):
        if C.exempt(a, b) is not None:
            assert C.k_partition(a) == C.k_partition(b), (a, b)
    # what is exempt among the thresholds, and what the route test can tell apart
    exempt = {t.name for t in C.THRESHOLDS
              if all(C.exempt(C.cell(B, C.rows_of(t.lo, CUS), t.K, CUS, t is C.WS_THRESHOLD),
                              C.cell(B, C.rows_of(t.hi, CUS), t.K, CUS, t is C.WS_THRESHOLD)) for B in t.Bs)}
    assert exempt == {"rowt: B > 4 && M >= 32 * 256", "xs8: blocks <= cus", "wide, B <= 16: M >= 48 * cus (units = 2)",
                      "wide, B <= 16: M >= 48 * cus (odd units)", "wide, B > 16: M >= 48 * cus (K = 576)",
                      "wide, B > 16: M >= 96 * cus (K = 576)", "wide, B > 16: M >= 48 * cus (K = 4096)",
                      "wide, B > 16: M >= 96 * cus (K = 4096)"}
    # the kernels behind the list: one K split in the ring kernel whatever its row tiles, two numbers for one kernel
    wide = open(os.path.join(CSRC, "gemm_wide_fp4.hip")).read()
    assert "constexpr int WR = 2, WK = 4, kTiles = WR * RT, kRows = 16 * kTiles;" in wide
    assert wide.count("if (cfg == 5 || cfg == 1) return") == 2
    small = open(os.path.join(CSRC, "gemm_small_fp4.hip")).read()
    assert "const int b0 = (pass * 8 + wave) * NBW;" in small and "for (int w = 0; w < 8; ++w) t += s_part[w][rt][e];" in small
    assert "bfrag[t] = pair_up8(xr[j][t]);" in small


def test_the_kernel_sources_state_the_restated_rules():
    """An edit of a heuristic has to be made here too."""
    small = open(os.path.join(CSRC, "gemm_small_fp4.hip")).read()
    for text in ["const bool short_few = M <= 2048 && B <= 2 && K <= 4096;",
                 "const bool want_mfma = v_small == 1 || (v_small < 0 && !short_few);",
                 "if ((units & 1) || ((units % 4) != 0 && (B >= 5 || M >= 48 * cus)) || (M >= 96 * cus && K >= 8192 && B >= 5) ||",
                 "(B >= 13 && K >= 12288 && M <= 16 * cus))",
                 "if (rc == -1 && mfma_ok && v_small < 0 && !short_few) {",
                 "if (rc == -1 && mfma_ok && (want_mfma || B > 8)) rc = mfma();",
                 "if (rc == -1 && ok && B <= 8 && K <= 16384) rc =",
                 "const int rowt = v_rowt > 0 ? v_rowt : ((B > 4 && M >= 32 * 256) ? 2 : 1);",
                 "const bool persist_auto = B <= 4 ? M >= 16384 : M > 4096;",
                 "if (v_persist != 0 && v_rowt <= 0 && v_xstage != 0 && K == 4096 && (v_persist == 1 || persist_auto)) {",
                 "const bool xs4 = v_xstage != 0 && B <= 4;",
                 "const bool xs8 = v_xstage != 0 && !xs4 && B <= 8 && (int)blocks <= device_cu_count();",
                 "if (units % 4 == 0) FP4_MF(4);", "if (units % 2 == 0) FP4_MF(2);",
                 "const auto kern = B <= 4 ? gemm16_mfma_persist_kernel<DT, 4> : (B <= 8 ? gemm16_mfma_persist_kernel<DT, 8> : "
                 "gemm16_mfma_persist_kernel<DT, 0>);",
                 "return for_row_chunks(c, B > 64 ? 64 : 16, gemm_small_entry);",
                 "return for_row_chunks(c, 64, gemm_small_ws_entry);",
                 "c.B >= 33 && c.B <= 64 && c.M > 0",
                 "if (B > 64 && B <= 128) B = (B + 1) / 2;",
                 "} else if (C <= 256 && nb <= 4) {", "} else if (C <= 512 && nb <= 2) {",
                 # the sweep hooks
                 "g_small_variant = v < 0 ? -1 : (v & 1);", "const int rowt = v < 0 ? 0 : ((v >> 4) & 3);",
                 "g_mfma_xstage = v < 0 ? -1 : ((v >> 9) & 1 ? 0 : 1);", "g_small_wide = v < 0 ? 0 : ((v >> 12) & 1);",
                 "g_mfma_persist = v < 0 ? -1 : ((v >> 10) & 3) == 1 ? 0 : (((v >> 10) & 3) == 2 ? 1 : -1);"]:
        assert text in small, text
    wide = open(os.path.join(CSRC, "gemm_wide_fp4.hip")).read()
    for text in ["cfg = M >= 48 * cus ? 3 : (M >= 20 * cus ? 2 : 1);",
                 "cfg = M >= 96 * cus ? 4 : (M >= 48 * cus ? 3 : (M >= 24 * cus ? 2 : 1));",
                 "if (cfg == 1 && B <= 32) cfg = 5;",
                 "if (cfg == 0 || B < 1 || (B <= 16 && !any_rows) || B > 64 || (K % 64) != 0 || M < 1) return -1;",
                 "if (cfg == 3 || NT == 1) return launch_gemm16(gemm16_wide_ring_kernel<DT, NT, 2>",
                 "void set_wide_variant(int v) { g_wide_cfg = v < 0 ? -1 : (v > 5 ? 5 : v); }"]:
        assert text in wide, text
    splitk = open(os.path.join(CSRC, "gemm_splitk_fp4.hip")).read()
    for text in ["if (B < 33 || B > 64 || blocksize != 64 || (K % 64) != 0 || K < 8192 ||",
                 "if (M < 16 || M >= 24 * int64_t(device_cu_count())) return 0;",
                 "const int64_t slices = (K / 64 + 7) / 8;", "return slices * B * M * 4;",
                 "const int64_t tiles = (int64_t)((M + 15) / 16) * slices, waves = 8 * int64_t(device_cu_count());",
                 "int tpw = (int)((tiles + waves - 1) / waves);", "const int rows_per_wg = 128 * tpw;"]:
        assert text in splitk, text
    call = open(os.path.join(CSRC, "fp4_call.h")).read()
    assert "const int64_t chunks = (c.B + unit - 1) / unit, per = (c.B + chunks - 1) / chunks;" in call


def test_forced_settings_round_trip_through_the_restated_hooks():
    """forced(cell) decoded by the restated set_small_variant / set_wide_variant and fed to the restated dispatcher gives the cell
    back: for the default cell of every launch of every case, and for every cell legal_cells() lists on those shapes."""
    assert C.set_small_variant(-1) == (-1, -1, -1, 0, -1) and C.set_wide_variant(-1) == -1 and C.set_wide_variant(9) == 5
    assert C.set_small_variant(0) == (0, -1, 1, 0, -1)
    assert C.set_small_variant(1 | (2 << 4)) == (1, 2, 1, 0, -1)
    assert C.set_small_variant(1 | (1 << 4) | (1 << 9)) == (1, 1, 0, 0, -1)
    assert C.set_small_variant(1 | (2 << 10)) == (1, -1, 1, 0, 1) and C.set_small_variant(1 | (1 << 10)) == (1, -1, 1, 0, 0)
    assert C.set_small_variant(1 << 12) == (0, -1, 1, 1, -1)
    assert C.forced(("valu",), 2) == {"gemm_small": 0} and C.forced(("mfma", 2, 4, 0), 16) == {"gemm_small": 1 | (2 << 4)}
    assert C.forced(("persist", 8), 5) == {"gemm_small": 1 | (2 << 10)}
    assert C.forced(("wide", 1, 3), 5) == {"gemm_small": 1 << 12, "gemm_wide": 3} and C.forced(("wide", 3, 4), 33) == {"gemm_wide": 4}
    with pytest.raises(ValueError):
        C.forced(("splitk", 3, 1), 33)
    n = 0
    for B, M, K, ws in C.CASES(CUS):
        for rows in (C.chunks(B, 64) if B > 64 else [B]):
            default = C.cell(rows, M, K, CUS, ws)
            legal = C.legal_cells(rows, M, K, CUS)
            if default[0] != "splitk":
                assert default in legal, (rows, M, K, default, legal)
            elif not ws:
                pytest.fail("split-K without a workspace")
            for c in legal:
                assert C.cell(rows, M, K, CUS, h=C.hooks_of(C.forced(c, rows))) == c, (rows, M, K, c)
                n += 1
    assert n > 300
    # every form of every family is forced on a tall grid (more than one resident round: M > 16 * cus) somewhere among the cases
    tall = {c for B, M, K, ws in C.CASES(CUS) if M > 16 * CUS and B <= 64 for c in C.legal_cells(B, M, K, CUS)}
    assert tall >= {("valu",), ("persist", 4), ("persist", 8), ("persist", 0)}
    assert tall >= {("mfma", rowt, 4, 0) for rowt in (1, 2)} | {("mfma", 1, 4, 4), ("mfma", 1, 2, 0), ("mfma", 2, 2, 0), ("mfma", 1, 1, 0)}
    assert tall >= {("wide", 1, cfg) for cfg in (5, 2, 3)} | {("wide", 2, cfg) for cfg in (5, 2, 3, 4)}
    assert tall >= {("wide", nt, cfg) for nt in (3, 4) for cfg in (1, 2, 3, 4)}
