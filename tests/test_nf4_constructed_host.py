"""Host-side proof of tests/nf4_constructed.py (no GPU): the closed form the GPU placement tests expect IS nf4_ref's product, the
byte cycle puts every byte value at every tested k, the one-hot outputs stay where the bar's relative half-ulp term holds, the f32
restatement of the batch-1 kernel fits the bar, the nested placement statistics expand exactly to what is claimed, and the adapter
matrices are exact in both 16-bit types."""
import numpy as np
import pytest
import torch

import nested_ref as N
import nf4_constructed as C
import nf4_ref as R

# the shapes of tests/test_gpu_nf4_constructed.py that are small enough to restate row by row, one per kind
SHAPES = [(257, 64, 64), (257, 512, 64), (33, 4096, 64), (9, 8224, 32), (37, 96, 32), (33, 250, 50), (200, 96, 32), (40, 1024, 64), (17, 576, 64)]
NESTED_SHAPES = [(200, 96, 32), (40, 1024, 64)]
DT16 = ["bfloat16", "float16"]


@pytest.mark.parametrize("M,K,bs", SHAPES)
def test_closed_form_is_nf4_refs_float64_product(M, K, bs):
    packed, am = C.byte_cycle_weight(M, K), C.placement_scales(M, K, bs)
    nib = R.unpack(packed, M * K).reshape(M, K)
    for B in (1, 5, 16):
        pos, val = C.one_hot_batches(K, B)
        assert sorted(set(pos.reshape(-1).tolist())) == C.one_hot_positions(K)
        assert (nib[np.arange(M)[None, :], pos.reshape(-1)[:, None]] == C.nibble(np.arange(M)[None, :], pos.reshape(-1)[:, None])).all()
        x = C.one_hot_rows(pos, val, K)
        want = np.stack([R.gemv_exact(row, packed, am, M, K, bs)[0] for row in x.reshape(-1, K)]).reshape(pos.shape + (M,))
        assert np.array_equal(C.closed_form_nf4(M, K, pos, val, bs), want)  # exactly: code * 2^n is an exact f32 product


def test_the_gemv_placement_cases_reach_every_cell_with_a_partial_last_pass():
    assert set(C.GEMV_PLACEMENT_CASES) <= set(R.GEMV_CELL_CASES)
    cells = [R.gemv_cell(M, K) for M, K in C.GEMV_PLACEMENT_CASES]
    assert len(set(cells)) == 12 == len(cells) and set(cells) == {R.gemv_cell(M, K) for M, K in R.GEMV_CELL_CASES}
    for (M, K), (ks, G, iters) in zip(C.GEMV_PLACEMENT_CASES, cells):
        assert (K // 32) % (G * 32 * ks) != 0, (M, K)  # dead lanes in the last pass
        other = [c for c in R.GEMV_CELL_CASES if R.gemv_cell(*c) == (ks, G, iters) and c != (M, K)]
        assert len(other) == 1
        if M % R.rows_per_workgroup(ks, iters) == 0:  # not the row-tail entry: only where that one is larger
            assert other[0][0] * other[0][1] > M * K and other[0][0] % R.rows_per_workgroup(ks, iters) != 0


def test_every_byte_value_occurs_at_every_tested_k_and_the_scales_differ_between_neighbours():
    M, K = 257, 2048
    by = C.byte_cycle_weight(M, K).reshape(M, K // 2)
    for k in C.one_hot_positions(K):
        assert sorted(by[:256, k // 2].tolist()) == list(range(256)), k
    for bs in (32, 64):
        am = C.placement_scales(M, K, bs).reshape(M, K // bs)
        assert am.min() == 2.0**-3 and am.max() == 2.0**9
        assert (am[1:] != am[:-1]).all() and (am[:, 1:] != am[:, :-1]).all()


@pytest.mark.parametrize("M,K,bs", SHAPES)
def test_one_hot_outputs_are_zero_or_normal_in_fp16(M, K, bs):
    smallest = float(np.float32(R.CODE_DECIMAL[8])) * 2.0**-3 * 0.75  # 0.0796 * 2^-3 * 0.75
    assert smallest >= C.F16_MIN_NORMAL
    for B in (1, 7, 64):
        pos, val = C.one_hot_batches(K, B)
        e = np.abs(C.closed_form_nf4(M, K, pos, val, bs))
        nz = e[e != 0]
        assert nz.min() >= smallest and nz.max() <= 3.0 * 2.0**9 < 65504
        assert (e == 0).any() or M < 16  # nibble 7 is NF4's only zero


def test_f32_restatement_is_one_rounding_away_and_inside_the_bar():
    for M, K, bs in SHAPES:
        pos, val = C.one_hot_batches(K, 1)
        exact = C.closed_form_nf4(M, K, pos, val, bs)
        f32 = C.gemv_f32_restatement(M, K, pos, val, bs).astype(np.float64)
        assert f32.dtype == np.float64 and (np.abs(f32 - exact) <= 2.0**-24 * np.abs(exact)).all()  # fl32(code * x), then exact
        assert (f32[exact == 0] == 0).all()
        for dtype in DT16 + ["float32"]:
            got = f32 if dtype == "float32" else torch.from_numpy(f32).float().to(getattr(torch, dtype)).double().numpy()
            assert (np.abs(got - exact) <= C.bar(exact, np.abs(exact), dtype)).all(), (M, K, dtype)


@pytest.mark.parametrize("offset", C.NESTED_OFFSETS)
@pytest.mark.parametrize("M,K,bs", NESTED_SHAPES)
def test_nested_statistics_expand_exactly_and_a_group_boundary_falls_inside_a_row(M, K, bs, offset):
    nb = M * K // bs
    q, nested, code, off = C.nested_statistics(nb, offset)
    assert q.dtype == np.uint8 and code.dtype == nested.dtype == np.float32 and len(set(code.tolist())) == 256
    frac, _ = np.frexp(code.astype(np.float64))
    assert (frac * 32 == np.round(frac * 32)).all() and code.min() == 2.0**-8 and code.max() == 31 / 16 * 2.0**7  # 5 bits each
    want = C.nested_expanded(nb, offset)
    for expand in (N.unnest, N.unnest_fma):  # exact, so one rounding or two give the same
        got = expand(q, nested, code, off, C.NESTED_GROUP)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    assert (want[1:] != want[:-1]).all()  # neighbouring blocks differ
    assert (want[C.NESTED_GROUP:] != want[:-C.NESTED_GROUP]).all()  # the same code under the next group's scale differs
    per_row = K // bs
    boundaries = [g for g in range(C.NESTED_GROUP, nb, C.NESTED_GROUP)]
    assert len(boundaries) >= 2
    if (M, K, bs) == (200, 96, 32):
        assert per_row == 3 and all(g % per_row for g in boundaries)  # 256 and 512 are no multiples of 3: both fall mid-row
    else:
        assert C.NESTED_GROUP % per_row == 0 and C.NESTED_GROUP // per_row == 16  # 16 rows per group
    # the one-hot outputs under these scales are normal fp16 numbers below fp16's largest
    pos, val = C.one_hot_batches(K, 1)
    e = np.abs(C.closed_form_nf4(M, K, pos, val, bs, absmax=want.astype(np.float32)))
    assert e[e != 0].min() >= C.F16_MIN_NORMAL and e.max() < 65504


def test_tabled_statistics_expand_bit_for_bit_including_zero_and_inf():
    a = np.random.default_rng(0).choice(np.array([0.0, np.inf, 2.0**-20, 0.013, 1024.0], np.float32), 700)
    q, nested, code, off = C.tabled_statistics(a)
    with np.errstate(invalid="ignore"):
        got = N.unnest(q, nested, code, off, C.NESTED_GROUP)
    assert np.array_equal(got.view(np.uint32), a.view(np.uint32))
    with pytest.raises(ValueError):
        C.tabled_statistics(np.arange(300, dtype=np.float32))


def test_adapter_matrices_are_exact_in_both_16_bit_types_and_differ_between_neighbours():
    b, a, s = C.lora_b(257, 256), C.lora_a(256, 8200), C.down_scale(256)
    for m in (a, b):
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(torch.from_numpy(m).to(dt).float(), torch.from_numpy(m))
        assert (m[1:] != m[:-1]).all() and (m[:, 1:] != m[:, :-1]).all() and np.abs(m).max() == 30 / 32
    assert set(np.abs(s).tolist()) == {1.0, 2.0, 4.0, 8.0} and (s < 0).any() and (s > 0).any()
    # one product of three small dyadic numbers: exact in f32 (and in bf16 for the B * t term: 30 * 3 needs 7 bits)
    assert float(np.abs(b).max() * 3.0) == 90 / 32
    for K in (8, 64, 4096, 8192, 8200):
        P = C.down_positions(K)
        assert {0, K - 8, K - 1} <= set(P) and all(0 <= k < K for k in P) and ({8191} <= set(P) or K < 8192) and ({8192} <= set(P) or K <= 8192)
        for rows in (1, 5, 64):
            pos, val = C.deal(P, rows)
            assert pos.shape == val.shape == (-(-len(P) // rows), rows) and set(pos.reshape(-1).tolist()) == set(P)


def test_builders_refuse_what_they_were_not_made_for():
    pos, val = np.array([0]), np.array([1.0])
    for bad in (lambda: C.closed_form_nf4(4, 96, pos, val, 64), lambda: C.closed_form_nf4(0, 64, pos, val), lambda: C.closed_form_nf4(4, 63, pos, val, 63),
                lambda: C.closed_form_nf4(4, 64, np.array([64]), val), lambda: C.closed_form_nf4(4, 64, pos, np.array([1.0, 2.0])),
                lambda: C.closed_form_nf4(4, 64, pos, val, absmax=np.ones(5, np.float32)), lambda: C.gemv_f32_restatement(4, 96, pos, val, 64),
                lambda: C.gemv_f32_restatement(4, 64, np.array([-1]), val), lambda: C.nested_statistics(0, 0.0), lambda: C.nested_statistics(10, 0.1),
                lambda: C.lora_b(4, 12), lambda: C.lora_b(0, 8), lambda: C.lora_a(264, 64), lambda: C.lora_a(8, 12), lambda: C.down_scale(4),
                lambda: C.down_positions(12), lambda: C.deal([], 4), lambda: C.deal([1], 0)):
        with pytest.raises(ValueError):
            bad()
