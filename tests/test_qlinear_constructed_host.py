"""Host-side proof of tests/qlinear_constructed.py (no GPU): the reference arithmetic of the batch > 1 path - a dense linear over the
dequantised weight, here torch's on the CPU over the ORACLE's dequant - meets every exact expectation the GPU tests hold the
`qlinear*` ops to, in f32, fp16 and bf16; the constructions have the properties they claim (every byte value at a fixed k, scales that
differ between neighbours, a bias that needs every bit of T, partial sums below 256); and ``routed`` tells the routes apart."""
import numpy as np
import pytest
import torch

import nested_ref as N
import qlinear_constructed as Q
from gpu_util import bits as tbits

TD = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
_W = {}


def _t(values, dtype):
    """float64 T values -> CPU tensor of T (exact: Q.bits has shown them representable wherever it matters)."""
    return torch.from_numpy(np.ascontiguousarray(values, np.float64)).to(TD[dtype])


def _canon(t):
    return torch.where(t == 0, torch.zeros_like(t), t)


def _weight(kind, M, K, fmt, dtype):
    key = (kind, M, K, fmt, dtype)
    if key not in _W:
        packed, am = {"cycle": lambda: (Q.byte_cycle_weight(M, K), Q.flat_scales(M, K)), "zero": lambda: Q.zero_code_weight(M, K, fmt),
                      "sums": lambda: Q.exact_sum_weight(M, K, fmt)}[kind]()
        _W[key] = Q.weight_T(packed, am, M, K, fmt, dtype)
    return _W[key]


@pytest.mark.parametrize("dtype", Q.DTYPES)
@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("M,K", Q.WEIGHT_SHAPES)
def test_one_hot_expectation_is_what_a_dense_linear_over_the_oracle_weight_returns(M, K, fmt, dtype):
    w = _weight("cycle", M, K, fmt, dtype)
    Q.bits(w, dtype)  # the oracle's weight consists of T values
    pos, val = Q.one_hot_batches(K, 7)
    assert sorted(set(pos.reshape(-1).tolist())) == Q.one_hot_positions(K)
    x = Q.one_hot_rows(pos, val, K).reshape(-1, K)
    want = Q.one_hot_expected(w, pos, val, dtype)
    assert want.shape == (x.shape[0], M) and (want != 0).any()
    got = torch.nn.functional.linear(_t(x, dtype), _t(w, dtype))
    assert np.array_equal(tbits(_canon(got)), Q.bits(want, dtype))
    # one product per output: exact in float64, and T(fl32(.)) of it is at most two roundings away
    exact = w[:, pos.reshape(-1)].T * val.reshape(-1, 1)
    half = {"float32": 2.0**-24, "float16": 2.0**-11, "bfloat16": 2.0**-8}[dtype]
    assert (np.abs(want - exact) <= (half + 2.0**-24) * np.abs(exact)).all()
    if dtype == "float16":  # no one-hot output is subnormal or overflows in fp16
        nz = np.abs(want[want != 0])
        assert nz.min() >= 2.0**-14 and nz.max() < 65504


@pytest.mark.parametrize("M,K", Q.WEIGHT_SHAPES + [(16, 64)])
def test_scales_differ_between_neighbouring_blocks_and_rows(M, K):
    block_of = np.arange(M * K, dtype=np.int64).reshape(M, K) // Q.BS
    am = Q.flat_scales(M, K)
    assert am.size == Q.n_blocks(M, K) and am.min() >= 2.0**-3 and am.max() <= 2.0**9
    s = am[block_of]
    assert (am[1:] != am[:-1]).all() and (s[1:] != s[:-1]).all()
    es = Q.exact_sum_scales(M, K)
    assert es.size == Q.n_blocks(M, K) and set(es.tolist()) == {1.0, 2.0, 4.0} and (es[1:] != es[:-1]).all()
    s = es[block_of]
    if K % Q.BS == 0:
        assert (s[1:] != s[:-1]).all()
    else:  # blocks straddle rows: three values cannot differ at every distance (see exact_sum_scales); they do at the distance d + 1
        d = K // Q.BS
        assert d % 3 == 0 and ((block_of[1:] - block_of[:-1] == d + 1) == (s[1:] != s[:-1])).all()
        assert (s[1:] != s[:-1]).mean() > 0.5


def test_the_byte_cycle_shows_every_byte_value_at_every_tested_k():
    M, K = Q.WEIGHT_SHAPES[0]
    by = Q.byte_cycle_weight(M, K).reshape(M, K // 2)
    for k in Q.one_hot_positions(K):
        assert sorted(by[:256, k // 2].tolist()) == list(range(256)), k
    assert (300 * 1000) % Q.BS != 0 and 1000 % Q.BS != 0 and 1000 % 16 != 0 and 300 % 16 != 0  # the straddling shape straddles


@pytest.mark.parametrize("dtype", Q.DTYPES)
def test_the_bias_needs_every_bit_of_its_type_and_differs_between_all_columns(dtype):
    b = Q.full_precision_bias(448, dtype)
    Q.bits(b, dtype)  # representable
    assert len(set(b.tolist())) == 448 and (b > 0).any() and (b < 0).any() and (b != 0).all()
    frac, _ = np.frexp(b)
    p = Q.SIGNIFICAND_BITS[dtype]
    scaled = np.abs(frac) * 2.0**p
    assert (scaled == np.round(scaled)).all() and (scaled % 2 == 1).all()  # p significant bits, the last one set
    if dtype == "float32":
        for narrow in ("float16", "bfloat16"):
            assert (Q.round_T(b.astype(np.float32), narrow) != b).all()
    elif dtype == "float16":
        assert (Q.round_T(b.astype(np.float32), "bfloat16") != b).all()


@pytest.mark.parametrize("dtype", Q.DTYPES)
@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("M,K", Q.WEIGHT_SHAPES)
def test_over_the_zero_code_weight_a_dense_linear_returns_the_bias_bits(M, K, fmt, dtype):
    w = _weight("zero", M, K, fmt, dtype)
    assert (w == 0).all() and not np.signbit(w).any()
    bias = Q.full_precision_bias(M, dtype)
    x = Q.arbitrary_rows((5, K), dtype, seed=M)
    assert np.isfinite(x).all() and (x > 0).any() and (x < 0).any() and np.abs(x).max() > 4 and np.abs(x[x != 0]).min() < 2.0**-4
    got = torch.nn.functional.linear(_t(x, dtype), _t(w, dtype), _t(bias, dtype))
    assert np.array_equal(tbits(got), np.broadcast_to(Q.bits(bias, dtype), (5, M)))


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("M,K", Q.WEIGHT_SHAPES + [(16, 64)])
def test_exact_sums_are_exact_in_every_type_and_order(M, K, fmt):
    packed, am = Q.exact_sum_weight(M, K, fmt)
    nz_code = packed.reshape(M, K // 2)
    pos = Q.exact_sum_positions(M, K)
    assert all(len(set(row.tolist())) == Q.TERMS for row in pos)
    assert pos.min(axis=1).max() < K // 4 or K < 256  # spread over the row: every row starts in its first quarter ...
    assert pos.max(axis=1).min() >= 3 * K // 4 or K < 256  # ... and reaches its last
    z = Q.ZERO_CODE[fmt]
    assert ((nz_code != ((z << 4) | z)).sum(axis=1) <= Q.TERMS).all()
    x = Q.exact_sum_rows((9, K))
    bias = Q.exact_sum_bias(M)
    assert set(np.unique(x).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and bias.min() >= -32 and bias.max() <= 32 and (M < 65 or (bias.min(), bias.max()) == (-32, 32))
    want = None
    perm = np.random.default_rng(K).permutation(K)
    for dtype in Q.DTYPES:
        w = _weight("sums", M, K, fmt, dtype)
        assert ((w != 0).sum(axis=1) == Q.TERMS).all() and set(np.unique(np.abs(w)).tolist()) == {0.0, 1.0, 2.0, 4.0}
        signs = np.sign(w[np.arange(M)[:, None], pos])
        assert (signs[:, 1:] != signs[:, :-1]).all() and (signs[1:] != signs[:-1]).all()  # signs differ between neighbours
        # 1. the bound: non-zeros x largest |w| x largest |x| + largest |bias| < 256
        assert Q.exact_sum_bound(w, x, bias) <= 224 < 256
        # 2. the float64 expectation survives a round trip through T (and is the same for every T: the weight values are)
        for b in (None, bias):
            y = Q.product(w, x, b)
            assert (y == np.round(y)).all() and np.abs(y).max() <= 224
            Q.bits(y, dtype)
        y, yb = Q.product(w, x), Q.product(w, x, bias)
        want = (y, yb) if want is None else want
        assert np.array_equal(want[0], y) and np.array_equal(want[1], yb) and np.abs(y).max() > 8
        # 3. a dense linear on the CPU returns those bits, also with the K axis permuted
        for xs, ws in ((x, w), (x[:, perm], w[:, perm])):
            got = torch.nn.functional.linear(_t(xs, dtype), _t(ws, dtype))
            assert np.array_equal(tbits(_canon(got)), Q.bits(y, dtype))
            got = torch.nn.functional.linear(_t(xs, dtype), _t(ws, dtype), _t(bias, dtype))
            assert np.array_equal(tbits(_canon(got)), Q.bits(yb, dtype))


@pytest.mark.parametrize("M,K", Q.NESTED_SHAPES)
def test_the_constructed_scales_fit_a_nested_table_that_expands_to_the_same_bits(M, K):
    for am in (Q.flat_scales(M, K), Q.exact_sum_scales(M, K)):
        q, nested, code, off = Q.tabled_statistics(am)
        got = N.unnest(q, nested, code, off, 256)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), am.view(np.uint32))


def test_row_shapes_cross_the_fused_kernels_thresholds():
    rows = [int(np.prod(s[:-1])) if len(s) > 1 else 1 for s in Q.row_shapes(192)]
    assert rows == [2, 5, 65, 129, 300, 1] and [len(s) for s in Q.row_shapes(192)] == [2, 3, 2, 2, 3, 1]


def test_builders_and_bits_refuse_what_they_were_not_made_for():
    for bad in (lambda: Q.flat_scales(0, 64), lambda: Q.zero_code_weight(3, 3, "nf4"), lambda: Q.exact_sum_weight(4, 16, "tree"),
                lambda: Q.full_precision_bias(449, "float32"), lambda: Q.bits(np.array([1.0 + 2.0**-9]), "bfloat16"),
                lambda: Q.bits(np.array([0.1]), "float32"), lambda: Q.weight_T(np.zeros(2, np.uint8), np.ones(1, np.float32), 1, 4, "int4", "float32"),
                lambda: Q.one_hot_expected(np.zeros((2, 4)), np.array([4]), np.array([1.0]), "float32"),
                lambda: Q.one_hot_expected(np.zeros((2, 4)), np.array([1]), np.array([0.1]), "float32"), lambda: Q.round_T(np.zeros(1), "int8")):
        with pytest.raises(ValueError):
            bad()
    assert np.array_equal(Q.bits(np.array([-0.0, 0.0, -1.0]), "float16"), np.array([0, 0, 0xBC00], np.uint16))


class _Counters:
    def __init__(self):
        self.n = {"direct": 0, "aten": 0}

    def qlinear_gemm_stats(self):
        return dict(self.n)


def test_routed_tells_the_routes_apart():
    ext = _Counters()
    with Q.routed(ext, "direct", calls=2):
        ext.n["direct"] += 2
    with Q.routed(ext, "aten"):
        ext.n["aten"] += 1
    for route, bump, calls in (("direct", "aten", None), ("aten", "direct", None), ("direct", None, None), ("direct", "direct", 2)):
        with pytest.raises(AssertionError):
            with Q.routed(ext, route, calls=calls):
                if bump:
                    ext.n[bump] += 1
    with pytest.raises(ValueError):
        with Q.routed(ext, "hipblaslt"):
            pass
