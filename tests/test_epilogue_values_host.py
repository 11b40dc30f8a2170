"""tests/epilogue_values.py against torch's CPU ops, at every 16-bit gate pattern (no GPU).

The gated chain over all 65536 gate patterns x U x R and the plain chains over E x E x R: every result of torch's own separate ops
(F.silu(g) * u + r; the rounded adds) must be a member of the reference set.  The number of gate patterns whose set has more than
one member is a condition: at most MULTI_MEMBER_CAP per dtype, so the set can never grow into a tolerance."""
import numpy as np
import pytest
import torch

import epilogue_values as V
from oracle import fp4_oracle as o

TORCH_DT = {V.BF16: torch.bfloat16, V.F16: torch.float16, V.F32: torch.float32}
MULTI_MEMBER_CAP = 16


def t_of(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(TORCH_DT[dtype])


def f32_of(t):
    return t.float().numpy()


@pytest.mark.parametrize("dtype", [V.BF16, V.F16])
def test_pattern_sets(dtype):
    E, U, R = V.edge_patterns(dtype), V.up_patterns(dtype), V.residual_patterns(dtype)
    n_exp = 1 << V.FORMAT[dtype]["exp_bits"]
    assert 8 * n_exp <= E.size <= 8 * n_exp + 40 and np.unique(E).size == E.size
    ev = V.values(E, dtype)
    for must in (0, 0x8000, 1, 0x8001, V.max_bits(dtype), V.max_bits(dtype) | 0x8000, V.inf_bits(dtype), V.inf_bits(dtype) | 0x8000):
        assert must in E
    assert np.isnan(ev).sum() >= 2
    lo, hi = V.neighbours(-V.E_OVERFLOW, dtype)
    assert lo in E and hi in E and np.isinf(V.exp_neg(V.values([lo], dtype)))[0] and np.isfinite(V.exp_neg(V.values([hi], dtype)))[0]
    for edge in V.D_IS_ONE:
        lo, hi = V.neighbours(edge, dtype)
        assert lo in E and hi in E and hi == lo + 1
    assert U.size == 13 and np.unique(U).size == 13 and R.size == 4
    uv = V.values(U, dtype)
    assert np.isnan(uv).sum() == 1 and np.isinf(uv).sum() == 2 and (uv == 0).sum() == 2
    sub = uv[5]
    assert sub < 0 and abs(sub) < V.values([1 << V.FORMAT[dtype]["man_bits"]], dtype)[0]
    assert set(V.bias_subset(dtype)) <= set(E) and np.unique(V.bias_subset(dtype)).size == 16
    assert np.array_equal(V.rt(V.activation_scales(dtype), dtype), V.activation_scales(dtype))  # activations are T values
    s = V.rt(V.sum_row_scales(dtype), dtype)  # the classes the off-grid scales stand for
    one, u, mx = np.float32(1.0), np.float32(V.ulp_of_one(dtype)), V.values([V.max_bits(dtype)], dtype)[0]
    assert s[0] == one and s[1] == one + 2 * u and s[2] == mx and np.isinf(s[3]) and s[4] == 0
    assert np.signbit(V.rt(-V.sum_row_scales(dtype)[4:], dtype))[0]


@pytest.mark.parametrize("dtype", [V.BF16, V.F16])
def test_roundings_and_the_oracles_own_epilogues_agree(dtype):
    """rt is the oracle's rounding on f32 input, non-finite classes included, and the oracle's epilogues are members of the sets."""
    allv = V.values(np.arange(0x10000, dtype=np.uint32).astype(np.uint16), dtype)
    assert np.array_equal(V.to_bits(allv, dtype)[~np.isnan(allv)], np.arange(0x10000, dtype=np.uint32).astype(np.uint16)[~np.isnan(allv)])
    rng = np.random.default_rng(0)
    raw = rng.integers(0, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        probes = np.concatenate([raw, allv, allv * np.float32(1 + 2.0**-9), np.array([np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, 65520.0, 65519.9], np.float32)])
        assert V.same(V.rt(probes, dtype), o.round_to(dtype)(probes)).all()
    assert V.same(V.rt(probes, dtype), f32_of(torch.from_numpy(probes).to(TORCH_DT[dtype]))).all()
    fin = allv[np.isfinite(allv)][::7]
    u = V.values(V.up_patterns(dtype), dtype)[[2, 3, 11, 12]]
    with np.errstate(over="ignore", invalid="ignore"):
        theirs = o.silu_mul_epilogue(fin[:, None], u[None, :], dtype, residual=np.float32(1.0))
        assert V.agrees(theirs, V.gated(fin[:, None], u[None, :], dtype, np.float32(1.0))).all()
        assert V.same(o.linear_epilogue(fin[:, None], dtype, u[None, :], u[None, ::-1]), V.plain_batch1(fin[:, None], dtype, u[None, :], u[None, ::-1])).all()


def test_formula_at_the_edges():
    q = lambda g: V.formula(np.float32(g), V.exp_neg(np.float32(g)))  # noqa: E731
    assert np.isnan(q(-np.inf)) and np.isnan(q(np.nan)) and q(np.inf) == np.inf
    assert q(-89.0) == 0 and np.signbit(q(-89.0)) and q(-88.5) < 0  # e overflows: -0 where true silu is about -3e-37
    assert q(0.0) == 0 and not np.signbit(q(0.0)) and np.signbit(q(-0.0))
    assert q(17.5) == np.float32(17.5) and q(16.75) == np.float32(16.75) and q(16.5) < np.float32(16.5)  # d = 1 from 16.64 on
    tiny = np.float32(2.0**-140)
    assert q(tiny) == tiny / 2 and q(-tiny) == -tiny / 2  # f32 subnormal gates (bf16 subnormals) keep their value
    es = V.exp_set(np.array([-89.0, 0.0, np.nan], np.float32))
    assert np.isinf(es[:, 0]).all() and np.isnan(es[:, 2]).all() and es[1, 1] < es[0, 1] < es[2, 1]


@pytest.mark.parametrize("dtype", [V.BF16, V.F16])
def test_gated_chain_every_gate_pattern_against_torch_cpu(dtype):
    gates = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    U, R = V.up_patterns(dtype), V.residual_patterns(dtype)
    gv, uv, rv = V.values(gates, dtype), V.values(U, dtype), V.values(R, dtype)
    multi = V.multi_member(V.silu_set(gv, dtype))
    print(f"epilogue-values-host | gated | {dtype} | gate patterns with a multi-member silu set: {int(multi.sum())} (cap {MULTI_MEMBER_CAP})"
          f" {[hex(int(b)) for b in gates[multi]]}")
    assert int(multi.sum()) <= MULTI_MEMBER_CAP
    s_t = torch.nn.functional.silu(t_of(gates, dtype))
    assert V.agrees(f32_of(s_t), V.silu_set(gv, dtype)).all()
    prod_t = s_t[:, None] * t_of(U, dtype)[None, :]
    checked = outside = 0
    for r_t, r in [(None, None)] + [(t_of(R[i:i + 1], dtype), rv[i]) for i in range(R.size)]:
        theirs = f32_of(prod_t if r_t is None else prod_t + r_t)
        ok = V.agrees(theirs, V.gated(gv[:, None], uv[None, :], dtype, r))
        checked, outside = checked + ok.size, outside + int((~ok).sum())
        assert ok.all(), (dtype, r, [hex(int(b)) for b in gates[~ok.all(axis=1)][:8]])
    print(f"epilogue-values-host | gated | {dtype} | {checked} chain results, {outside} outside the set")
    assert checked == 65536 * 13 * 5
    # the final results differ between members at no more gate patterns than the silu does
    full = V.multi_member(V.gated(gv[:, None], uv[None, :], dtype)).any(axis=1)
    assert not (full & ~multi).any()


@pytest.mark.parametrize("dtype", [V.BF16, V.F16, V.F32])
def test_plain_chains_against_torch_cpu_adds(dtype):
    T = TORCH_DT[dtype]
    src = V.BF16 if dtype == V.F32 else dtype
    E = V.edge_patterns(src)
    ev = V.values(E, src)
    sub = V.values(V.bias_subset(src), src)
    rs = [None] + list(V.values(V.residual_prime_patterns(src), src))
    to_t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(T)  # noqa: E731  (exact: the values are T values)
    # f32 sums off the T grid: each pattern, and each pattern moved by half and by a quarter of an ulp of T (ties, near-ties)
    with np.errstate(over="ignore", invalid="ignore"):
        sums = np.concatenate([ev, ev * np.float32(1 + V.ulp_of_one(src) / 2), ev * np.float32(1 - V.ulp_of_one(src) / 4)]).astype(np.float32)
    checked = outside = 0
    for total, bias in ((sums[:, None], sub[None, :]), (np.concatenate([sub, V.sum_row_scales(src)])[:, None], ev[None, :])):
        total, bias = np.broadcast_arrays(total, bias)
        for r in rs:
            t1 = torch.from_numpy(total.copy()).to(T)
            t1 = t1 + to_t(bias)
            tb = (torch.from_numpy(total.copy()) + torch.from_numpy(bias.copy())).to(T)
            if r is not None:
                t1, tb = t1 + to_t(np.float32(r)), tb + to_t(np.float32(r))
            ok1, okb = V.same(f32_of(t1), V.plain_batch1(total, dtype, bias, r)), V.same(f32_of(tb), V.plain_batch(total, dtype, bias, r))
            outside += int((~ok1).sum()) + int((~okb).sum())
            assert ok1.all(), (dtype, "batch-1", r)
            assert okb.all(), (dtype, "batch", r)
            checked += 2 * total.size
    no_bias = torch.from_numpy(sums).to(T)
    assert V.same(f32_of(no_bias), V.plain_batch(sums, dtype)).all() and V.same(f32_of(no_bias), V.plain_batch1(sums, dtype)).all()
    print(f"epilogue-values-host | plain | {dtype} | {checked} chain results, {outside} outside")
