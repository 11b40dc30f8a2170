"""Host-side proof of tests/fp4_constructed.py (no GPU): the closed form the GPU placement tests expect IS the oracle's product, its
one-hot cases stay where the bar's relative half-ulp term holds, what the kernels compute in f32 fits the bar with room to spare,
and the guard checker notices a write into either guard."""
import numpy as np
import pytest
import torch

import fp4_constructed as C
from oracle import fp4_oracle as o

SHAPES = [(257, 64, 64), (257, 512, 64), (33, 4096, 64), (257, 1472, 64), (9, 32768, 64), (37, 96, 32), (17, 8256, 64),
          # the VALU small-batch kernel's families at other block sizes (test_gpu_fp4_constructed.VALU_BLOCKSIZES, M = its M_PLACE)
          (257, 96, 32), (257, 256, 128), (257, 512, 256), (257, 4096, 4096)]
DT16 = ["bfloat16", "float16"]


@pytest.mark.parametrize("M,K,bs", SHAPES)
def test_closed_form_is_the_oracles_float64_product(M, K, bs):
    packed, am = C.byte_cycle_weight(M, K), C.placement_scales(M, K, bs)
    assert packed.size == M * K // 2 and am.size == M * K // bs
    nib = o.unpack_nibbles(packed).reshape(M, K)
    for B in (1, 5, 16):
        pos, val = C.one_hot_batches(K, B)
        assert sorted(set(pos.reshape(-1).tolist())) == C.one_hot_positions(K)  # every position is used
        assert (nib[np.arange(M)[None, :], pos.reshape(-1)[:, None]] == C.nibble(np.arange(M)[None, :], pos.reshape(-1)[:, None])).all()
        x = C.one_hot_rows(pos, val, K)
        want = np.stack([o.gemv_exact(row, packed, am, M, K, bs) for row in x.reshape(-1, K)]).reshape(pos.shape + (M,))
        got = C.closed_form(M, K, pos, val, bs)
        assert np.array_equal(got, want)  # bit for bit: the f32 product code * 2^n is exact


def test_the_weight_runs_through_every_byte_and_the_scales_differ_between_neighbours():
    M, K = 257, 512
    by = C.byte_cycle_weight(M, K).reshape(M, K // 2)
    for j in (0, 1, 31, 255):
        assert sorted(by[:256, j].tolist()) == list(range(256))
    am = C.placement_scales(M, K).reshape(M, K // 64)
    assert am.min() == 2.0**-3 and am.max() == 2.0**9
    assert (am[1:] != am[:-1]).all() and (am[:, 1:] != am[:, :-1]).all()
    assert C.one_hot_positions(4096)[:64] == list(range(64)) and {2047, 2048, 4031, 4032, 4094, 4095} <= set(C.one_hot_positions(4096))
    assert C.one_hot_positions(64) == list(range(64))


@pytest.mark.parametrize("K,bs", [(96, 32), (256, 128), (512, 256), (4096, 4096)])
def test_a_wrong_scale_index_shows_as_a_wrong_power_of_two(K, bs):
    """The runtime-blocksize families: every block of a row is reached by a one-hot position, and the scale an index off by one would
    read - the next block's, the next row's, the flat neighbour across a row end - is another power of two."""
    M = 257
    am = C.placement_scales(M, K, bs).reshape(M, K // bs)
    assert {k // bs for k in C.one_hot_positions(K)} == set(range(K // bs))
    assert (am[1:] != am[:-1]).all() and (am[:, 1:] != am[:, :-1]).all()
    flat = am.reshape(-1)
    assert (flat[1:] != flat[:-1]).all()
    assert (np.log2(am) == np.round(np.log2(am))).all()
    # a shift off by one (blocks twice or half as long) reads another scale wherever the index changes
    nb = K // bs
    if nb > 1:
        j = np.arange(nb)
        assert (am[:, j // 2] != am[:, j])[:, 1:].all()


@pytest.mark.parametrize("M,K,bs", SHAPES)
def test_one_hot_outputs_are_zero_or_normal_in_fp16(M, K, bs):
    """The bar's half-ulp term is relative, which holds for normal outputs only: every non-zero expectation is a normal fp16 number
    (and far from overflow), so one tolerance formula serves all three dtypes."""
    for B in (1, 7, 64):
        pos, val = C.one_hot_batches(K, B)
        e = np.abs(C.closed_form(M, K, pos, val, bs))
        nz = e[e != 0]
        assert nz.min() >= C.F16_MIN_NORMAL and nz.max() <= 3.0 * 2.0**9 < 65504
        assert (e == 0).any()  # nibbles 0 and 8 occur: the +-0 expectation is exercised


def test_f32_restatement_of_the_kernels_is_inside_the_bar():
    """((12 code * x) * absmax) * f32(1/12), rounded once: the distance to the closed form (CODE_PARAM's f32 literals differ from
    k / 12 by up to 1.1e-6 relative, f32(1/12) adds 6e-8) stays below the bar  1.01 ulp/2 + 1e-5 |exact|  on every one-hot case."""
    for dtype in DT16:
        worst = 0.0
        for M, K, bs in SHAPES:
            for B in (1, 16):
                pos, val = C.one_hot_batches(K, B)
                exact = C.closed_form(M, K, pos, val, bs)
                got = C.kernel_restatement(M, K, pos, val, dtype, bs)
                tol = C.bar(exact, np.abs(exact), dtype)
                worst = max(worst, float((np.abs(got - exact) / tol).max()))
                assert (got[exact == 0] == 0).all()
        print(f"f32 restatement, {dtype}: worst err/tol = {worst:.3f}")
        assert worst < 1.0, (dtype, worst)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.uint8])
def test_guard_checker_notices_a_write_into_either_guard(dtype):
    n, g = 37, C.guard_elems(5)
    assert g >= 4096 and g % 16 == 0 and C.guard_elems(5000) >= 10000
    buf, view = C.guarded(n, dtype, g, "cpu")
    assert buf.numel() == n + 2 * g and view.numel() == n and view.data_ptr() == buf.data_ptr() + g * buf.element_size()
    assert C.untouched(buf) and C.guards_intact(buf, n, g)
    view.zero_()  # the kernel's own output region: not a guard
    assert C.guards_intact(buf, n, g) and not C.untouched(buf)
    for where in (0, g - 1, g + n, n + 2 * g - 1):
        C.refill(buf)
        assert C.untouched(buf)
        buf[where] = 1
        assert not C.guards_intact(buf, n, g), where
    C.refill(buf)
    buf[g], buf[g + n - 1] = 1, 1  # first and last element of the view
    assert C.guards_intact(buf, n, g)
