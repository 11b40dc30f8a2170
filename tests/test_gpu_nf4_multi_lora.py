"""Several LoRA adapters in one batch, selected per activation row on the device: fp4_hip_lora_down_multi,
fp4_hip_gemm_lora_multi_nf4, fp4_hip_gemv_lora_multi_nf4 through the C ABI, the torch ops, MultiLoRANF4Linear and
attach_lora_adapters / load_lora_adapters.

The kernel tests need no tolerance: a row with adapter a must carry the BITS of the single-adapter entry point called with slice a
(tests/test_gpu_nf4_lora.py pins those to the float64 oracle), a row without an adapter the bits of the plain fused entry point
(tests/test_gpu_nf4_fused.py), and a row of t without an adapter is +0.0.  Every equality test first asserts on its REFERENCES that,
row by row, the outputs of any two different adapters and of "no adapter" differ somewhere - otherwise a kernel that ignores ids could
pass.  Adapters are of the base's magnitude (test_gpu_nf4_lora.adapter), so that holds by a wide margin.  Only the layer's torch
fallback (70 rows) and the toy decoder are held to float64 bars, which are those of tests/test_gpu_nf4_lora.py."""
import json
import math

import pytest
import torch

import hipabi
import nf4_fused_cases as FC
import nf4_lora_cases as LC
import nf4_multi_lora_cases as MC
from gpu_util import dev
from test_gpu_nf4_fused import GATED, NONE, bs_of, gemm_fused, gemv_fused, guarded, guards_intact, rand, untouched, weight
from test_gpu_nf4_lora import (BS, S, _dense_reference, _layer_products, _nf4_linear, _toy_and_adapter, adapter, adapter_terms, check, down,
                               gemm_lora, gemv_lora)

pytestmark = pytest.mark.gpu
DT16 = [torch.bfloat16, torch.float16]
DT3 = DT16 + [torch.float32]
N = MC.N_ADAPTERS


@pytest.fixture(autouse=True)
def _nf4_variant():
    hipabi.set_variant("gemv_nf4", -1)
    yield
    hipabi.set_variant("gemv_nf4", -1)


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def ids_t(ids):
    return torch.tensor(list(ids), dtype=torch.int32, device=dev())


def down_multi(x, A_stack, scale_stack, ids, t=None, expect_ok=True, n=None, Rr=None, rows=None):
    K = A_stack.shape[2]
    rows = x.numel() // K if rows is None else rows
    Rr = A_stack.shape[1] if Rr is None else Rr
    if t is None:
        t = torch.empty(rows, Rr, dtype=torch.float32, device=x.device)
    rc = MC.lib().fp4_hip_lora_down_multi(hipabi._ptr(x), hipabi._ptr(A_stack), hipabi._ptr(scale_stack), hipabi._ptr(ids), hipabi._ptr(t),
                                          rows, A_stack.shape[0] if n is None else n, Rr, K, hipabi.DT[x.dtype], hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return t
    return rc


def gemm_multi(x, P, Am, M, K, B_stack, ids, t, bs=BS, bias=None, residual=None, epilogue=NONE, out=None, expect_ok=True, Rr=None, B=None,
               n=None, dtype=None):
    B = x.numel() // K if B is None else B
    if out is None:
        out = torch.empty(B, M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = MC.lib().fp4_hip_gemm_lora_multi_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(Am), hipabi._ptr(bias), hipabi._ptr(residual),
                                              hipabi._ptr(B_stack), hipabi._ptr(ids), B_stack.shape[0] if n is None else n, hipabi._ptr(t),
                                              B_stack.shape[-1] if Rr is None else Rr, hipabi._ptr(out), B, M, K, bs,
                                              hipabi.DT[dtype or x.dtype], epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def gemv_multi(x, P, Am, M, K, B_stack, ids, t, bs=BS, bias=None, residual=None, epilogue=NONE, out=None, expect_ok=True, Rr=None, n=None,
               dtype=None):
    if out is None:
        out = torch.empty(M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = MC.lib().fp4_hip_gemv_lora_multi_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(Am), hipabi._ptr(bias), hipabi._ptr(residual),
                                              hipabi._ptr(B_stack), hipabi._ptr(ids), B_stack.shape[0] if n is None else n, hipabi._ptr(t),
                                              B_stack.shape[-1] if Rr is None else Rr, hipabi._ptr(out), M, K, bs,
                                              hipabi.DT[dtype or x.dtype], epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def stack(M, K, r, dtype, seed, n=N):
    """n adapters of test_gpu_nf4_lora.adapter's magnitude, stacked: A [n, r, K], B [n, M, r], scale [n, r] (a factor per adapter)."""
    parts = [adapter(M, K, r, dtype, seed + 17 * a) for a in range(n)]
    scale = torch.stack([p[2] * (1.0 + 0.25 * a) for a, p in enumerate(parts)])
    return torch.stack([p[0] for p in parts]).contiguous(), torch.stack([p[1] for p in parts]).contiguous(), scale.contiguous()


def bits(t):
    """The tensor's bit patterns as integers: +0 and -0 differ, NaNs compare by payload."""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def rows_all_differ(refs):
    """refs: [n_choices, rows, width] - True where every row differs somewhere between any two choices (checked on the references)."""
    for i in range(len(refs)):
        for j in range(i + 1, len(refs)):
            if not bool((bits(refs[i]) != bits(refs[j])).reshape(refs[i].shape[0], -1).any(dim=1).all()):
                return False
    return True


def pick(refs, none, ids):
    """Row b of refs[ids[b]] where ids[b] names an adapter, of `none` where it does not."""
    return torch.stack([refs[i][b] if MC.valid(i) else none[b] for b, i in enumerate(ids)])


# ---- 1. the down projection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT3, ids=str)
def test_down_rows_carry_the_single_adapter_kernels_bits(dtype):
    for K in MC.DOWN_K:
        x64 = rand((64, K), dtype, K)
        for Rr in MC.RANKS:
            A_stack, _, scale_stack = stack(8, K, Rr, dtype, K + Rr)
            for rows in MC.ROWS:
                x = x64[:rows].contiguous()
                refs = torch.stack([down(x, A_stack[a], scale_stack[a]) for a in range(N)])
                zero = torch.zeros(rows, Rr, device=dev())
                assert rows_all_differ(torch.cat([refs, zero[None]]))
                for name, ids in MC.id_patterns(rows).items():
                    buf = torch.full((rows * Rr + 128,), float("nan"), device=dev())
                    t = down_multi(x, A_stack, scale_stack, ids_t(ids), buf[64:64 + rows * Rr].view(rows, Rr))
                    assert bool(buf[:64].isnan().all()) and bool(buf[64 + rows * Rr:].isnan().all()), (K, Rr, rows, name)
                    assert same_bits(t, pick(refs, zero, ids)), (K, Rr, rows, name)  # no-adapter rows: +0.0, bit for bit


# ---- 2. 1..64 rows on the matrix-core kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16, ids=str)
@pytest.mark.parametrize("M,K", MC.BATCH_SHAPES, ids=[f"{m}x{k}" for m, k in MC.BATCH_SHAPES])
def test_batched_rows_carry_the_single_adapter_or_the_plain_fused_bits(M, K, dtype):
    assert (M, K) in FC.BATCH_SHAPES
    P, Am = weight(M, K)
    xs = rand((64, K), dtype, K + 3)
    rs = rand((64, M), dtype, M + 5)
    bias = rand(M, dtype, M, 0.1)
    big = M * K >= 4096 * 4096  # the largest shape: one id pattern per dtype and epilogue
    for Rr in MC.RANKS:
        A_stack, B_stack, scale_stack = stack(M, K, Rr, dtype, Rr)
        for B in LC.batch_rows(K):
            x = x64 = xs[:B].contiguous()
            ts = [down(x, A_stack[a], scale_stack[a]) for a in range(N)]
            patterns = MC.id_patterns(B)
            if big:
                patterns = {"with_none": patterns["with_none"]}
            for epi in (NONE, GATED):
                Mo = M // 2 if epi == GATED else M
                r = rs[:B, :Mo].contiguous()
                for b_, r_ in ((None, None), (bias, r)):
                    refs = torch.stack([gemm_lora(x, P, Am, M, K, B_stack[a], ts[a], bias=b_, residual=r_, epilogue=epi) for a in range(N)])
                    none = gemm_fused(x, P, Am, M, K, BS, b_, r_, epi)
                    assert rows_all_differ(torch.cat([refs, none[None]]))
                    for name, ids in patterns.items():
                        idt = ids_t(ids)
                        t = down_multi(x, A_stack, scale_stack, idt)
                        assert same_bits(t, pick(ts, torch.zeros_like(t), ids))
                        want = pick(refs, none, ids)
                        buf, out = guarded(B * Mo, dtype)
                        got = gemm_multi(x64, P, Am, M, K, B_stack, idt, t, bias=b_, residual=r_, epilogue=epi, out=out.view(B, Mo))
                        assert guards_intact(buf, B * Mo)
                        assert same_bits(got, want), (M, K, Rr, B, epi, name, b_ is not None)
                        if r_ is not None:  # the residual in place
                            h = r.clone()
                            gemm_multi(x, P, Am, M, K, B_stack, idt, t, bias=b_, residual=h, epilogue=epi, out=h)
                            assert same_bits(h, want), (M, K, Rr, B, epi, name, "in place")


# ---- 3. one row ----------------------------------------------------------------------------------------------------------------------------
ONE_ROW_IDS = [0, N - 1] + MC.NO_ADAPTER


def _one_row(M, K, dtypes, epi, what):
    bs = bs_of(K)
    P, Am = weight(M, K, bs)
    Mo = M // 2 if epi == GATED else M
    for dtype in dtypes:
        x = rand(K, dtype, K, 2.0 if epi == GATED else 1.0)
        bias, r = rand(M, dtype, M, 0.1), rand(Mo, dtype, M + 1)
        for Rr in MC.RANKS:
            A_stack, B_stack, scale_stack = stack(M, K, Rr, dtype, Rr + 3)
            ts = [down(x, A_stack[a], scale_stack[a]) for a in range(N)]
            refs = torch.stack([gemv_lora(x, P, Am, M, K, B_stack[a], ts[a], bs, bias, r, epi) for a in range(N)])
            none = gemv_fused(x, P, Am, M, K, bs, bias, r, epi)
            assert rows_all_differ(torch.cat([refs, none[None]])[:, None, :])
            for i in ONE_ROW_IDS:
                idt = ids_t([i])
                t = down_multi(x, A_stack, scale_stack, idt)
                assert same_bits(t, ts[i] if MC.valid(i) else torch.zeros_like(t))
                want = refs[i] if MC.valid(i) else none
                if dtype == torch.float32:
                    got = gemv_multi(x, P, Am, M, K, B_stack, idt, t, bs, bias, r, epi)
                else:
                    buf, out = guarded(Mo, dtype)
                    got = gemv_multi(x, P, Am, M, K, B_stack, idt, t, bs, bias, r, epi, out=out)
                    assert guards_intact(buf, Mo)
                assert same_bits(got, want), (what, M, K, dtype, Rr, i)
                h = r.clone()  # the residual in place
                gemv_multi(x, P, Am, M, K, B_stack, idt, t, bs, bias, h, epi, out=h)
                assert same_bits(h, want), (what, M, K, dtype, Rr, i, "in place")


ONE_ROW_PLAIN = FC.GEMV_PLAIN[1::2]  # one shape per line of nf4_ref.GEMV_CELL_CASES: the one with a row tail
ONE_ROW_GATED = FC.GEMV_GATED[1::2]  # the same with M even


@pytest.mark.parametrize("M,K", ONE_ROW_PLAIN, ids=[f"{m}x{k}" for m, k in ONE_ROW_PLAIN])
def test_one_row_plain_epilogue_every_cell(M, K):
    _one_row(M, K, DT3, NONE, "plain")


@pytest.mark.parametrize("M,K", ONE_ROW_GATED, ids=[f"{m}x{k}" for m, k in ONE_ROW_GATED])
def test_one_row_gated_epilogue_every_cell(M, K):
    _one_row(M, K, DT16, GATED, "gated")


@pytest.mark.parametrize("variant", [0, 1])
def test_one_row_both_table_layouts(variant):
    hipabi.set_variant("gemv_nf4", variant)
    for M, K in FC.GEMV_VARIANT_SHAPES:
        _one_row(M, K, DT3, NONE, ("plain", variant))
        _one_row(M, K, DT16, GATED, ("gated", variant))


# ---- 4. slice offsets past 2^31 elements -------------------------------------------------------------------------------------------------
def test_stack_offsets_beyond_2_pow_31_elements():
    n, M, K, Rr, dtype = 33, 262144, 64, 256, torch.bfloat16
    assert (n - 1) * M * Rr >= 2**31  # the last slice starts past what a 32-bit element offset holds
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip("needs ~8 GiB of free device memory")
    P, Am = weight(M, K)
    B_stack = torch.empty(n, M, Rr, dtype=dtype, device=dev())  # only slices 0 and 32 are filled, and only they are selected
    A_stack = torch.zeros(n, Rr, K, dtype=dtype, device=dev())
    scale_stack = torch.full((n, Rr), S, device=dev())
    for a in (0, n - 1):
        A_stack[a], B_stack[a], _ = adapter(M, K, Rr, dtype, 100 + a)
    ids = [n - 1, 0, -1, n - 1, n]
    x = rand((len(ids), K), dtype, 7)
    ts = {a: down(x, A_stack[a], scale_stack[a]) for a in (0, n - 1)}
    idt = ids_t(ids)
    t = down_multi(x, A_stack, scale_stack, idt)
    for epi in (NONE, GATED):
        refs = {a: gemm_lora(x, P, Am, M, K, B_stack[a], ts[a], epilogue=epi) for a in (0, n - 1)}
        none = gemm_fused(x, P, Am, M, K, BS, None, None, epi)
        assert rows_all_differ(torch.stack([refs[0], refs[n - 1], none]))
        got = gemm_multi(x, P, Am, M, K, B_stack, idt, t, epilogue=epi)
        want = torch.stack([refs[i][b] if i in refs else none[b] for b, i in enumerate(ids)])
        assert same_bits(got, want), epi
        # one row, the last slice
        x1 = x[0].contiguous()
        t1 = down_multi(x1, A_stack, scale_stack, ids_t([n - 1]))
        assert same_bits(t1, ts[n - 1][:1])
        assert same_bits(gemv_multi(x1, P, Am, M, K, B_stack, ids_t([n - 1]), t1, epilogue=epi),
                         gemv_lora(x1, P, Am, M, K, B_stack[n - 1], t1, epilogue=epi)), epi
    del B_stack, A_stack
    torch.cuda.empty_cache()


# ---- 5. capture: a replay follows an in-place rewrite of ids ----------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [8, 1])
def test_a_captured_step_follows_in_place_rewrites_of_ids(rows):
    M, K, Rr, dtype = 1026, 4096, 16, torch.bfloat16
    P, Am = weight(M, K)
    A_stack, B_stack, scale_stack = stack(M, K, Rr, dtype, 1)
    x, r = rand((rows, K), dtype, 2), rand((rows, M), dtype, 3)
    idt = ids_t([0] * rows)
    t, out = torch.empty(rows, Rr, device=dev()), torch.empty(rows, M, dtype=dtype, device=dev())

    def step():
        down_multi(x, A_stack, scale_stack, idt, t)
        if rows == 1:
            gemv_multi(x, P, Am, M, K, B_stack, idt, t, residual=r, out=out)
        else:
            gemm_multi(x, P, Am, M, K, B_stack, idt, t, residual=r, out=out)

    rewrites = [[b % N for b in range(rows)], [-1] * rows, [(N - 1, -7, 1, MC.INT32_MAX)[b % 4] for b in range(rows)]]
    eager = []
    for ids in rewrites:
        idt.copy_(ids_t(ids))
        step()
        eager.append((t.clone(), out.clone()))
    assert not same_bits(eager[0][1], eager[1][1]) and not same_bits(eager[0][1], eager[2][1])
    idt.copy_(ids_t([0] * rows))
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for ids, (t_want, out_want) in zip(rewrites, eager):
        idt.copy_(ids_t(ids))  # in place: the graph holds this tensor's address
        out.zero_()
        t.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(t, t_want) and same_bits(out, out_want), ids


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_and_t_untouched():
    M, K, dtype = 64, 1024, torch.bfloat16
    P, Am = weight(M, K)
    x = rand((65, K), dtype, 1)
    A_stack, _, scale_stack = stack(M, K, 264, dtype, 2, n=2)
    B_stack = rand((2, M + 1, 264), dtype, 3)
    idt = ids_t([0, 1] * 33)
    t = torch.full((65 * 264 + 8,), 7.0, device=dev())
    buf, out = guarded(65 * M, dtype)
    x32 = x.float()
    U, I = hipabi.ERR_UNSUPPORTED, hipabi.ERR_INVALID
    d = lambda **k: down_multi(x, A_stack, scale_stack, idt, t, expect_ok=False, **{"rows": 4, "Rr": 8, **k})
    v = lambda **k: gemv_multi(x, P, Am, M, K, B_stack, idt, t, out=out, expect_ok=False, **{"Rr": 8, **k})
    m = lambda **k: gemm_multi(x, P, Am, M, K, B_stack, idt, t, out=out, expect_ok=False, **{"B": 4, "Rr": 8, **k})
    assert d(rows=65) == U and "not covered" in hipabi.last_error()
    assert m(B=65) == U and "not covered" in hipabi.last_error()
    for call in (d, v, m):
        assert call(Rr=12) == U
        assert call(Rr=264) == U
        assert call(n=0) == I and "n_adapters" in hipabi.last_error()
    # a stack offset by 2 bytes
    assert MC.lib().fp4_hip_lora_down_multi(hipabi._ptr(x), A_stack.data_ptr() + 2, hipabi._ptr(scale_stack), hipabi._ptr(idt), hipabi._ptr(t),
                                            4, 2, 8, K, hipabi.BF16, hipabi._stream()) == U
    off = B_stack.reshape(-1)[1:]
    for epi in (NONE, GATED):
        assert MC.lib().fp4_hip_gemm_lora_multi_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(Am), None, None, hipabi._ptr(off), hipabi._ptr(idt),
                                                    2, hipabi._ptr(t), 8, hipabi._ptr(out), 4, M, K, BS, hipabi.BF16, epi, hipabi._stream()) == U
        assert "not available" in hipabi.last_error()
        assert MC.lib().fp4_hip_gemv_lora_multi_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(Am), None, None, hipabi._ptr(off), hipabi._ptr(idt),
                                                    2, hipabi._ptr(t), 8, hipabi._ptr(out), M, K, BS, hipabi.BF16, epi, hipabi._stream()) == U
    # f32 with the gated epilogue
    assert gemv_multi(x32, P, Am, M, K, B_stack.float(), idt, t, out=out, expect_ok=False, Rr=8, epilogue=GATED) == U
    assert "not available" in hipabi.last_error()
    assert gemm_multi(x32, P, Am, M, K, B_stack.float(), idt, t, out=out, expect_ok=False, B=4, Rr=8, epilogue=GATED) == U
    # null ids, odd M with the gated epilogue, an unknown epilogue
    null = MC.lib()
    assert null.fp4_hip_lora_down_multi(hipabi._ptr(x), hipabi._ptr(A_stack), hipabi._ptr(scale_stack), None, hipabi._ptr(t), 4, 2, 8, K,
                                        hipabi.BF16, hipabi._stream()) == I
    assert null.fp4_hip_gemm_lora_multi_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(Am), None, None, hipabi._ptr(B_stack), None, 2,
                                            hipabi._ptr(t), 8, hipabi._ptr(out), 4, M, K, BS, hipabi.BF16, NONE, hipabi._stream()) == I
    assert null.fp4_hip_gemv_lora_multi_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(Am), None, None, hipabi._ptr(B_stack), None, 2,
                                            hipabi._ptr(t), 8, hipabi._ptr(out), M, K, BS, hipabi.BF16, NONE, hipabi._stream()) == I
    for call in (v, m):
        assert call(epilogue=7) == I and "unknown epilogue" in hipabi.last_error()
    assert gemv_multi(x, P, Am, M - 1, K, B_stack, idt, t, out=out, expect_ok=False, Rr=8, epilogue=GATED) == I
    assert "even row count" in hipabi.last_error()
    assert gemm_multi(x, P, Am, M - 1, K, B_stack, idt, t, out=out, expect_ok=False, B=4, Rr=8, epilogue=GATED) == I
    assert "even row count" in hipabi.last_error()
    torch.cuda.synchronize()
    assert untouched(buf) and bool((t == 7.0).all())


# ---- 7. torch ops ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16, ids=str)
def test_torch_ops_equal_the_c_abi_bit_for_bit(dtype):
    import torch_bnb_fp4 as pkg

    M, K, Rr = 258, 2048, 24
    P, Am = weight(M, K)
    Bt = P.reshape(-1, 1).t()
    A_stack, B_stack, scale_stack = stack(M, K, Rr, dtype, 1)
    b = rand(M, dtype, M, 0.1)
    sel = ids_t([(0, -1, 2, 1, N)[i % 5] for i in range(64)])  # longer than the batch: the first `rows` ids are used
    for rows in (1, 5, 40):
        x = rand((rows, K), dtype, rows, 2.0)
        t = pkg.ext.lora_down_multi(x, A_stack, scale_stack, sel)
        assert t.dtype == torch.float32 and t.shape == (rows, Rr) and same_bits(t, down_multi(x, A_stack, scale_stack, sel))
        for epi in (NONE, GATED):
            r = rand((rows, M // 2 if epi == GATED else M), dtype, 9)
            if rows == 1:
                got = pkg.ext.gemv_nf4_lora_multi(x, Bt, Am, BS, [M, K], b, r, epi, B_stack, sel, t)
                assert same_bits(got, gemv_multi(x.reshape(-1), P, Am, M, K, B_stack, sel, t, BS, b, r.reshape(-1), epi).reshape(1, -1))
            got = pkg.ext.gemm_nf4_lora_multi(x, Bt, Am, BS, [M, K], b, r, epi, B_stack, sel, t)
            assert same_bits(got, gemm_multi(x, P, Am, M, K, B_stack, sel, t, BS, b, r, epi)) and got.shape == (rows, M // 2 if epi == GATED else M)
    with pytest.raises(RuntimeError, match="ids must be"):
        pkg.ext.lora_down_multi(x, A_stack, scale_stack, sel[:3])          # fewer ids than rows
    with pytest.raises(RuntimeError, match="ids must be"):
        pkg.ext.gemm_nf4_lora_multi(x, Bt, Am, BS, [M, K], None, None, NONE, B_stack, sel.long(), t)
    with pytest.raises(RuntimeError, match="A_stack must be"):
        pkg.ext.lora_down_multi(x, A_stack[0], scale_stack, sel)
    with pytest.raises(RuntimeError, match="B_stack must be"):
        pkg.ext.gemm_nf4_lora_multi(x, Bt, Am, BS, [M, K], None, None, NONE, B_stack[:, :-1].contiguous(), sel, t)
    with pytest.raises(RuntimeError, match="not available"):
        pkg.ext.gemv_nf4_lora_multi(x[:1].contiguous(), Bt, Am, BS, [M, K], None, None, NONE, B_stack[:, :, :12].contiguous(), sel,
                                    t[:1, :12].contiguous())
    with pytest.raises(RuntimeError, match="not covered"):
        pkg.ext.lora_down_multi(rand((65, K), dtype, 1), A_stack, scale_stack, ids_t([0] * 65))


# the host layer's mistake table (tests/test_gpu_ext_checks.py: every mistake a weight op's signature allows, then good operands
# against the C ABI) applied to the two multi-adapter weight ops, plus the mistakes their own operands allow.  That file's list of
# ops is keyed on the ops' doc strings and is left as it is; the two ops are held to the same table here.
def _multi_ops():
    import test_gpu_ext_checks as X

    class MultiOp(X.Op):
        def operands(self):
            if not hasattr(self, "_operands"):
                a = dict(X.Op.operands(self))
                K = self.K
                A_stack, a["B_stack"], scale_stack = stack(X.M, K, X.RANK, X.DT, 21, n=2)
                a["ids"] = ids_t([1, -1, 0, 1][: self.rows])
                a["t"] = down_multi(a["A"], A_stack, scale_stack, a["ids"])
                self._operands = a
            return self._operands

    order = X.FUSED + ("B_stack", "ids", "t")
    flat = lambda a, *names: [None if a.get(n) is None else a[n].reshape(-1) for n in names]  # noqa: E731
    return X, [
        MultiOp("gemv_nf4_lora_multi", order, 64, 1, 1,
                lambda a: gemv_multi(a["A"].reshape(-1), a["P"], a["absmax"], X.M, a["Bshape"][1], a["B_stack"], a["ids"], a["t"], BS,
                                     *flat(a, "bias", "residual"), a["epilogue"]).reshape(1, -1), {"last dim is not K": "in_features"}),
        MultiOp("gemm_nf4_lora_multi", order, 512, 4, 128,
                lambda a: gemm_multi(a["A"], a["P"], a["absmax"], X.M, a["Bshape"][1], a["B_stack"], a["ids"], a["t"], BS, a["bias"],
                                     a["residual"], a["epilogue"])),
    ]


@pytest.mark.parametrize("which", [0, 1], ids=["gemv_nf4_lora_multi", "gemm_nf4_lora_multi"])
def test_weight_ops_refuse_every_mistake_of_the_shared_table_and_of_their_own_operands(which):
    X, ops = _multi_ops()
    op = ops[which]
    X.test_every_mistake_is_refused_and_good_operands_reach_the_c_abi_untouched(op)
    good = op.operands()
    own = {
        "ids of int64": (dict(good, ids=good["ids"].long()), "ids must be"),
        "fewer ids than rows": (dict(good, ids=good["ids"][:0]), "ids must be"),
        "ids on the host": (dict(good, ids=good["ids"].cpu()), "must be a CUDA tensor"),
        "a single adapter's B": (dict(good, B_stack=good["B_stack"][0]), "B_stack must be"),
        "B_stack of m - 1 rows": (dict(good, B_stack=good["B_stack"][:, :-1].contiguous()), "B_stack must be"),
        "B_stack of the other 16-bit dtype": (dict(good, B_stack=good["B_stack"].to(torch.float16)), "B_stack must be"),
        "t of the wrong numel": (dict(good, t=good["t"].reshape(-1)[:-1]), "t must hold"),
        "t in bf16": (dict(good, t=good["t"].to(torch.bfloat16)), "t must hold"),
    }
    for mistake, (a, substring) in own.items():
        with pytest.raises(RuntimeError) as info:
            op(a)
        assert substring in str(info.value), (op, mistake, str(info.value))


# ---- 8. the layer, fused route -------------------------------------------------------------------------------------------------------------
def _fused_258(dtype):
    import torch_bnb_fp4 as pkg

    M, K = 258, 2048
    P, Am = weight(M, K)
    mk = lambda: pkg.FusedNF4Linear.from_packed(P.reshape(-1, 1), Am, (M, K), BS, dtype=dtype)
    return pkg, M, K, mk


@pytest.mark.parametrize("dtype", DT16, ids=str)
def test_layer_rows_equal_the_single_adapter_layer_and_the_plain_layer(dtype):
    import torch_bnb_fp4.fused as fused_mod

    pkg, M, K, mk = _fused_258(dtype)
    r = 16
    ads = [adapter(M, K, r, dtype, 11 * a + 1)[:2] + (S * (1 + a),) for a in range(N)]
    sel = pkg.AdapterSelection(dev())
    ptr = sel.set([0]).ids.data_ptr()
    multi = pkg.MultiLoRANF4Linear.from_fused(mk(), ads, sel)
    singles = [pkg.LoRANF4Linear.from_fused(mk(), *ad) for ad in ads]
    plain = mk()
    xs, res = rand((40, K), dtype, 9), rand((40, M), dtype, 10)
    for rows in (1, 8, 40):
        assert fused_mod.lora_fused_ahead(rows, M, K, r)
        x, rr = xs[:rows].contiguous(), res[:rows].contiguous()
        refs = torch.stack([s(x, rr) for s in singles])
        none = plain(x, rr)
        assert rows_all_differ(torch.cat([refs, none[None]]))
        for name, ids in MC.id_patterns(rows).items():
            sel.set(ids)
            assert sel.ids.data_ptr() == ptr and len(sel) == rows
            got = multi(x, rr)
            assert got.shape == (rows, M) and same_bits(got, pick(refs, none, ids)), (rows, name)
    assert multi._fused_ok and multi._small_ok and multi._lora_ok and all(s._fused_ok and s._small_ok and s._lora_ok for s in singles)


@pytest.mark.parametrize("dtype", DT16, ids=str)
def test_gate_up_layer_rows_equal_the_single_adapter_gate_up_layer(dtype):
    pkg, M, K, _ = _fused_258(dtype)
    P, Am = weight(M, K)  # rows as an interleaved gate|up weight: M / 2 outputs
    mk = lambda: pkg.FusedNF4Linear(pkg.FusedNF4Linear.from_packed(P.reshape(-1, 1), Am, (M, K), BS, dtype=dtype).quant_data, GATED)
    H = M // 2
    pairs = [((*adapter(H, K, 8, dtype, 5 * a + 1)[:2], S), (*adapter(H, K, 12, dtype, 5 * a + 2)[:2], 0.5 * (a + 1))) for a in range(N)]
    sel = pkg.AdapterSelection(dev())
    multi = pkg.MultiLoRANF4Linear.gate_up_from_fused(mk(), pairs, sel)
    singles = [pkg.LoRANF4Linear.gate_up_from_fused(mk(), g, u) for g, u in pairs]
    plain = mk()
    assert multi.rank == 24 and multi.epilogue == GATED
    xs = rand((40, K), dtype, 9, 2.0)
    for rows in (1, 8, 40):
        x = xs[:rows].contiguous()
        refs = torch.stack([s(x) for s in singles])
        none = plain(x)
        assert rows_all_differ(torch.cat([refs, none[None]]))
        for name, ids in MC.id_patterns(rows).items():
            sel.set(ids)
            got = multi(x)
            assert got.shape == (rows, H) and same_bits(got, pick(refs, none, ids)), (rows, name)
    assert multi._fused_ok and multi._small_ok and multi._lora_ok


def test_mixed_ranks_are_padded_to_one_common_rank():
    """Ranks 4, 8, 24 -> common rank 24: each row equals, as numbers, a LoRANF4Linear whose adapter was padded to 24 by hand (zero
    rows of A and zero columns of B add exact zeros to the same f32 chain)."""
    dtype = torch.bfloat16
    pkg, M, K, mk = _fused_258(dtype)
    ranks = (4, 8, 24)
    ads = [adapter(M, K, r, dtype, 3 * r)[:2] + (S,) for r in ranks]
    sel = pkg.AdapterSelection(dev())
    multi = pkg.MultiLoRANF4Linear.from_fused(mk(), ads, sel)
    assert multi.rank == 24 and multi.ranks == list(ranks) and tuple(multi.lora_B_stack.shape) == (3, M, 24)
    singles = []
    for (A, B, s), r in zip(ads, ranks):
        A24 = torch.cat([A, A.new_zeros(24 - r, K)], 0)
        B24 = torch.cat([B, B.new_zeros(M, 24 - r)], 1).contiguous()
        s24 = torch.cat([torch.full((r,), s), torch.zeros(24 - r)]).to(dev())
        singles.append(pkg.LoRANF4Linear.from_fused(mk(), A24, B24, s24))
    xs = rand((40, K), dtype, 4)
    for rows in (1, 8, 40):
        x = xs[:rows].contiguous()
        refs = torch.stack([s(x) for s in singles])
        none = mk()(x)
        assert rows_all_differ(torch.cat([refs, none[None]]))
        ids = MC.id_patterns(rows)["with_none"] if rows > 1 else [2]
        sel.set(ids)
        assert torch.equal(multi(x), pick(refs, none, ids)), rows


# ---- 9. the layer, fallback ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16, ids=str)
def test_layer_fallback_at_70_rows_against_the_oracle(dtype):
    """The bar is the one tests/test_gpu_nf4_lora.py holds LoRANF4Linear's 70-row fallback to (its `check`, both forms): against the
    exact-weight oracle with the fallback's base term and the weight rounding's worst case, and - the check that holds the adapter
    term - against the parent's own output for the base at the fused ops' bar without its base term."""
    import torch_bnb_fp4 as pkg

    K, M, r, rows = 512, 384, 16, 70
    lin = _nf4_linear(M, K, dtype, 1)
    ads = [adapter(M, K, r, dtype, 7 * a + 1) for a in range(N)]
    sel = pkg.AdapterSelection(dev(), capacity=128)
    layer = pkg.MultiLoRANF4Linear.from_linear(lin, [(A, B, S) for A, B, _ in ads], sel)
    ids = [(0, -1, 2, 1, N, 1)[b % 6] for b in range(rows)]
    sel.set(ids)
    x = rand((rows, K), dtype, 11)
    exact, s1 = _layer_products(lin, x)
    d, s2 = torch.zeros_like(exact), torch.zeros_like(s1)
    for a, (A, B, scale) in enumerate(ads):
        mask = torch.tensor([i == a for i in ids], device=dev()).unsqueeze(1)
        da, sa = adapter_terms(x, A, B, scale)
        d, s2 = torch.where(mask, da, d), torch.where(mask, sa, s2)
    y = layer(x)
    assert y.shape == (rows, M)
    check(y, exact + d, s1, s2, dtype, ("multi layer, 70 rows, oracle", dtype), base=exact, weights_rounded=True)
    base = pkg.FusedNF4Linear.from_linear(lin)(x).double()
    check(y, base + d, torch.zeros_like(s1), s2, dtype, ("multi layer, 70 rows, on the parent's base", dtype))
    none_rows = [b for b, i in enumerate(ids) if not MC.valid(i)]
    assert torch.equal(y[none_rows], pkg.FusedNF4Linear.from_linear(lin)(x)[none_rows])  # +0 added in f32, one cast: the base's values
    with pytest.raises(ValueError, match="one id per row"):
        layer(x[:69].contiguous())


# ---- 10. attach and load ---------------------------------------------------------------------------------------------------------------
TOY_MODULES = (("self_attn.q_proj", "HH"), ("self_attn.o_proj", "HH"), ("mlp.gate_proj", "IH"), ("mlp.up_proj", "IH"), ("mlp.down_proj", "HI"))


def _toy_state(H, I, r, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    dims = {"H": H, "I": I}
    state = {}
    for i in range(2):
        for name, (m, k) in TOY_MODULES:
            A, B = torch.randn(r, dims[k], generator=g) / math.sqrt(dims[k]), torch.randn(dims[m], r, generator=g) * 0.05
            if (i, name) not in skip:
                state[f"base_model.model.model.layers.{i}.{name}.lora_A.weight"] = A
                state[f"base_model.model.model.layers.{i}.{name}.lora_B.weight"] = B
    return state


def _filled(state, H, I, r):
    """The state with zero tensors for the modules it lacks (what the float64 reference indexes)."""
    full = {k: torch.zeros_like(v) for k, v in _toy_state(H, I, r, 0).items()}
    full.update(state)
    return full


def test_attach_lora_adapters_and_load_lora_adapters_on_a_toy_decoder(tmp_path):
    import torch_bnb_fp4 as pkg
    from oracle import torch_cpu
    from safetensors.torch import save_file
    import nf4_ref as R

    H, I, dtype = 512, 768, torch.bfloat16
    specs = {"tenant_a": (4, 8, False, ()), "tenant_b": (8, 16, False, ((1, "self_attn.o_proj"),)), "tenant_c": (4, 4, True, ())}
    states = {name: _toy_state(H, I, r, 40 + j, skip) for j, (name, (r, _, _, skip)) in enumerate(specs.items())}
    adapters = {name: (states[name], r, alpha, rs) for name, (r, alpha, rs, _) in specs.items()}

    def fresh():
        toy, _ = _toy_and_adapter(H, I, 4, dtype)
        assert pkg.fuse_gated_mlps(toy, nf4=True) == 2
        return toy

    toy, _ = _toy_and_adapter(H, I, 4, dtype)
    code = torch.from_numpy(R.CODE.copy()).to(dev())
    dense = {}
    for i, blk in enumerate(toy.model.layers):
        for name, _ in TOY_MODULES:
            qd = blk.get_submodule(name).quant_data
            dense[(i, name)] = torch_cpu.dequantize(qd.A.reshape(-1), qd.absmax, int(qd.M), int(qd.N), qd.blocksize, torch.float32, code).double()
    assert pkg.fuse_gated_mlps(toy, nf4=True) == 2
    sel = pkg.attach_lora_adapters(toy, adapters)
    assert isinstance(sel, pkg.AdapterSelection) and sel.names == list(specs) and sel.n_layers == 8
    blk = toy.model.layers[1]
    assert type(blk.self_attn.q_proj) is pkg.MultiLoRANF4Linear and type(blk.mlp.gate_up) is pkg.MultiLoRANF4Linear
    assert blk.self_attn.q_proj.selection is sel and blk.mlp.gate_up.selection is sel and blk.mlp.gate_up.rank == 16
    o_proj = blk.self_attn.o_proj
    assert o_proj.n_adapters == 3 and float(o_proj.lora_B_stack[1].abs().max()) == 0.0 and float(o_proj.lora_A_stack[1].abs().max()) == 0.0
    assert float(o_proj.lora_B_stack[0].abs().max()) > 0 and float(toy.model.layers[0].self_attn.o_proj.lora_B_stack[1].abs().max()) > 0

    def want_for(h, names):
        rows = []
        for b, name in enumerate(names):
            if name is None:
                st, s = {k: torch.zeros_like(v) for k, v in _filled({}, H, I, 4).items()}, 0.0
            else:
                r, alpha, rs, _ = specs[name]
                st, s = _filled(states[name], H, I, r), alpha / (math.sqrt(r) if rs else r)
            rows.append(_dense_reference(dense, st, s, h[b:b + 1]))
        return torch.cat(rows)

    for names in (["tenant_b"], ["tenant_a", None, "tenant_c", "tenant_b", "tenant_b", None, "tenant_a", "tenant_c"]):
        rows = len(names)
        sel.set_by_name(names)
        assert sel.ids.tolist() == [-1 if n is None else list(specs).index(n) for n in names]
        h = rand((rows, H), dtype, rows, 0.5)
        got = toy(h)
        want = want_for(h, names)
        base_only = want_for(h, [None] * rows)
        for b, name in enumerate(names):  # per sequence, at the bar of tests/test_gpu_nf4_lora.py's toy decoder
            rel = float((got[b].double() - want[b]).abs().max() / want[b].abs().max())
            print(f"toy decoder, {rows} rows, row {b} ({name}): max |err| / max |want| = {rel:.4f}")
            assert rel <= 2e-2, (rows, b, name, rel)
            if name is not None:
                assert float((want[b] - base_only[b]).abs().max() / want[b].abs().max()) >= 0.1
    with pytest.raises(KeyError, match="no adapter named"):
        sel.set_by_name(["tenant_z"])
    # the same adapters from directories in peft's layout give the same model, bit for bit
    dirs = {}
    for name, (r, alpha, rs, skip) in specs.items():
        d = tmp_path / name
        d.mkdir()
        save_file(states[name], str(d / "adapter_model.safetensors"))
        (d / "adapter_config.json").write_text(json.dumps({"r": r, "lora_alpha": alpha, "use_rslora": rs, "peft_type": "LORA",
                                                           "target_modules": ["q_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]}))
        dirs[name] = str(d)
    toy2 = fresh()
    sel2 = pkg.load_lora_adapters(toy2, dirs)
    assert sel2.names == list(specs) and sel2.n_layers == 8
    names = ["tenant_c", None, "tenant_b", "tenant_a"]
    sel.set_by_name(names)
    sel2.set_by_name(names)
    h = rand((4, H), dtype, 5, 0.5)
    assert torch.equal(toy2(h), toy(h))
    toy3 = fresh()
    with pytest.raises(KeyError, match="no such module"):
        pkg.attach_lora_adapters(toy3, {"x": ({"base_model.model.model.layers.5.self_attn.q_proj.lora_A.weight": torch.zeros(4, H),
                                               "base_model.model.model.layers.5.self_attn.q_proj.lora_B.weight": torch.zeros(H, 4)}, 4, 8, False)})
    assert type(toy3.model.layers[0].self_attn.q_proj) is not pkg.MultiLoRANF4Linear  # a call that raises leaves the model as it was
