"""Double-quantised (nested) absmax read directly by the 1..64-row NF4 kernels and beside a LoRA adapter: fp4_hip_gemm_nested_nf4,
fp4_hip_gemm_lora_nested_nf4 and fp4_hip_gemv_lora_nested_nf4 through the C ABI, then the torch ops and the modules.

One bar: EQUAL BITS with the un-nested entry point (fp4_hip_gemm_fused_nf4, fp4_hip_gemm_lora_nf4, fp4_hip_gemv_lora_nf4) on the
ORACLE-expanded absmax (tests/nested_ref.py, numpy on the CPU) - the kernels differ from their twins only in how they obtain the
block's scale, so no tolerance applies.  The cases are tests/nested_batch_cases.py's; tests/test_nested_batch_host.py shows that
they reach every dispatcher cell."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

import hipabi
import nested_batch_cases as NB
import nested_ref as N
import nf4_fused_cases as FC
from gpu_util import dev, to_dev
from test_gpu_nf4_fused import DT16, GATED, NONE, bs_of, gemm_fused, guarded, guards_intact, rand, untouched
from test_gpu_nf4_lora import adapter, down, gemm_lora, gemv_lora

pytestmark = pytest.mark.gpu
BS = 64


@pytest.fixture(autouse=True)
def _variants():
    yield
    hipabi.set_variant("gemm_wide_nf4", -1)
    hipabi.set_variant("gemv_nf4", -1)


@functools.lru_cache(maxsize=1)
def table():
    return N.dynamic_map()


@functools.lru_cache(maxsize=1)
def table_dev():
    return to_dev(table())


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def gemm_nested(x, P, q, nested, code, offset, M, K, bias=None, residual=None, epilogue=NONE, out=None, g=256, expect_ok=True, bs=BS,
                dtype=None, B=None):
    B = x.numel() // K if B is None else B
    if out is None:
        out = torch.empty(B, M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = NB.lib().fp4_hip_gemm_nested_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(q), hipabi._ptr(nested), hipabi._ptr(code), offset, g,
                                          hipabi._ptr(bias), hipabi._ptr(residual), hipabi._ptr(out), B, M, K, bs,
                                          hipabi.DT[dtype or x.dtype], epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def gemm_lora_nested(x, P, q, nested, code, offset, M, K, lB, t, bias=None, residual=None, epilogue=NONE, out=None, g=256, expect_ok=True,
                     bs=BS, dtype=None, B=None, Rr=None):
    B = x.numel() // K if B is None else B
    if out is None:
        out = torch.empty(B, M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = NB.lib().fp4_hip_gemm_lora_nested_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(q), hipabi._ptr(nested), hipabi._ptr(code), offset,
                                               g, hipabi._ptr(bias), hipabi._ptr(residual), hipabi._ptr(lB), hipabi._ptr(t),
                                               lB.shape[1] if Rr is None else Rr, hipabi._ptr(out), B, M, K, bs,
                                               hipabi.DT[dtype or x.dtype], epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


def gemv_lora_nested(x, P, q, nested, code, offset, M, K, lB, t, bias=None, residual=None, epilogue=NONE, out=None, g=256, expect_ok=True,
                     bs=BS, dtype=None, Rr=None):
    if out is None:
        out = torch.empty(M // 2 if epilogue == GATED else M, dtype=x.dtype, device=x.device)
    rc = NB.lib().fp4_hip_gemv_lora_nested_nf4(hipabi._ptr(x), hipabi._ptr(P), hipabi._ptr(q), hipabi._ptr(nested), hipabi._ptr(code), offset,
                                               g, hipabi._ptr(bias), hipabi._ptr(residual), hipabi._ptr(lB), hipabi._ptr(t),
                                               lB.shape[1] if Rr is None else Rr, hipabi._ptr(out), M, K, bs, hipabi.DT[dtype or x.dtype],
                                               epilogue, hipabi._stream())
    if expect_ok:
        assert rc == hipabi.OK, (rc, hipabi.last_error())
        return out
    return rc


@functools.lru_cache(maxsize=None)
def nested_weight(M, K, offset=0.0237, bs=BS):
    """Random NF4 bytes with double-quantised statistics - every code present where there are 256 blocks, a scale of its own per
    group, one group of scale zero where there are more than two - and the ORACLE's expansion of them (numpy, on the CPU) as the f32
    absmax the un-nested entry point is given.  Made once per (shape, offset) and only read."""
    g = torch.Generator(device=dev()).manual_seed(29 * M + K)
    packed = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev(), generator=g)
    nb = M * K // bs
    rng = np.random.default_rng(M * 3 + K)
    q = rng.integers(0, 256, nb).astype(np.uint8)
    if nb >= 256:
        q[rng.permutation(nb)[:256]] = np.arange(256, dtype=np.uint8)
        assert len(set(q.tolist())) == 256
    ng = -(-nb // 256)
    nested = (rng.random(ng) * 0.03 + 0.01).astype(np.float32)
    if ng > 2:
        nested[1] = 0.0  # a group that expands to exactly the offset
    offset = float(np.float32(offset))
    expanded = N.unnest(q, nested, table(), offset, 256)
    return packed, to_dev(q), to_dev(nested), offset, to_dev(expanded)


def check_every_form(rows, M, Mg, K, dtype, offset=0.0237, what=""):
    """plain, bias + residual, residual in place (residual == out) on an [M, K] weight; gate|up with bias (and residual, and in
    place) on an [Mg, K] weight; each against fp4_hip_gemm_fused_nf4 on the oracle-expanded absmax, into guarded outputs."""
    code = table_dev()
    P, q, nested, off, A = nested_weight(M, K, offset)
    x, b, r = rand((rows, K), dtype, rows + K, 0.5), rand(M, dtype, M, 0.1), rand((rows, M), dtype, M + 1)
    for bias, res in ((None, None), (b, r), (None, r)):
        buf, out = guarded(rows * M, dtype)
        got = gemm_nested(x, P, q, nested, code, off, M, K, bias, res, out=out.view(rows, M))
        want = gemm_fused(x, P, A, M, K, BS, bias, res)
        assert guards_intact(buf, rows * M)
        assert torch.equal(got, want), (what, rows, M, K, dtype, bias is not None, res is not None, int((got != want).sum()))
    h = r.clone()
    gemm_nested(x, P, q, nested, code, off, M, K, b, h, out=h)
    assert torch.equal(h, gemm_fused(x, P, A, M, K, BS, b, r)), (what, rows, M, K, dtype, "in place")
    P, q, nested, off, A = nested_weight(Mg, K, offset)
    b, r = rand(Mg, dtype, Mg, 0.1), rand((rows, Mg // 2), dtype, Mg + 1)
    for bias, res in ((b, None), (b, r)):
        buf, out = guarded(rows * Mg // 2, dtype)
        got = gemm_nested(x, P, q, nested, code, off, Mg, K, bias, res, GATED, out=out.view(rows, Mg // 2))
        assert guards_intact(buf, rows * Mg // 2)
        assert torch.equal(got, gemm_fused(x, P, A, Mg, K, BS, bias, res, GATED)), (what, rows, Mg, K, dtype, "gated", res is not None)
    h = r.clone()
    gemm_nested(x, P, q, nested, code, off, Mg, K, b, h, GATED, out=h)
    assert torch.equal(h, gemm_fused(x, P, A, Mg, K, BS, b, r, GATED)), (what, rows, Mg, K, dtype, "gated in place")


# ---- every dispatcher cell -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16, ids=str)
@pytest.mark.parametrize("K", NB.SMALL_K)
def test_small_kernel_every_cell_and_epilogue(K, dtype):
    for M, Mg in zip(NB.SMALL_M, NB.SMALL_M_GATED):
        for rows in NB.SMALL_ROWS:
            check_every_form(rows, M, Mg, K, dtype, what=f"small {NB.small_cell(rows, M, K)}")


@pytest.mark.parametrize("dtype", DT16, ids=str)
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("K", NB.WIDE_K)
def test_wide_kernel_every_cell_and_epilogue(K, variant, dtype):
    hipabi.set_variant("gemm_wide_nf4", variant)  # 16 / 32 weight rows per workgroup, for the nested call and its twin alike
    for rows in NB.WIDE_ROWS:
        check_every_form(rows, NB.WIDE_M, NB.WIDE_M_GATED, K, dtype, what=f"wide {NB.wide_cell(rows, K, variant)}")


@pytest.mark.parametrize("rows,M,K", NB.CHUNKED)
def test_65_and_128_rows_are_two_chunks(rows, M, K):
    for dtype in DT16:
        check_every_form(rows, M, M + (M & 1), K, dtype, what="two chunks")


# ---- group geometry and values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,M,K,what", NB.GEOMETRY, ids=[f"{r}x{m}x{k}" for r, m, k, _ in NB.GEOMETRY])
def test_group_geometry_with_every_offset_sign(rows, M, K, what):
    for offset in NB.OFFSETS:
        check_every_form(rows, M, M + (M & 1), K, torch.bfloat16, offset, what)
    check_every_form(rows, M, M + (M & 1), K, torch.float16, NB.OFFSETS[0], what)


def test_statistics_on_which_two_roundings_and_an_fma_differ():
    """The fixture of the unnest tests (1000 blocks of 64 draws of 0.05 * N(0, 1), nested by the oracle with offset = mean): shown
    here, on the CPU, to tell multiply-then-add from a fused multiply-add, then run as the statistics of a 25 x 2560 weight through
    both kernels.  The outputs are 16-bit, so one f32 ulp in a scale moves an fp16 output across a rounding boundary about twice in
    10^5 outputs: the second half repeats the fixture's first three whole groups over weights with 5 * 10^5 and 2 * 10^6 outputs and
    shows that there the un-nested twin on FMA-rounded scales gives other bits - a kernel that formed the scale with one rounding
    misses the bit-exact bar on it."""
    a = N.recipe_absmax()
    offset = float(np.float32(a.mean()))
    q, nested, _ = N.nest(a, offset, table(), 256)
    two, fma = N.unnest(q, nested, table(), offset, 256), N.unnest_fma(q, nested, table(), offset, 256)
    differ = int((two.view(np.uint32) != fma.view(np.uint32)).sum())
    print(f"{differ} of {a.size} expanded values differ between two roundings and an FMA")
    assert differ >= a.size // 100
    M, K = 25, 2560
    assert M * K // BS == a.size
    g = torch.Generator(device=dev()).manual_seed(11)
    P = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev(), generator=g)
    qd, nd, A, A_fma = to_dev(q), to_dev(nested), to_dev(two), to_dev(fma)
    for dtype in DT16:
        for rows in (4, 17):  # the small kernel (K % 512 == 0), the wide one
            x = rand((rows, K), dtype, rows, 0.5)
            got = gemm_nested(x, P, qd, nd, table_dev(), offset, M, K)
            assert torch.equal(got, gemm_fused(x, P, A, M, K))
        lA, lB, scale = adapter(M, K, 8, dtype, 3)
        x1 = rand(K, dtype, 1, 0.5)
        t1 = down(x1, lA, scale)
        assert torch.equal(gemv_lora_nested(x1, P, qd, nd, table_dev(), offset, M, K, lB, t1), gemv_lora(x1, P, A, M, K, lB, t1))
    # f32 outputs show a scale's last bit directly: the GEMV with the adapter, 25 rows
    x1 = rand(K, torch.float32, 1, 0.5)
    lA, lB, scale = adapter(M, K, 8, torch.float32, 3)
    t1 = down(x1, lA, scale)
    got = gemv_lora_nested(x1, P, qd, nd, table_dev(), offset, M, K, lB, t1)
    assert torch.equal(got, gemv_lora(x1, P, A, M, K, lB, t1)) and not torch.equal(got, gemv_lora(x1, P, A_fma, M, K, lB, t1))
    # the batched kernels, fp16: three whole groups of the fixture, repeated
    reps = 334
    qr, nr = np.tile(q[:768], reps), np.tile(nested[:3], reps)
    two, fma = N.unnest(qr, nr, table(), offset, 256), N.unnest_fma(qr, nr, table(), offset, 256)
    qd, nd, A, A_fma = to_dev(qr), to_dev(nr), to_dev(two), to_dev(fma)
    for rows, M, K in ((16, 32064, 512), (17, 128256, 128)):  # the small kernel, the wide one
        assert M * K // BS == qr.size
        P = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev(), generator=g)
        x = rand((rows, K), torch.float16, rows, 0.5)
        got = gemm_nested(x, P, qd, nd, table_dev(), offset, M, K)
        assert torch.equal(got, gemm_fused(x, P, A, M, K))
        moved = int((got != gemm_fused(x, P, A_fma, M, K)).sum())
        print(f"{rows} rows, {M} x {K}: {moved} of {got.numel()} fp16 outputs differ on FMA-rounded scales")
        assert moved > 0


# ---- guards ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,M,K", [(8, 33, 1536), (5, 16, 2048), (17, 33, 320), (64, 33, 768), (1, 33, 320)])
def test_statistics_carved_out_of_larger_tensors_and_offset_operands(rows, M, K):
    """absmax_u8 and nested_absmax are slices of larger tensors.  The bytes around the codes are 255 and the table's entry 255 is
    +inf (no code in range uses it); the floats around the group scales are NaN: a code or a group scale read from outside its array
    decodes to inf / NaN and shows in the output.  x, packed, bias, residual and out sit at 16-byte-aligned addresses 16 bytes into
    their allocations, the codes at an odd address."""
    nb = M * K // BS
    ng = -(-nb // 256)
    rng = np.random.default_rng(nb)
    q = rng.integers(0, 255, nb).astype(np.uint8)  # 0..254
    nested = (rng.random(ng) * 0.03 + 0.01).astype(np.float32)
    code = table().copy()
    code[255] = np.inf
    offset = 0.0173
    A = to_dev(N.unnest(q, nested, code, offset, 256))
    assert bool(torch.isfinite(A).all())
    pad = 4099
    qbig = torch.full((nb + 2 * pad,), 255, dtype=torch.uint8, device=dev())
    qbig[pad:pad + nb] = to_dev(q)
    nbig = torch.full((ng + 64,), float("nan"), device=dev())
    nbig[32:32 + ng] = to_dev(nested)
    qd, nd, cd = qbig[pad:pad + nb], nbig[32:32 + ng], to_dev(code)
    assert qd.data_ptr() % 2 == 1 and nd.data_ptr() % 16 == 0

    def shifted(t):  # the same values 16 bytes into a fresh allocation
        n = 16 // t.element_size()
        buf = torch.empty(t.numel() + n, dtype=t.dtype, device=t.device)
        buf[n:] = t.reshape(-1)
        return buf[n:].view(t.shape)

    g = torch.Generator(device=dev()).manual_seed(M + K)
    P = torch.randint(0, 256, (M * K // 2,), dtype=torch.uint8, device=dev(), generator=g)
    for dtype in DT16:
        x, b, r = rand((rows, K), dtype, rows, 0.5), rand(M, dtype, M, 0.1), rand((rows, M), dtype, 7)
        want = gemm_fused(x, P, A, M, K, BS, b, r)
        assert bool(torch.isfinite(want.float()).all())
        buf, out = guarded(rows * M + 8, dtype)
        got = gemm_nested(shifted(x), shifted(P), qd, nd, cd, offset, M, K, shifted(b), shifted(r), out=out[8:].view(rows, M))
        assert guards_intact(buf, rows * M + 8) and untouched(buf, 64, 72)
        assert torch.equal(got, want), (dtype, int((got != want).sum()))
        if rows <= 64:
            lA, lB, scale = adapter(M, K, 8, dtype, 5)
            t = down(x, lA, scale)
            got = gemm_lora_nested(shifted(x), shifted(P), qd, nd, cd, offset, M, K, shifted(lB), shifted(t), shifted(b), shifted(r))
            assert torch.equal(got, gemm_lora(x, P, A, M, K, lB, t, BS, b, r))
        if rows == 1:
            got = gemv_lora_nested(shifted(x), shifted(P), qd, nd, cd, offset, M, K, shifted(lB), shifted(t), shifted(b), shifted(r))
            assert torch.equal(got.reshape(1, M), gemv_lora(x, P, A, M, K, lB, t, BS, b, r).reshape(1, M))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_poisoned_out_untouched():
    M, K, rows = 32, 512, 8
    P, q, nested, offset, A = nested_weight(M, K)
    code = table_dev()
    x = rand((rows, K + 8), torch.bfloat16, 1).reshape(-1)
    x8 = x[:rows * K].view(rows, K)
    lA, lB, scale = adapter(M, K, 8, torch.bfloat16, 2)
    t = down(x8, lA, scale)
    buf, out = guarded(129 * M, torch.bfloat16)
    U, I = hipabi.ERR_UNSUPPORTED, hipabi.ERR_INVALID
    gemm = lambda **kw: gemm_nested(kw.pop("x", x8), kw.pop("P", P), kw.pop("q", q), kw.pop("nested", nested), kw.pop("code", code), offset,
                                    kw.pop("M", M), kw.pop("K", K), out=out, expect_ok=False, B=kw.pop("B", rows),
                                    dtype=kw.pop("dtype", torch.bfloat16), **kw)
    glora = lambda **kw: gemm_lora_nested(kw.pop("x", x8), kw.pop("P", P), kw.pop("q", q), kw.pop("nested", nested), kw.pop("code", code),
                                          offset, kw.pop("M", M), kw.pop("K", K), kw.pop("lB", lB), kw.pop("t", t), out=out, expect_ok=False,
                                          B=kw.pop("B", rows), dtype=kw.pop("dtype", torch.bfloat16), **kw)
    vlora = lambda **kw: gemv_lora_nested(kw.pop("x", x8[0]), kw.pop("P", P), kw.pop("q", q), kw.pop("nested", nested), kw.pop("code", code),
                                          offset, kw.pop("M", M), kw.pop("K", K), kw.pop("lB", lB), kw.pop("t", t), out=out, expect_ok=False,
                                          dtype=kw.pop("dtype", torch.bfloat16), **kw)
    twins = ((gemm, "fp4_hip_gemm_fused_nf4"), (glora, "fp4_hip_gemm_lora_nf4"), (vlora, "fp4_hip_gemv_lora_nf4"))
    for call, twin in twins:
        for g in (64, 128, 512):
            assert call(g=g) == U
            assert "nested_blocksize" in hipabi.last_error() and "fp4_hip_absmax_unnest" in hipabi.last_error() and twin in hipabi.last_error()
        for g in (0, -256):
            assert call(g=g) == I and "nested_blocksize" in hipabi.last_error()
        for null in ("x", "P", "q", "nested", "code"):
            assert call(**{null: None}) == I and "null" in hipabi.last_error(), (twin, null)
        assert call(x=x[1:1 + K] if call is vlora else x[1:1 + rows * K].view(rows, K)) == U  # x not 16-byte aligned
        assert call(epilogue=7) == I
        assert call(M=M - 1, epilogue=GATED) == I and "even row count" in hipabi.last_error()
        assert call(M=0) == hipabi.OK
    for call in (gemm, glora):
        assert call(bs=32) == U and "not covered" in hipabi.last_error()
        assert call(K=480) == U and call(K=96) == U  # K % 64 != 0
        assert call(dtype=torch.float32) == U
        assert call(B=0) == hipabi.OK
    assert gemm(B=129) == U and "not covered" in hipabi.last_error()
    assert glora(B=65) == U and "not covered" in hipabi.last_error()
    assert glora(Rr=12) == U and vlora(Rr=12) == U and glora(lB=None, Rr=8) == I and vlora(t=None) == I
    assert vlora(K=496, bs=16) == U and "not available" in hipabi.last_error()
    assert vlora(dtype=torch.float32, epilogue=GATED) == U
    torch.cuda.synchronize()
    assert untouched(buf)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def test_captured_calls_follow_an_in_place_change_of_x():
    M, K = 34, 1024
    P, q, nested, offset, A = nested_weight(M, K)
    code = table_dev()
    for dtype in DT16:
        lA, lB, scale = adapter(M, K, 8, dtype, 1)
        for rows in (1, 8, 40):  # the GEMV with the adapter (and one row of the small kernel), the small kernel, the wide one
            x, r = rand((rows, K), dtype, rows, 0.5), rand((rows, M), dtype, 3)
            out, out_l, t = torch.empty_like(r), torch.empty_like(r), torch.empty(rows, 8, device=dev())
            lora_nested, lora_twin = (gemv_lora_nested, gemv_lora) if rows == 1 else (gemm_lora_nested, gemm_lora)
            step = lambda: (gemm_nested(x, P, q, nested, code, offset, M, K, None, r, out=out), down(x, lA, scale, t),
                            lora_nested(x, P, q, nested, code, offset, M, K, lB, t, None, r, out=out_l))
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()  # warm-up: the code objects are loaded before the capture
                side.synchronize()
                with torch.cuda.graph(graph, stream=side):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            x.copy_(rand((rows, K), dtype, rows + 100, 0.5))  # in place: the captured calls read the new values
            out.zero_(), out_l.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, gemm_fused(x, P, A, M, K, BS, None, r)), (dtype, rows)
            assert torch.equal(out_l, lora_twin(x, P, A, M, K, lB, down(x, lA, scale), BS, None, r).reshape(rows, M)), (dtype, rows)


# ---- LoRA ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", FC.GEMV_VARIANT_SHAPES, ids=[f"{m}x{k}" for m, k in FC.GEMV_VARIANT_SHAPES])
def test_gemv_lora_nested_equals_the_lora_gemv_on_the_expanded_absmax(M, K):
    bs = bs_of(K)
    P, q, nested, offset, A = nested_weight(M, K, 0.0237, bs)
    code = table_dev()
    for variant in (0, 1):
        hipabi.set_variant("gemv_nf4", variant)
        for dtype in DT16 + [torch.float32]:
            x, b, r = rand(K, dtype, K), rand(M, dtype, M, 0.1), rand(M, dtype, M + 1)
            for Rr in NB.LORA_RANKS:
                lA, lB, scale = adapter(M, K, Rr, dtype, Rr)
                t = down(x, lA, scale)
                for bias, res in ((None, None), (b, r)):
                    got = gemv_lora_nested(x, P, q, nested, code, offset, M, K, lB, t, bias, res, bs=bs)
                    want = gemv_lora(x, P, A, M, K, lB, t, bs, bias, res)
                    assert torch.equal(got, want), (variant, dtype, Rr, bias is not None, int((got != want).sum()))
                if dtype != torch.float32:
                    rh = r[: M // 2].contiguous()
                    buf, out = guarded(M // 2, dtype)
                    got = gemv_lora_nested(x, P, q, nested, code, offset, M, K, lB, t, b, rh, GATED, out=out, bs=bs)
                    assert guards_intact(buf, M // 2)
                    assert torch.equal(got, gemv_lora(x, P, A, M, K, lB, t, bs, b, rh, GATED)), (variant, dtype, Rr, "gated")
            h = r.clone()  # in place: the residual aliases out
            gemv_lora_nested(x, P, q, nested, code, offset, M, K, lB, t, b, h, out=h, bs=bs)
            assert torch.equal(h, gemv_lora(x, P, A, M, K, lB, t, bs, b, r))


@pytest.mark.parametrize("M,K", NB.LORA_SHAPES, ids=[f"{m}x{k}" for m, k in NB.LORA_SHAPES])
def test_gemm_lora_nested_equals_the_lora_gemm_on_the_expanded_absmax(M, K):
    P, q, nested, offset, A = nested_weight(M, K)
    code = table_dev()
    for dtype in DT16:
        b = rand(M, dtype, M, 0.1)
        for rows in NB.LORA_ROWS:
            x, r, rh = rand((rows, K), dtype, rows, 0.5), rand((rows, M), dtype, 5), rand((rows, M // 2), dtype, 6)
            for Rr in NB.LORA_RANKS:
                lA, lB, scale = adapter(M, K, Rr, dtype, Rr + rows)
                t = down(x, lA, scale)
                for bias, res, epi in ((None, None, NONE), (b, r, NONE), (None, None, GATED), (b, rh, GATED)):
                    n = rows * (M // 2 if epi == GATED else M)
                    buf, out = guarded(n, dtype)
                    got = gemm_lora_nested(x, P, q, nested, code, offset, M, K, lB, t, bias, res, epi, out=out.view(rows, -1))
                    want = gemm_lora(x, P, A, M, K, lB, t, BS, bias, res, epi)
                    assert guards_intact(buf, n)
                    assert torch.equal(got, want), (dtype, rows, Rr, epi, bias is not None, int((got != want).sum()))
            h = r.clone()
            gemm_lora_nested(x, P, q, nested, code, offset, M, K, lB, t, b, h, out=h)
            assert torch.equal(h, gemm_lora(x, P, A, M, K, lB, t, BS, b, r))


# ---- torch ops -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16, ids=str)
def test_torch_ops_equal_the_c_abi_bit_for_bit(dtype):
    import torch_bnb_fp4 as pkg

    for M, K in ((34, 1024), (34, 320)):
        P, q, nested, offset, A = nested_weight(M, K)
        Bt, code = P.reshape(-1, 1).t(), table_dev()
        b = rand(M, dtype, M, 0.1)
        lA, lB, scale = adapter(M, K, 24, dtype, 4)
        for rows in (2, 16, 40, 64, 65, 128):
            x = rand((rows, K), dtype, rows, 0.5)
            for epi in (NONE, GATED):
                r = rand((rows, M // 2 if epi == GATED else M), dtype, 9)
                got = pkg.ext.gemm_nf4_nested(x, Bt, q, nested, code, offset, 256, BS, [M, K], b, r, epi)
                assert torch.equal(got, gemm_nested(x, P, q, nested, code, offset, M, K, b, r, epi)) and got.shape == r.shape
                if rows <= 64:
                    t = pkg.ext.lora_down(x, lA, scale)
                    got = pkg.ext.gemm_nf4_lora_nested(x, Bt, q, nested, code, offset, 256, BS, [M, K], b, r, epi, lB, t)
                    assert torch.equal(got, gemm_lora_nested(x, P, q, nested, code, offset, M, K, lB, t, b, r, epi))
        x3 = rand((2, 4, K), dtype, 3, 0.5)
        assert pkg.ext.gemm_nf4_nested(x3, Bt, q, nested, code, offset, 256, BS, [M, K], None, None, NONE).shape == (2, 4, M)
        x1 = rand((1, K), dtype, 1, 0.5)
        t1 = pkg.ext.lora_down(x1, lA, scale)
        for epi in (NONE, GATED):
            r = rand((1, M // 2 if epi == GATED else M), dtype, 9)
            got = pkg.ext.gemv_nf4_lora_nested(x1, Bt, q, nested, code, offset, 256, BS, [M, K], b, r, epi, lB, t1)
            want = gemv_lora_nested(x1.reshape(-1), P, q, nested, code, offset, M, K, lB, t1, b, r.reshape(-1), epi)
            assert torch.equal(got, want.reshape(1, -1))
        with pytest.raises(RuntimeError, match="nested_blocksize"):
            pkg.ext.gemm_nf4_nested(x1.expand(2, K).contiguous(), Bt, q, torch.cat([nested] * 4), code, offset, 64, BS, [M, K], None, None, NONE)
        with pytest.raises(RuntimeError, match="not covered"):
            pkg.ext.gemm_nf4_lora_nested(rand((65, K), dtype, 1), Bt, q, nested, code, offset, 256, BS, [M, K], None, None, NONE, lB,
                                         torch.zeros(65, 24, device=dev()))


# ---- what the ops refuse before they launch: the mistake table of tests/test_gpu_ext_checks.py over the three new ops ------------------
from test_gpu_ext_checks import M as M_OPS, NESTED as NESTED_ORDER, Op, rows_of  # noqa: E402


class NestedOp(Op):
    """An op of the extension that takes the compressed statistics in absmax's place; operands as Op.operands makes them for
    gemv_nf4_nested, for every row count."""

    @functools.lru_cache(maxsize=None)
    def operands(self):
        K, rows = self.K, self.rows
        P, q, nested, offset, _ = nested_weight(M_OPS, K)
        a = dict(absmax_u8=q, nested_absmax=nested, code=table_dev(), offset=offset, nested_blocksize=256, A=rand((rows, K), torch.bfloat16, 5 + rows, 2.0),
                 B=P.reshape(-1, 1).t(), P=P, blocksize=BS, Bshape=[M_OPS, K], bias=rand(M_OPS, torch.bfloat16, 7, 0.1),
                 residual=rand((rows, M_OPS), torch.bfloat16, 9), epilogue=NONE)
        if "lora_B" in self.order:
            lA, a["lora_B"], scale = adapter(M_OPS, K, 8, torch.bfloat16, 11)
            a["t"] = down(a["A"], lA, scale)
        return a


_stats = lambda a: (a["P"], a["absmax_u8"], a["nested_absmax"], a["code"], a["offset"], M_OPS, a["Bshape"][1])  # noqa: E731
_SHORT = {"absmax one scale short": "absmax_u8 holds"}
NESTED_OPS = [
    NestedOp("gemm_nf4_nested", NESTED_ORDER, 1024, 4, 128,
             lambda a: gemm_nested(a["A"], *_stats(a), a["bias"], a["residual"], a["epilogue"]), _SHORT, absmax="absmax_u8"),
    NestedOp("gemm_nf4_lora_nested", NESTED_ORDER + ("lora_B", "t"), 1024, 4, 128,
             lambda a: gemm_lora_nested(a["A"], *_stats(a), a["lora_B"], a["t"], a["bias"], a["residual"], a["epilogue"]), _SHORT,
             absmax="absmax_u8"),
    NestedOp("gemv_nf4_lora_nested", NESTED_ORDER + ("lora_B", "t"), 1024, 1, 1,
             lambda a: gemv_lora_nested(a["A"].reshape(-1), *_stats(a), a["lora_B"], a["t"], a["bias"], a["residual"].reshape(-1),
                                        a["epilogue"]).reshape(1, -1), _SHORT, absmax="absmax_u8"),
]


@pytest.mark.parametrize("op", NESTED_OPS, ids=repr)
def test_every_operand_mistake_is_refused_and_good_operands_reach_the_c_abi_untouched(op):
    """test_gpu_ext_checks.py's item, row for row: non-contiguous A, a CPU tensor, int8 / short B, statistics one code short, a wrong
    last dim, rows over the limit, bias of the wrong size / dtype, residual numel, unknown epilogue; then valid calls, both epilogues."""
    good = op.operands()
    before = {k: v.clone() for k, v in good.items() if torch.is_tensor(v)}
    seen = 0
    for mistake, make, exc, substring in rows_of(op):
        with pytest.raises(exc) as info:
            op(make(op, dict(good)))
        assert substring in str(info.value), (op, mistake, substring, str(info.value))
        seen += 1
    assert seen == 11, (op, seen)  # every row of the table applies to these ops but one of the two row-count rows
    extra = {"nested_absmax one group short": (dict(good, nested_absmax=good["nested_absmax"][:-1]), "group scales"),
             "a 255-entry table": (dict(good, code=good["code"][:-1]), "256 entries"),
             "int8 codes": (dict(good, absmax_u8=good["absmax_u8"].view(torch.int8)), "uint8"),
             "statistics on the CPU": (dict(good, nested_absmax=good["nested_absmax"].cpu()), "CUDA")}
    if "lora_B" in op.order:
        extra["lora_B of m - 1 rows"] = (dict(good, lora_B=good["lora_B"][:-1]), "lora_B must")
        extra["t of the wrong numel"] = (dict(good, t=good["t"].reshape(-1)[:-1]), "t must hold")
    for mistake, (bad, substring) in extra.items():
        with pytest.raises(RuntimeError) as info:
            op(bad)
        assert substring in str(info.value), (op, mistake, str(info.value))
    for epilogue in (NONE, GATED):
        a = dict(good, epilogue=epilogue, residual=good["residual"][:, :M_OPS // 2].contiguous() if epilogue == GATED else good["residual"])
        got = op(a)
        assert torch.equal(got, op.reference(a).reshape(got.shape)), (op, epilogue)
        assert got.shape == (op.rows, M_OPS // 2 if epilogue == GATED else M_OPS)
    assert all(torch.equal(good[k], v) for k, v in before.items())


CROSS = [(op, name) for op in NESTED_OPS for name in ("B", "absmax_u8", "bias", "residual") + (("lora_B", "t") if "lora_B" in op.order else ())]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU to put an operand on")
@pytest.mark.parametrize("op,name", CROSS, ids=[f"{op}-{name}" for op, name in CROSS])
def test_an_operand_on_another_device_is_refused(op, name):
    good = op.operands()
    with pytest.raises(RuntimeError, match="device"):
        op(dict(good, **{name: good[name].to(torch.device("cuda", 1))}))


# ---- modules ---------------------------------------------------------------------------------------------------------------------------
class _MLP(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = nn.Linear(H, I, bias=False), nn.Linear(H, I, bias=False), nn.Linear(I, H)
        self.act_fn = nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class _Net(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.mlp = _MLP(H, I)

    def forward(self, x):
        return self.mlp(x)


H, I = 512, 768
PROJECTIONS = ("gate_proj", "up_proj", "down_proj")


@pytest.fixture(scope="module")
def nested_file(tmp_path_factory):
    """A double-quantised NF4 checkpoint written by save_fp4_model(nested=True) from a freshly quantised toy net."""
    import torch_bnb_fp4 as pkg

    torch.manual_seed(5)
    net = pkg.recursively_replace_with_fp4_linear(_Net(H, I).to(torch.bfloat16), as_dtype=torch.bfloat16, device=dev(), quant_type="nf4")
    path = str(tmp_path_factory.mktemp("nested_batch") / "model.safetensors")
    pkg.save_fp4_model(net, path, nested=True)
    return path


def _load(path, resident):
    import torch_bnb_fp4 as pkg

    return pkg.load_fp4_layers(_Net(H, I).to(torch.bfloat16), path, device=dev(), nested="resident" if resident else "expand")


def test_resident_layers_under_the_switch_equal_the_expanded_ones_under_the_same_switch(nested_file):
    import torch_bnb_fp4 as pkg

    resident, expanded = _load(nested_file, True), _load(nested_file, False)
    default = _load(nested_file, False)
    layers = lambda m: [getattr(m.mlp, n) for n in PROJECTIONS]
    assert all(type(l) is pkg.NestedNF4Linear for l in layers(resident))

    def compare(other, rows_list):
        for name, res, exp in zip(PROJECTIONS, layers(resident), layers(other)):
            for rows in rows_list:
                x, r = rand((rows, res.in_features), torch.bfloat16, rows, 0.5), rand((rows, res.out_features), torch.bfloat16, rows + 1)
                assert torch.equal(res(x), exp(x)), (name, rows)
                assert torch.equal(res(x, r), exp(x) + r), (name, rows, "residual")

    # the switch off: nothing existing moved
    compare(default, (2, 16, 24, 64, 65))
    assert pkg.set_small_batch_fused(resident, True, nf4=True, nf4_wide=True) == pkg.set_small_batch_fused(expanded, True, nf4=True, nf4_wide=True) == 3
    calls = []
    real = pkg.nested.ext.gemm_nf4_nested
    try:
        pkg.nested.ext.gemm_nf4_nested = lambda *a: (calls.append(a[0].shape[0]), real(*a))[1]
        compare(expanded, (2, 16, 24, 64))
        assert sorted(set(calls)) == [2, 16, 24, 64] and len(calls) == 3 * 4 * 2  # every call went through the nested op
        compare(expanded, (65,))  # both fall back and agree
        compare(default, (65,))
        assert len(calls) == 24
    finally:
        pkg.nested.ext.gemm_nf4_nested = real
    x3 = rand((2, 4, H), torch.bfloat16, 3, 0.5)
    assert torch.equal(resident.mlp.gate_proj(x3), expanded.mlp.gate_proj(x3)) and resident.mlp.gate_proj(x3).shape == (2, 4, I)
    h = rand((16, H), torch.bfloat16, 8, 0.5)
    assert torch.equal(resident(h), expanded(h))
    step = pkg.GraphedStep(lambda t: resident(t), h)
    for scale in (1.0, -0.5):
        assert torch.equal(step(h * scale), resident(h * scale))
    assert pkg.fuse_gated_mlps(resident, nf4=True) == 0  # compressed groups span rows: still not recognised


def test_attach_lora_on_a_resident_model_equals_attach_lora_on_the_expanded_one(nested_file):
    import torch_bnb_fp4 as pkg

    resident, expanded = _load(nested_file, True), _load(nested_file, False)
    g = torch.Generator().manual_seed(4)
    r = 12  # padded to 16
    state = {}
    for name, (M, K) in (("mlp.gate_proj", (I, H)), ("mlp.up_proj", (I, H)), ("mlp.down_proj", (H, I))):
        state[f"base_model.model.{name}.lora_A.weight"] = torch.randn(r, K, generator=g) / K**0.5
        state[f"base_model.model.{name}.lora_B.weight"] = torch.randn(M, r, generator=g) * 0.05
    assert pkg.attach_lora(resident, state, r=r, lora_alpha=24) == pkg.attach_lora(expanded, state, r=r, lora_alpha=24) == 3
    for name in PROJECTIONS:
        assert type(getattr(resident.mlp, name)) is pkg.LoRANestedNF4Linear and type(getattr(expanded.mlp, name)) is pkg.LoRANF4Linear
        assert getattr(resident.mlp, name).absmax_u8.dtype == torch.uint8
    for rows in (1, 8):
        h = rand((rows, H), torch.bfloat16, rows, 0.5)
        y = resident(h)
        assert y.shape == (rows, H) and bool(torch.isfinite(y.float()).all())
        assert torch.equal(y, expanded(h)), rows
        x, res = rand((rows, I), torch.bfloat16, rows + 2, 0.5), rand((rows, H), torch.bfloat16, rows + 3)
        assert torch.equal(resident.mlp.down_proj(x, res), expanded.mlp.down_proj(x, res)), (rows, "residual")
    # the adapter changes the output (the comparison above is not of two bare models)
    bare = _load(nested_file, True)
    h = rand((8, H), torch.bfloat16, 8, 0.5)
    assert not torch.equal(bare(h), resident(h))
    step = pkg.GraphedStep(lambda t: resident(t), h)
    for scale in (1.0, -0.5):
        assert torch.equal(step(h * scale), resident(h * scale))
    # 65 rows: the base through the layer's own path, the adapter in torch - as the expanded layer's fallback does
    h65 = rand((65, H), torch.bfloat16, 65, 0.5)
    y65 = resident(h65)
    assert y65.shape == (65, H) and bool(torch.isfinite(y65.float()).all())
    assert torch.equal(y65, expanded(h65))  # LoRANF4Linear._adapter_in_torch over dequant + GEMM: the same bits
    x65, r65 = rand((65, I), torch.bfloat16, 66, 0.5), rand((65, H), torch.bfloat16, 67)
    assert torch.equal(resident.mlp.down_proj(x65, r65), expanded.mlp.down_proj(x65, r65))
