"""fp4_hip_gemm_small / _fused / _ws at the tall weights their dispatch thresholds key on (tests/fp4_batch_cases.py: both sides of
every threshold, the decode workload's own shapes), with the compute-unit count taken from the device.

Per weight shape, built once: random packed bytes and positive scales drawn on the device, x ~ N(0, 1) rounded to bf16 and fp16, a
bias on every other shape.  Checker: the float64 product of the WHOLE weight with all rows, and |W| |x|, formed on the device by the
pure-torch oracle (oracle/torch_cpu.py) in row chunks, tied to the C oracle (c_oracle.gemv_f64) on the first 8, the last 8 and 48
random weight rows for the first and the last activation row.  Bar of test_gpu_gemv.py on every output element:
|y - y*| <= ulp_T(y*)/2 * 1.01 + 1e-5 * sum |x w|.

* values: the default call AND every cell that can be forced on the shape (fp4_batch_cases.legal_cells: each kernel family in each
  row-tile / ring / staging form) meet the bar - the forced geometries run on the multi-round grid, not only the predicted one;
* route: the default call's bits are the bits of forced(cell(...)) of the restated dispatcher; per threshold, on the probe shape,
  the forced outputs of the two neighbouring cells differ in at least one element (either dtype) unless the pair is exempt
  (fp4_batch_cases.EXEMPT: one K partition and summation order, no difference possible) - then the two outputs must be bit-identical;
* split-K: fp4_hip_gemm_small_ws_bytes equals the restatement, the workspace is exactly as large as asked and sits, like the output,
  between sentinel guards, two runs give the same bits;
* epilogues on the workload's tall shape: residual bit-exact against oracle.linear_epilogue of the plain result, gate|up within 1 ulp
  of torch's silu(g) * u, >= 99.8 % identical (the rule of test_gpu_fused.test_small_batch_epilogues);
* one layer above: ext.gemm_small_fp4 / _fused and a TorchFP4Linear with small_batch_fused are the C ABI bit for bit."""
import numpy as np
import pytest
import torch

import fp4_batch_cases as C
import fp4_constructed as FC
import hipabi
from gpu_util import HALF_ULP, NPDT, dev
from oracle import c_oracle, fp4_oracle as o, torch_cpu

pytestmark = pytest.mark.gpu
BS = 64
DT16 = [torch.bfloat16, torch.float16]
NONE, GATED = hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS
SHAPES = C.SHAPES()
WS_GUARD = 1 << 16  # bytes on either side of the workspace (a multiple of 16: the view keeps the alignment the kernels ask for)


def cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def _random_fp4(n_elems, seed):
    """Random packed bytes + positive scales on the device (as tests/test_gpu_dispatch_table.py: any byte pattern is a valid FP4
    weight, -0 and the 1/192 code included)."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    packed = torch.randint(0, 256, (n_elems // 2,), dtype=torch.uint8, device=dev(), generator=g)
    absmax = torch.rand(n_elems // BS, device=dev(), generator=g) * 0.05 + 0.005
    return packed, absmax


def _rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(shape, device=dev(), generator=g) * scale).to(dtype)


def _device_f64_product(packed_d, absmax_d, x64_d, M, K, table_d, magnitudes=False):
    """W @ X in float64 for the whole weight and a [K, n] right-hand side, by the pure-torch oracle on the device, in row chunks of
    <= 32 Mi elements.  Returns [n, M]."""
    out = torch.empty(M, x64_d.shape[1], dtype=torch.float64, device=dev())
    step = max(1, (1 << 25) // K)
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        p = packed_d[r0 * K // 2:r1 * K // 2]
        if magnitudes:
            p = p & 0x77
        w = torch_cpu.dequantize(p, absmax_d[r0 * K // BS:r1 * K // BS], r1 - r0, K, BS, torch.float32, table_d)
        out[r0:r1] = w.double() @ x64_d
    return out.t().contiguous()


def _tie_to_the_c_oracle(packed_d, absmax_d, M, K, x64_d, exact_d, scale_d, seed):
    """The device-side evaluation against c_oracle.gemv_f64 on the first 8, the last 8 and 48 random weight rows, for the first and
    the last column of the right-hand side."""
    rng = np.random.default_rng(seed)
    rows = np.unique(np.concatenate([np.arange(min(8, M)), np.arange(max(0, M - 8), M), rng.integers(0, M, 48)]))
    rows_d = torch.from_numpy(rows).to(dev())
    p_rows = packed_d.view(M, K // 2)[rows_d].cpu().numpy().reshape(-1)
    a_rows = absmax_d.view(M, K // BS)[rows_d].cpu().numpy().reshape(-1)
    for col in (0, x64_d.shape[1] - 1):
        xv = x64_d[:, col].cpu().numpy()
        want = c_oracle.gemv_f64(xv, p_rows, a_rows, len(rows), K, BS)
        assert np.allclose(exact_d[col, rows_d].cpu().numpy(), want, rtol=1e-11, atol=1e-13), (M, K, col)
        want = c_oracle.gemv_f64(np.abs(xv), p_rows & 0x77, a_rows, len(rows), K, BS)
        assert np.allclose(scale_d[col, rows_d].cpu().numpy(), want, rtol=1e-11, atol=1e-13), (M, K, col)


class Weight:
    """One weight with its activations and float64 answers, built once per shape: x[dtype] [rows, K], bias[dtype] (or None),
    exact[dtype] and scale[dtype] [rows, M] (bias included, as gpu_util.Case.rows does)."""

    def __init__(self, M, K, rows, with_bias, seed):
        self.M, self.K = M, K
        self.P, self.A = _random_fp4(M * K, seed)
        table_d = torch_cpu.code_table("codebook").to(dev())
        x32 = _rand((rows, K), torch.float32, seed + 1)
        self.x = {dt: x32.to(dt) for dt in DT16}
        X = torch.cat([self.x[dt].double() for dt in DT16]).t().contiguous()  # [K, 2 * rows]
        exact = _device_f64_product(self.P, self.A, X, M, K, table_d)
        scale = _device_f64_product(self.P, self.A, X.abs(), M, K, table_d, magnitudes=True)
        _tie_to_the_c_oracle(self.P, self.A, M, K, X, exact, scale, seed)
        self.bias, self.exact, self.scale = {}, {}, {}
        for i, dt in enumerate(DT16):
            b = _rand((M,), dt, seed + 2, 0.1) if with_bias else None
            self.bias[dt] = b
            self.exact[dt] = exact[i * rows:(i + 1) * rows] + (b.double() if with_bias else 0.0)
            self.scale[dt] = scale[i * rows:(i + 1) * rows] + (b.double().abs() if with_bias else 0.0)

    def ratio(self, y, dt, b0=0):
        """(worst |err| / tol, elements outside the bar) of an output for the activation rows b0 .. b0 + rows(y) - 1."""
        e, s = self.exact[dt][b0:b0 + y.shape[0]], self.scale[dt][b0:b0 + y.shape[0]]
        tol = HALF_ULP[dt] * 1.01 * e.abs() + 1e-5 * s + 1e-30
        err = (y.double() - e).abs()
        return float((err / tol).max()), int((~(err <= tol)).sum())  # (a NaN is outside the bar)

    def run(self, dt, B, settings=None, b0=0, residual=None, epilogue=NONE, bias=True):
        """fp4_hip_gemm_small (or _fused, for an epilogue) on rows b0 .. b0 + B - 1 under the given fp4_hip_set_variant settings, into
        an output filled with a sentinel (an element no workgroup stores must not pass as the previous call's)."""
        x = self.x[dt][b0:b0 + B]
        b = self.bias[dt] if bias else None
        out = torch.full((B, self.M // 2 if epilogue == GATED else self.M), FC.SENTINEL16, dtype=torch.int16, device=dev()).view(dt)
        try:
            for kernel, v in (settings or {}).items():
                hipabi.set_variant(kernel, v)
            if residual is None and epilogue == NONE:
                return hipabi.gemm_small(x, self.P, self.A, self.M, self.K, BS, bias=b, out=out)
            return hipabi.gemm_small_fused(x, self.P, self.A, self.M, self.K, BS, b, residual, epilogue, out=out)
        finally:
            hipabi.set_variant("gemm_small", -1)
            hipabi.set_variant("gemm_wide", -1)


def _name(c):
    return "-".join(str(v) for v in c)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ulps(a, b):
    def line(t):
        v = _bits(t).to(torch.int32) & 0xFFFF
        return torch.where(v >= 0x8000, 0x8000 - v, v)
    return (line(a) - line(b)).abs()


def _as_np(t):
    return t.float().cpu().numpy()


def _report(what, worst):
    for key, r in worst.items():
        print(f"fp4-batch {what} {key}: worst |err| / tol = {r:.3f}")


@pytest.mark.parametrize("s", SHAPES, ids=[C.shape_id(s) for s in SHAPES])
def test_tall_shapes_by_heuristic_and_forced(s):
    n_cu = cus()
    M, K = C.rows_of(s.m, n_cu), s.K
    index = SHAPES.index(s)
    w = Weight(M, K, max(s.Bs + s.ws_Bs), with_bias=index % 2 == 1, seed=1000003 * M + K)
    worst = {}

    def within_bar(y, dt, key, b0=0):
        r, bad = w.ratio(y, dt, b0)
        worst[key] = max(worst.get(key, 0.0), r)
        assert bad == 0, (C.shape_id(s), M, K, dt, key, bad, r)

    for B in s.Bs:
        launches = C.cells(B, M, K, n_cu)
        rows = C.chunks(B, 64) if B > 64 else [B]
        assert len(launches) == len(rows)
        for dt in DT16:
            # the default dispatch: inside the bar, and the bits of the restated cell forced from outside
            y = w.run(dt, B)
            within_bar(y, dt, f"B={B} default={'+'.join(_name(c) for c in launches)}")
            b0 = 0
            for c, n in zip(launches, rows):
                forced = w.run(dt, n, C.forced(c, n), b0)
                assert torch.equal(_bits(y[b0:b0 + n]), _bits(forced)), (C.shape_id(s), B, dt, c, "the route is not the restated one")
                b0 += n
            if B > 64:
                continue
            # every other geometry that can be forced on this shape
            for c in C.legal_cells(B, M, K, n_cu):
                within_bar(w.run(dt, B, C.forced(c, B)), dt, f"B={B} forced={_name(c)}")
            # 17..64 rows with the one-pass path declined: 16-row launches, each the cell the restatement names
            if B > 16 and s.m[0] == 0:
                off = {"gemm_wide": 0}
                y = w.run(dt, B, off)
                within_bar(y, dt, f"B={B} one-pass-declined")
                b0 = 0
                for c, n in zip(C.cells(B, M, K, n_cu, h=C.hooks_of(off)), C.chunks(B, 16)):
                    assert torch.equal(_bits(y[b0:b0 + n]), _bits(w.run(dt, n, C.forced(c, n), b0))), (C.shape_id(s), B, dt, c, b0)
                    b0 += n

    # calls that bring the workspace the library asks for
    for B in s.ws_Bs:
        want = hipabi.lib().fp4_hip_gemm_small_ws_bytes
        want.restype = hipabi.ctypes.c_int64
        want.argtypes = [hipabi.ctypes.c_int64] * 3 + [hipabi.ctypes.c_int] * 2
        for dt in DT16:
            asked = want(B, M, K, BS, hipabi.DT[dt])
            assert asked == C.ws_bytes(B, M, K, n_cu), (C.shape_id(s), B, asked)
            plain = w.run(dt, B)
            x, b = w.x[dt][:B], w.bias[dt]
            if asked == 0:  # past the threshold: the workspace entry is the plain one
                y, _ = hipabi.gemm_small_ws(x, w.P, w.A, M, K, BS, bias=b, workspace=torch.empty(1 << 20, dtype=torch.uint8, device=dev()))
                assert torch.equal(_bits(y), _bits(plain))
                continue
            c = C.cell(B, M, K, n_cu, True)
            assert c[0] == "splitk"
            ws_buf, ws = FC.guarded(asked, torch.uint8, WS_GUARD, dev())
            g = FC.guard_elems(M)
            out_buf, out = FC.guarded(B * M, dt, g, dev())
            assert ws.data_ptr() % 16 == 0 and ws.numel() == asked
            y, _ = hipabi.gemm_small_ws(x, w.P, w.A, M, K, BS, bias=b, workspace=ws, out=out.view(B, M))
            torch.cuda.synchronize()
            assert FC.guards_intact(ws_buf, asked, WS_GUARD) and FC.guards_intact(out_buf, B * M, g), (C.shape_id(s), B, dt)
            within_bar(y, dt, f"B={B} workspace={_name(c)}")
            first = y.clone()
            FC.refill(ws_buf)
            y2, _ = hipabi.gemm_small_ws(x, w.P, w.A, M, K, BS, bias=b, workspace=ws)
            assert torch.equal(_bits(first), _bits(y2)) and FC.guards_intact(ws_buf, asked, WS_GUARD)
            # the split-K path ran: its sum over K slices is not the one-pass kernel's, and among B * M outputs that shows
            differing = int((_bits(first) != _bits(plain)).sum())
            print(f"fp4-batch split-K {C.shape_id(s)} B={B} {dt}: differs from the one-pass kernel in {differing} of {B * M} elements")
            assert differing > 0, (C.shape_id(s), B, dt)

    # the thresholds this shape is a side of: the two neighbouring cells, forced on the probe side, must be distinguishable - or be
    # exempt, and then identical
    for t in C.THRESHOLDS:
        if t.K != K or s.m not in (t.lo, t.hi):
            continue
        for B in t.Bs:
            ws = t is C.WS_THRESHOLD
            lo, hi = C.cell(B, C.rows_of(t.lo, n_cu), K, n_cu, ws), C.cell(B, C.rows_of(t.hi, n_cu), K, n_cu, ws)
            if C.exempt(lo, hi) is not None:
                # one K partition and summation order: the list is held to its word, bit for bit, on either side of the threshold
                # (what the two settings run HERE, e.g. the 8-row x image only below its threshold, is the restatement's answer)
                ran = [C.cell(B, M, K, n_cu, h=C.hooks_of(C.forced(c, B))) for c in (lo, hi)]
                assert C.exempt(*ran) is not None or ran[0] == ran[1]
                for dt in DT16:
                    a, b = w.run(dt, B, C.forced(lo, B)), w.run(dt, B, C.forced(hi, B))
                    assert torch.equal(_bits(a), _bits(b)), (t.name, B, dt, ran, "listed as exempt, but the bits differ")
                print(f"fp4-batch threshold [{t.name}] B={B} at {C.shape_id(s)}: {_name(ran[0])} | {_name(ran[1])} exempt "
                      f"({C.exempt(lo, hi)[0]}), bit-identical")
                continue
            if s.m != getattr(t, t.probe):
                continue
            differing = 0
            for dt in DT16:
                if ws:  # the split-K side is the call with the workspace, the other side the same call without
                    a = hipabi.gemm_small_ws(w.x[dt][:B], w.P, w.A, M, K, BS, bias=w.bias[dt])[0]
                    b = w.run(dt, B)
                else:
                    a, b = w.run(dt, B, C.forced(lo, B)), w.run(dt, B, C.forced(hi, B))
                differing += int((_bits(a) != _bits(b)).sum())
            print(f"fp4-batch threshold [{t.name}] B={B}: {_name(lo)} | {_name(hi)} differ in {differing} of {2 * B * M} elements")
            assert differing > 0, (t.name, B, lo, hi, "the route test cannot tell these two cells apart")
    _report(C.shape_id(s), worst)
    del w
    torch.cuda.empty_cache()


@pytest.mark.parametrize("m,K", C.EPILOGUE_SHAPES, ids=[f"{C.m_id(m)}x{K}" for m, K in C.EPILOGUE_SHAPES])
def test_epilogues_on_the_tall_workload_shape(m, K):
    """The residual and the gate|up epilogue of every kernel family at the decode workload's gate|up shape: the default call at
    every row count, every forced cell at 8 and at 32 rows."""
    n_cu = cus()
    M = C.rows_of(m, n_cu)
    s = next(s for s in SHAPES if (s.m, s.K) == (m, K))
    w = Weight(M, K, max(s.Bs), with_bias=True, seed=1000003 * M + K + 5)
    for B in s.Bs:
        for dt in DT16:
            r = _rand((B, M), dt, 31 * B + 7)
            rh = r[:, : M // 2].contiguous()
            for settings in [None] + ([C.forced(c, B) for c in C.legal_cells(B, M, K, n_cu)] if B in (8, 32) else []):
                plain = w.run(dt, B, settings)
                got = w.run(dt, B, settings, residual=r)
                want = o.linear_epilogue(_as_np(plain), NPDT[dt], None, _as_np(r))
                assert np.array_equal(_as_np(got).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (B, dt, settings)
                ref = torch.nn.functional.silu(plain[:, 0::2]) * plain[:, 1::2]
                gu = w.run(dt, B, settings, epilogue=GATED)
                gur = w.run(dt, B, settings, residual=rh, epilogue=GATED)
                assert gu.shape == (B, M // 2)
                for a, b in ((gu, ref), (gur, ref + rh)):
                    d = _ulps(a, b)
                    same = float((d == 0).float().mean())
                    assert int(d.max()) <= 1 and same >= 0.998, (B, dt, settings, int(d.max()), same)
    del w
    torch.cuda.empty_cache()


def test_torch_ops_equal_the_c_abi_on_the_tall_shapes():
    """ext.gemm_small_fp4 / ext.gemm_small_fp4_fused at 14336 x 4096 x 8 rows and at (24 cus - 1) x 8192 x 33 rows, where the op brings
    the split-K workspace itself: the C ABI's bits, plain and with both epilogues."""
    import torch_bnb_fp4 as pkg

    n_cu = cus()
    for M, K, B in ((14336, 4096, 8), (24 * n_cu - 1, 8192, 33)):
        P, A = _random_fp4(M * K, M + K)
        asked = C.ws_bytes(B, M, K, n_cu)
        assert (asked > 0) == (B == 33)
        for dt in DT16:
            x, b = _rand((B, K), dt, B), _rand((M,), dt, 3, 0.1)
            got = pkg.ext.gemm_small_fp4(x, P.view(-1, 1).t(), A, BS, [M, K], b)
            want = hipabi.gemm_small_ws(x, P, A, M, K, BS, bias=b)[0] if asked else hipabi.gemm_small(x, P, A, M, K, BS, bias=b)
            assert got.shape == (B, M) and torch.equal(_bits(got), _bits(want)), (M, K, B, dt)
            for epi in (NONE, GATED):
                if epi == GATED and M % 2:
                    continue
                m_out = M // 2 if epi == GATED else M
                r = _rand((B, m_out), dt, 9)
                got = pkg.ext.gemm_small_fp4_fused(x, P.view(-1, 1).t(), A, BS, [M, K], b, r, epi)
                if asked:
                    want = hipabi.gemm_small_ws(x, P, A, M, K, BS, b, r, epi)[0]
                else:
                    want = hipabi.gemm_small_fused(x, P, A, M, K, BS, b, r, epi)
                assert got.shape == (B, m_out) and torch.equal(_bits(got), _bits(want)), (M, K, B, dt, epi)
        del P, A
    torch.cuda.empty_cache()


def test_a_layer_with_small_batch_fused_equals_the_c_abi_at_14336_x_4096():
    import torch_bnb_fp4 as pkg

    M, K = 14336, 4096
    torch.manual_seed(3)
    lin = torch.nn.Linear(K, M, device=dev())
    for dt in DT16:
        layer = pkg.TorchFP4Linear(pkg.swap_linear_with_bnb_linear(lin, dtype=dt).to(dev()))
        assert pkg.set_small_batch_fused(layer, True) == 1
        qd = layer.quant_data
        for B in (8, 32):
            x = _rand((B, K), dt, B + 1)
            with torch.inference_mode():
                y = layer(x)
            assert qd.bias.dtype == dt and y.shape == (B, M)
            want = hipabi.gemm_small(x, qd.A.reshape(-1), qd.absmax, M, K, BS, bias=qd.bias)
            assert torch.equal(_bits(y), _bits(want)), (dt, B)
        del layer
    torch.cuda.empty_cache()
