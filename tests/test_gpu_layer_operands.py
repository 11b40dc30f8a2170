"""The seam above the kernels: every layer class of the package, handed activations that were NOT freshly allocated, and FP4 layers
of block sizes the fused small-batch op does not take (tests/layer_operand_cases.py has the presentations, the recording proxy and the
sweep with its four assertions; tests/test_layer_operands_host.py runs the same sweep on the CPU doubles in strict mode).

Values.  Every output element is held to the project's bar against a float64 reference: the product of the dequantised weight
(oracle/torch_cpu.py; tests/nf4_ref.py for NF4; tests/nested_ref.py's expansion of the statistics for resident layers) plus the bias,
the adapter term in float64, and the residual.  The bar, 1.01 ulp_T(y*)/2 + 1e-5 sum |x w|, is the bar of ONE rounding, and a route
that rounds once is held to exactly it.  Some routes document more, e.g. the GEMV epilogue T(T(T(sum) + bias) + residual), and a
rounding of a partial sum is half an ulp of THAT partial sum, which a residual of the opposite sign leaves far above half an ulp of the
final y*: for those the half-ulp term is charged once per rounding the RECORDED route documents, each at its own partial sum
(Ref.__call__ lists the roundings per op family; profiles/layer_operands.txt states the deviation per route).  Dequant + GEMM
multiplies by the weight dequantised to the activation dtype, so a qlinear* route is held against that weight.  Gate|up outputs use
the suite's criterion for them (test_gpu_nf4_fused.assert_close_ulp at 0.999: at most one ulp from torch's silu * mul of the layer's
own plain rows, which are held to the bar above) on every call of 1000 elements or more; a layer here has 64 outputs a row, so a
smaller call has the one-ulp limit alone and the identical fraction of all calls of the sweep together is held to 0.999 as well.

Every sweep prints its records ("layer-operands | ..." lines; profiles/layer_operands.txt keeps them) and names every failing cell."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

import layer_operand_cases as L
import nested_ref as N
import nf4_ref as R4
from gpu_util import HALF_ULP, dev, to_dev
from oracle import c_oracle, fp4_oracle as o, torch_cpu
from test_gpu_nf4_fused import ulps

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT16 = [BF16, F16]
NONE, GATED = 0, 1
NESTED_OFFSET = 0.0237


def pkg():
    import torch_bnb_fp4

    return torch_bnb_fp4


@pytest.fixture()
def rec(monkeypatch):
    return L.install(monkeypatch, pkg().ext)


# ---- weights and float64 references ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight(kind, M, K, seed, bs=64):
    """(packed uint8 [M K / 2, 1] and f32 absmax on the device, the dequantised weight as float64 [M, K]); quantised by the oracles."""
    w = (np.random.default_rng(seed).standard_normal(M * K) * 0.05).astype(np.float32)
    if kind == "fp4":
        packed, am = c_oracle.quantize(w, bs) if bs == 64 else o.quantize_fp4(w, bs)
        w64 = torch_cpu.dequantize(torch.from_numpy(packed), torch.from_numpy(am), M, K, bs, torch.float32).double().numpy()
    else:
        packed, am = R4.quantize(w, bs)
        w64 = R4.dequantize_f32(packed, am, bs, M * K).reshape(M, K).astype(np.float64)
    return to_dev(packed).view(-1, 1), to_dev(am), w64


@functools.lru_cache(maxsize=None)
def nested_weight(M, K, seed):
    """An NF4 weight whose absmax is double-quantised by tests/nested_ref.py, and the float64 weight of the EXPANDED statistics."""
    w = (np.random.default_rng(seed).standard_normal(M * K) * 0.05).astype(np.float32)
    packed, am = R4.quantize(w, 64)
    table = N.dynamic_map()
    q, nested, _ = N.nest(am, NESTED_OFFSET, table, 256)
    expanded = N.unnest(q, nested, table, NESTED_OFFSET, 256)
    w64 = R4.dequantize_f32(packed, expanded, 64, M * K).reshape(M, K).astype(np.float64)
    return to_dev(packed).view(-1, 1), to_dev(q), to_dev(nested), to_dev(table), w64


def vector(n, seed, dtype, scale=0.1):
    return L.random(n, dtype, seed, dev(), scale)


def adapter(M, K, seed, dtype, rank=L.RANK):
    A = L.random((rank, K), dtype, seed, dev(), K ** -0.5)
    B = L.random((M, rank), dtype, seed + 1, dev(), 0.05)
    return A, B, 2.0


def f64(t):
    return t.detach().double().cpu().numpy()


class Ref:
    """x [n, K] -> (y* float64 [n, M], tol): see the module docstring.  ``adapters``: (A, B, scale) triples as the layer holds them."""

    def __init__(self, w64, bias=None, adapters=()):
        self.w, self.bias = w64, None if bias is None else f64(bias)
        self.adapters = [(f64(A), f64(B), float(s)) for A, B, s in adapters]
        self._rounded = {}

    def weight(self, dtype, route):
        """What the route multiplies by: the fused ops the f32 product code * absmax, dequant + GEMM that product rounded to T (the
        dequantised weight is a tensor of the activation dtype: oracle/torch_cpu.dequantize(..., dtype))."""
        if dtype == F32 or not any(op.startswith("qlinear") for op in L.ops(route)):
            return self.w
        if dtype not in self._rounded:  # the f32 products are exact in float64, so this is one rounding, torch's
            self._rounded[dtype] = torch.from_numpy(self.w.astype(np.float32)).to(dtype).double().numpy()
        return self._rounded[dtype]

    def __call__(self, x, residual=None, ids=None, dtype=None, route=()):
        """The half-ulp term is charged once per rounding the recorded route documents, at the partial sum that is rounded:
        * a GEMV op (gemv_*): T(T(T(sum [+ adapter]) + bias) + residual) - the bias is a rounding of its own, the fused adapter none;
        * a batched op (gemm_*) and dequant + GEMM (qlinear*): T(sum + bias [+ adapter]), F.linear's one rounding, then T(. + residual);
        * an adapter the route did not fuse (no *_lora* op) is added by torch to the rounded base and rounded again;
        * a residual is one more rounding wherever it is added (in the kernel or by torch: T(t + r) either way).
        A route that rounds once - no residual, and a bias only on a batched op - gets the project's bar itself."""
        w = self.weight(dtype, route)
        x = f64(x).reshape(-1, w.shape[1])
        names = [op for op in L.ops(route) if not op.startswith("lora_down")]
        gemv = bool(names) and names[-1].startswith("gemv_")
        adapter_fused = any("lora" in op for op in names)
        s = x @ w.T
        scale = np.abs(x) @ np.abs(w).T
        b = 0.0 if self.bias is None else self.bias
        if self.bias is not None:
            scale = scale + np.abs(self.bias)
        a = np.zeros_like(s)
        if self.adapters:
            ids = [0] * x.shape[0] if ids is None else ids
            ds = np.zeros_like(s)
            for row, i in enumerate(ids):
                if 0 <= i < len(self.adapters):
                    A, B, f = self.adapters[i]
                    a[row] = ((x[row] @ A.T) * f) @ B.T
                    ds[row] = ((np.abs(x[row]) @ np.abs(A).T) * abs(f)) @ np.abs(B).T
            scale = scale + ds
        fused_a = a if adapter_fused else 0.0
        if gemv:
            half = np.abs(s + fused_a)
            if self.bias is not None:
                half = half + np.abs(s + fused_a + b)
        else:
            half = np.abs(s + b + fused_a)
        y = s + b + a
        if self.adapters and not adapter_fused:
            half = half + np.abs(y)
        if residual is not None:
            y = y + f64(residual).reshape(y.shape)
            half = half + np.abs(y)
        return y, HALF_ULP[dtype] * 1.01 * half + 1e-5 * scale + 1e-30


def bar_check(ref, dtype, ids_of=None):
    def check(rows, x, res, y, route):
        exact, tol = ref(x, res, None if ids_of is None else ids_of(L.n_rows(rows)), dtype, route)
        err = np.abs(f64(y).reshape(exact.shape) - exact)
        ratio = float((err / tol).max())
        assert ratio <= 1.0, f"worst err/tol {ratio:.3f}"
        return ratio
    return check


class GatedCheck:
    """Gate|up: at most one ulp from torch's silu * mul of the layer's own plain rows (+ residual) on every call, identical on 99.9 % of
    the elements of every call that has 1000 or more and of the whole sweep; the plain rows - the same weight, bias and adapter behind
    the plain epilogue - are held to the bar."""

    def __init__(self, rec, plain_layer, plain_check):
        self.rec, self.plain, self.plain_check = rec, plain_layer, plain_check
        self.same = self.total = 0

    def __call__(self, rows, x, res, y, route):
        self.rec.take()
        p = self.plain(L.placed(x, "fresh"))
        ratio = self.plain_check(rows, x, None, p, self.rec.take())
        want = nn.functional.silu(p[..., 0::2]) * p[..., 1::2]
        if res is not None:
            want = want + res
        d = ulps(y, want)
        self.same += int((d == 0).sum())
        self.total += d.numel()
        assert int(d.max()) <= 1, f"{int(d.max())} ulp from silu * mul of the plain rows"
        same = float((d == 0).float().mean())
        assert d.numel() < 1000 or same >= 0.999, f"identical to silu * mul of the plain rows on {same:.5f} of {d.numel()} elements"
        return ratio

    def finish(self, failures, name):
        frac = self.same / max(1, self.total)
        print(f"layer-operands | {name} | gate|up identical to torch's silu * mul on {frac:.5f} of {self.total} elements (bar: >= 0.999)")
        if frac < 0.999:
            failures.append(f"2 values | {name} | gate|up identical fraction {frac:.5f} < 0.999")


class Cells:
    """A test item sweeps its layer class over dtypes and shapes; what fails is gathered and asserted once, in ``done()``, so that one
    run names every failing cell (and the suite does not grow by an item per cell)."""

    def __init__(self):
        self.failures = []

    def expect(self, ok, *what):
        if not ok:
            self.failures.append(" | ".join(str(w) for w in what))

    def done(self):
        assert not self.failures, f"{len(self.failures)} failing cells:\n" + "\n".join(self.failures[:300])


def run(cells, rec, name, dtype, build, K, M_out, rows, residual=False, check=None, before=None):
    """``build()`` twice: the layer that only sees fresh allocations and the one that sees everything."""
    virgin, exposed = build(), build()
    records, failures = L.sweep(rec, virgin, exposed, K, M_out, rows, dtype, dev(), residual=residual, check=check, before=before, name=name)
    if isinstance(check, GatedCheck):
        check.finish(failures, name)
    L.report(name, dtype, records, failures)
    cells.failures += [f"{str(dtype)[6:]} | {f}" for f in failures]
    return records


def tname(shape):
    return f"{shape[0]}x{shape[1]}"


def dname(dtype):
    return str(dtype)[6:]


# ---- TorchFP4Linear under each switch ------------------------------------------------------------------------------------------------------
def torch_linear(kind, M, K, dtype, bs=64, seed=1):
    P, A, w64 = weight(kind, M, K, seed, bs)
    code = (pkg().nn.fp4_code() if kind == "fp4" else pkg().nn.nf4_code()).to(dev())
    bias = vector(M, seed + 50, dtype)
    return pkg().serialization.plain_linear(P, A, code, (M, K), bs, dtype, kind, bias), Ref(w64, bias)


LINEAR_CASES = [("fp4", "off", None, DT16 + [F32]), ("fp4", "small_batch_fused", {}, DT16 + [F32]),
                ("nf4", "off", None, DT16), ("nf4", "nf4", dict(nf4=True), DT16), ("nf4", "nf4_wide", dict(nf4_wide=True), DT16)]


@pytest.mark.parametrize("kind,switch,switches,dtypes", LINEAR_CASES, ids=[f"{k}-{s}" for k, s, _, _ in LINEAR_CASES])
def test_torch_linear_under_each_switch(rec, kind, switch, switches, dtypes):
    """TorchFP4Linear, FP4 and NF4: the reference dispatch (the switch off takes every call - assertion 1's yardstick) and each of the
    three switches of set_small_batch_fused; every dtype the route admits, both shapes."""
    cells = Cells()
    fused_op = {"small_batch_fused": "gemm_small_fp4", "nf4": "gemm_small_nf4", "nf4_wide": "gemm_wide_nf4"}.get(switch)
    for dtype in dtypes:
        for M, K in L.SHAPES:
            rows = L.ROWS_F32 if dtype == F32 else L.ROWS + (L.ROWS_FP4_MORE if kind == "fp4" else [])
            ref = torch_linear(kind, M, K, dtype)[1]

            def build():
                layer = torch_linear(kind, M, K, dtype)[0]
                if switches is not None:
                    assert pkg().set_small_batch_fused(layer, True, **switches) == 1
                return layer
            name = f"TorchFP4Linear {kind} {switch} {M}x{K}"
            records = run(cells, rec, name, dtype, build, K, M, rows, check=bar_check(ref, dtype))
            # the switch does route: every many-row call of a covered cell went to the fused op, whatever the presentation
            for r, how, route, _ in records:
                n = L.n_rows(r)
                if switch == "small_batch_fused":
                    want = n >= 2 and (dtype != F32 or n <= 8)
                elif switch == "nf4":
                    want = 2 <= n <= 16 and K % 512 == 0
                elif switch == "nf4_wide":
                    want = 17 <= n <= 64 or (2 <= n <= 16 and K % 512 != 0)
                else:
                    want = False
                ok = (fused_op in L.ops(route)) == want if fused_op else not any(op.startswith("gemm_") for op in L.ops(route))
                cells.expect(ok, dname(dtype), "route", name, r, how, L.show(route))
    cells.done()


# ---- FusedFP4Linear / FusedNF4Linear -------------------------------------------------------------------------------------------------------
def fused_cls(kind):
    return pkg().FusedFP4Linear if kind == "fp4" else pkg().FusedNF4Linear


def gate_up_parts(kind, K, dtype):
    (Pg, Ag, wg), (Pu, Au, wu) = weight(kind, 64, K, 11), weight(kind, 64, K, 12)
    bg, bu = vector(64, 61, dtype), vector(64, 62, dtype)
    w64 = np.stack([wg, wu], 1).reshape(128, K)  # rows g0, u0, g1, u1, ...
    bias = torch.stack([bg, bu], 1).reshape(-1)
    return (Pg, Ag), (Pu, Au), bg, bu, w64, bias


def fused_rows(kind, dtype):
    return L.ROWS + (L.ROWS_FP4_MORE if kind == "fp4" else [])


@pytest.mark.parametrize("kind", ["fp4", "nf4"])
def test_fused_linear_with_bias_and_residual(rec, kind):
    """f32 where a route admits it: the FP4 GEMV (NF4's fused ops are 16-bit)."""
    cells = Cells()
    for dtype in DT16 + ([F32] if kind == "fp4" else []):
        for M, K in L.SHAPES:
            P, A, w64 = weight(kind, M, K, 1)
            bias = vector(M, 51, dtype)
            build = lambda: fused_cls(kind).from_packed(P, A, (M, K), 64, bias)  # noqa: E731
            rows = L.ROWS_F32 if dtype == F32 else fused_rows(kind, dtype)
            run(cells, rec, f"{fused_cls(kind).__name__} plain {M}x{K}", dtype, build, K, M, rows, residual=True,
                check=bar_check(Ref(w64, bias), dtype))
    cells.done()


@pytest.mark.parametrize("kind", ["fp4", "nf4"])
def test_fused_linear_gate_up(rec, kind):
    cells = Cells()
    cls = fused_cls(kind)
    for dtype in DT16:
        for _, K in L.SHAPES:
            gate, up, bg, bu, w64, bias = gate_up_parts(kind, K, dtype)
            build = lambda: cls.gate_up_from_packed(gate, up, (64, K), 64, bg, bu)  # noqa: E731
            plain = cls(build().quant_data, NONE)
            check = GatedCheck(rec, plain, bar_check(Ref(w64, bias), dtype))
            run(cells, rec, f"{cls.__name__} gate|up 2x64x{K}", dtype, build, K, 64, fused_rows(kind, dtype), residual=True, check=check)
    cells.done()


# ---- LoRA ----------------------------------------------------------------------------------------------------------------------------------
def test_lora_linear_plain(rec):
    cells = Cells()
    for dtype in DT16:
        for M, K in L.SHAPES:
            P, A, w64 = weight("nf4", M, K, 1)
            bias = vector(M, 51, dtype)
            ad = adapter(M, K, 71, dtype)
            build = lambda: pkg().LoRANF4Linear.from_fused(pkg().FusedNF4Linear.from_packed(P, A, (M, K), 64, bias), *ad)  # noqa: E731
            name = f"LoRANF4Linear plain {M}x{K}"
            records = run(cells, rec, name, dtype, build, K, M, L.ROWS, residual=True, check=bar_check(Ref(w64, bias, [ad]), dtype))
            for r, how, route, _ in records:  # the adapter stays on its fused route, whatever the presentation
                want = ["lora_down", "gemv_nf4_lora" if L.n_rows(r) == 1 else "gemm_nf4_lora"]
                cells.expect(L.ops(route) == want, dname(dtype), "route", name, r, how, L.show(route))
    cells.done()


def test_lora_linear_gate_up(rec):
    cells = Cells()
    for dtype in DT16:
        for _, K in L.SHAPES:
            gate, up, bg, bu, w64, bias = gate_up_parts("nf4", K, dtype)
            ga, ua = adapter(64, K, 73, dtype), adapter(64, K, 75, dtype)
            build = lambda: pkg().LoRANF4Linear.gate_up_from_fused(  # noqa: E731
                pkg().FusedNF4Linear.gate_up_from_packed(gate, up, (64, K), 64, bg, bu), ga, ua)
            gu = build()
            plain = pkg().LoRANF4Linear(gu.quant_data, NONE, gu.lora_A, gu.lora_B, gu.lora_scale)
            # the stacked adapter, as the layer holds it: one scale per adapter row, folded into A for the reference
            stacked = [(gu.lora_A.double() * gu.lora_scale.double()[:, None], gu.lora_B, 1.0)]
            check = GatedCheck(rec, plain, bar_check(Ref(w64, bias, stacked), dtype))
            run(cells, rec, f"LoRANF4Linear gate|up 2x64x{K}", dtype, build, K, 64, L.ROWS, residual=True, check=check)
    cells.done()


IDS = [0, 1, -1]


def test_multi_lora_linear(rec):
    """Two adapters, ids that mix 0, 1 and -1 (the bare base model) over the rows."""
    cells = Cells()
    sel = pkg().AdapterSelection(device=dev())
    ids_of = lambda n: [IDS[(b + n) % 3] for b in range(n)]  # noqa: E731
    for dtype in DT16:
        for M, K in L.SHAPES:
            P, A, w64 = weight("nf4", M, K, 1)
            bias = vector(M, 51, dtype)
            ads = [adapter(M, K, 81, dtype), adapter(M, K, 83, dtype, rank=8)]
            build = lambda: pkg().MultiLoRANF4Linear.from_fused(pkg().FusedNF4Linear.from_packed(P, A, (M, K), 64, bias), ads, sel)  # noqa: E731
            name = f"MultiLoRANF4Linear {M}x{K}"
            records = run(cells, rec, name, dtype, build, K, M, L.ROWS, residual=True,
                          check=bar_check(Ref(w64, bias, ads), dtype, ids_of), before=lambda n: sel.set(ids_of(n)))
            for r, how, route, _ in records:
                want = ["lora_down_multi", "gemv_nf4_lora_multi" if L.n_rows(r) == 1 else "gemm_nf4_lora_multi"]
                cells.expect(L.ops(route) == want, dname(dtype), "route", name, r, how, L.show(route))
    cells.done()


# ---- resident (nested) layers ------------------------------------------------------------------------------------------------------------------
def nested_layer(M, K, dtype, bias, **switches):
    P, q, nested, table, _ = nested_weight(M, K, 1)
    layer = pkg().NestedNF4Linear(P, q, nested, table, NESTED_OFFSET, (M, K), 64, bias, dtype)
    if switches:
        assert pkg().set_small_batch_fused(layer, True, **switches) == 1
    return layer


@pytest.mark.parametrize("switch", ["off", "nf4", "nf4_wide", "both"])
def test_nested_linear_under_both_switches(rec, switch):
    cells = Cells()
    switches = {"off": {}, "nf4": dict(nf4=True), "nf4_wide": dict(nf4_wide=True), "both": dict(nf4=True, nf4_wide=True)}[switch]
    for dtype in DT16:
        for M, K in L.SHAPES:
            bias = vector(M, 51, dtype)
            build = lambda: nested_layer(M, K, dtype, bias, **switches)  # noqa: E731
            name = f"NestedNF4Linear {switch} {M}x{K}"
            records = run(cells, rec, name, dtype, build, K, M, L.ROWS, residual=True,
                          check=bar_check(Ref(nested_weight(M, K, 1)[4], bias), dtype))
            for r, how, route, _ in records:
                n, small = L.n_rows(r), K % 512 == 0
                routed = 2 <= n <= 64 and (switches.get("nf4", False) if n <= 16 and small else switches.get("nf4_wide", False))
                cells.expect(("gemm_nf4_nested" in L.ops(route)) == routed, dname(dtype), "route", name, r, how, L.show(route))
    cells.done()


def test_lora_nested_linear(rec):
    cells = Cells()
    for dtype in DT16:
        for M, K in L.SHAPES:
            bias = vector(M, 51, dtype)
            ad = adapter(M, K, 71, dtype)
            build = lambda: pkg().LoRANestedNF4Linear.from_nested(nested_layer(M, K, dtype, bias, nf4=True, nf4_wide=True), *ad)  # noqa: E731
            run(cells, rec, f"LoRANestedNF4Linear {M}x{K}", dtype, build, K, M, L.ROWS, residual=True,
                check=bar_check(Ref(nested_weight(M, K, 1)[4], bias, [ad]), dtype))
    cells.done()


# ---- a gated MLP through fuse_gated_mlps ----------------------------------------------------------------------------------------------------
class ToyMLP(nn.Module):
    def __init__(self, gate, up, down):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj, self.act_fn = gate, up, down, nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


@pytest.mark.parametrize("kind", ["fp4", "nf4"])
def test_gated_mlp_through_fuse_gated_mlps(rec, kind):
    """hidden 512 -> 2 x 64 -> 128.  The value of an MLP has no one-rounding bar; its halves have: the fused gate|up layer is swept on its
    own above, and here the MLP's output is held to the bar against the float64 down projection of the layer's own gate|up output."""
    cells = Cells()
    for dtype in DT16:
        gated_mlp_cells(cells, rec, kind, dtype)
    cells.done()


def gated_mlp_cells(cells, rec, kind, dtype):
    H, I, O = 512, 64, 128
    code = (pkg().nn.fp4_code() if kind == "fp4" else pkg().nn.nf4_code()).to(dev())
    Pd, Ad, wd = weight(kind, O, I, 13)
    ref = Ref(wd)

    def build():
        lin = lambda s, m, k: pkg().serialization.plain_linear(*weight(kind, m, k, s)[:2], code, (m, k), 64, dtype, kind, None)  # noqa: E731
        root = nn.Sequential(ToyMLP(lin(11, I, H), lin(12, I, H), lin(13, O, I)))
        assert pkg().fuse_gated_mlps(root, nf4=kind == "nf4") == 1 and isinstance(root[0], pkg().FusedGatedMLP)
        assert pkg().set_small_batch_fused(root, True, nf4=True, nf4_wide=True) == 1  # the down projection
        return root[0]

    fresh_only = build()  # computes the gate|up output the check starts from; sees fresh allocations only

    def check(rows, x, res, y, route):
        h = fresh_only.gate_up(L.placed(x, "fresh"))
        exact, tol = ref(h, None, None, dtype, route[1:])  # the down projection's part of the route
        ratio = float((np.abs(f64(y).reshape(exact.shape) - exact) / tol).max())
        assert ratio <= 1.0, f"worst err/tol {ratio:.3f}"
        return ratio

    rows = L.ROWS + (L.ROWS_FP4_MORE if kind == "fp4" else [])  # the FP4 gate|up op takes up to 128 rows
    run(cells, rec, f"FusedGatedMLP {kind} 512-2x64-128", dtype, build, H, O, rows, check=check)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_an_off_alignment_static_input(rec):
    """FusedNF4Linear, 8 rows, the static input one element off a 16-byte boundary: the replay is bit-equal to eager and follows an
    in-place rewrite of the input (the copy that makes the call coverable is part of the captured step)."""
    M, K = L.MAIN
    P, A, _ = weight("nf4", M, K, 1)
    layer = pkg().FusedNF4Linear.from_packed(P, A, (M, K), 64, vector(M, 51, BF16))
    view = lambda buf: buf[1:1 + 8 * K].view(8, K)  # noqa: E731
    buf = torch.zeros(8 * K + 8, dtype=BF16, device=dev())
    view(buf).copy_(L.random((8, K), BF16, 5, dev()))
    assert view(buf).is_contiguous() and view(buf).data_ptr() % 16 == 2
    eager = layer(view(buf)).clone()
    assert L.ops(rec.take()) == ["gemm_nf4_fused"]
    step = pkg().GraphedStep(lambda b: layer(view(b)), buf)
    assert view(step.static_inputs[0]).data_ptr() % 16 == 2
    assert L.same_bits(step(buf), eager)
    for seed in (6, 7):
        view(buf).copy_(L.random((8, K), BF16, seed, dev()))
        assert L.same_bits(step(buf), layer(view(buf)))
    assert L.same_bits(step(buf), layer(view(buf).clone()))  # ... and to the fresh-allocation call


# ---- block sizes at module level ---------------------------------------------------------------------------------------------------------------
def blocksize_calls(cells, rec, name, dtype, call, check, route_ok, K, M):
    """2 and 8 rows in every presentation through ``call(x, res, how)``: no exception, values, the recorded route; a failing cell is
    recorded (and printed like the sweep's) and the next one still runs."""
    dt = dname(dtype)

    def fail(kind, rows, how, what):
        print(f"layer-operands | FAIL | {dt} | {kind} | {name} | rows {rows} | {how} | {what}")
        cells.expect(False, dt, kind, name, f"rows {rows}", how, what)

    for rows in L.BLOCKSIZE_ROWS:
        x, res = L.random((rows, K), dtype, rows, dev()), L.random((rows, M), dtype, rows + 9, dev())
        for how in L.PLACEMENTS:
            rec.take()
            try:
                y = call(x, res, how)
            except RuntimeError as exc:
                fail("1 no exception", rows, how, f"{L.show(rec.take())} | {str(exc)[:160]}")
                continue
            route = rec.take()
            try:
                ratio = f"{check(rows, x, res, y, route):.3f}"
            except AssertionError as exc:
                ratio = "-"
                fail("2 values", rows, how, f"{L.show(route)} | {str(exc)[:160]}")
            print(f"layer-operands | {name} | {dt} | rows {rows} | {how} | {L.show(route)} | worst err/tol {ratio}")
            if not route_ok(L.ops(route)):
                fail("route", rows, how, L.show(route))


def one_qlinear(route_ops):
    return len(route_ops) == 1 and route_ops[0].startswith("qlinear")


def test_fp4_linear_blocksizes_under_the_switch(rec):
    """FP4 layers from oracle-quantised bytes (the device quantiser takes powers of two from 32), small_batch_fused on, 2 and 8 rows:
    no exception, values within the bar, and the recorded route - gemm_small_fp4 for a power of two >= 32 (and for f32 activations
    at every blocksize: the f32 GEMV per row), qlinear* for 16 and 96 with 16-bit activations."""
    cells, M = Cells(), L.BLOCKSIZE_M
    for bs, K in L.BLOCKSIZE_CASES:
        for dtype in DT16 + [F32]:
            layer, ref = torch_linear("fp4", M, K, dtype, bs, seed=bs)
            assert pkg().set_small_batch_fused(layer, True) == 1
            fused = dtype == F32 or L.fused_blocksize(bs)
            blocksize_calls(cells, rec, f"TorchFP4Linear fp4 blocksize {bs} K {K}", dtype, lambda x, res, how: layer(L.placed(x, how)),
                            lambda rows, x, res, y, route: bar_check(ref, dtype)(rows, x, None, y, route),
                            (lambda r: r == ["gemm_small_fp4"]) if fused else one_qlinear, K, M)
    cells.done()


def test_fused_fp4_linear_blocksizes(rec):
    """FusedFP4Linear._batched_covers carries the same clause, so the same cases: gemm_small_fp4_fused for a power of two >= 32 with
    16-bit activations; the unfused sequence (qlinear*: the layer's own small_batch_fused is off) for 16 and 96, and for f32 at every
    blocksize (the batched fused op is 16-bit)."""
    cells, M = Cells(), L.BLOCKSIZE_M
    for bs, K in L.BLOCKSIZE_CASES:
        for dtype in DT16 + [F32]:
            P, A, w64 = weight("fp4", M, K, bs, bs)
            bias = vector(M, bs + 50, dtype)
            layer = pkg().FusedFP4Linear.from_packed(P, A, (M, K), bs, bias)
            fused = dtype != F32 and L.fused_blocksize(bs)
            blocksize_calls(cells, rec, f"FusedFP4Linear blocksize {bs} K {K}", dtype,
                            lambda x, res, how: layer(L.placed(x, how), residual=L.placed(res, "fresh" if how == "fresh" else "off1")),
                            bar_check(Ref(w64, bias), dtype), (lambda r: r == ["gemm_small_fp4_fused"]) if fused else one_qlinear, K, M)
    cells.done()


# ---- the text of a refusal ---------------------------------------------------------------------------------------------------------------------
def test_a_misaligned_pointer_is_not_reported_as_a_datatype_problem():
    """The C ABI still refuses the pointer, in its own words; the host layer adds "Unsupported datatype: " to the entry points' dtype
    refusals only ("unsupported dtype <n>"), not to every message that prints dtype=<n> among the shape it refuses."""
    M, K = L.MAIN
    P, A, _ = weight("fp4", M, K, 1)
    buf = torch.zeros(4 * K + 8, dtype=BF16, device=dev())
    x = buf[1:1 + 4 * K].view(4, K)
    with pytest.raises(RuntimeError) as info:
        pkg().ext.gemm_small_fp4(x, P.t(), A, 64, [M, K], None)
    text = str(info.value)
    assert text.startswith(f"fp4_hip_gemm_small: shape B=4 M={M} K={K} blocksize=64 dtype=2 is not covered; use dequant + GEMM"), text
    assert "Unsupported datatype" not in text
