"""The fused kernels' epilogues at EDGE VALUES, at every call site, through the C ABI (tests/epilogue_values.py is the reference).

The sums are pinned elsewhere (test_gpu_fp4_constructed.py, test_gpu_nf4_constructed.py); here no sum needs a hard weight, and what
is checked is the elementwise chain behind it - bias add, the roundings to T, g / (1 + expf(-g)), the product with the up row, the
residual add - at +-0, +-inf, NaN, subnormals of both 16-bit types, gates below -88.72 (expf overflows: -0) and from 16.64 on (1 + e is
1), 0 * inf and inf - inf through bias, up row and residual, overflow of T, ties at every rounding and the sign of zero after each.

* bias-driven: every weight nibble is the zero code (FP4 nibble 0, NF4 nibble 7; filled on the device), so every sum is +0, and
  bias[2i] carries the gate pattern, bias[2i + 1] the up value, `residual` the residual.  Any pattern at any shape.
* sum-driven: one +-1.0 code per weight row at k = 0 under a block scale that holds the value, a one-hot activation whose entry
  differs per batch row (each batch row another class of sums: unchanged, +0, ties, towards the subnormals, past max); for the
  LoRA forms the value sits in lora_B[row][0] and the batch row's factor in t over an all-zero weight.

The multi-adapter forms (ids mixing -1 and real adapters) and the nested forms run the bias-driven edge set (the LoRA ones with a
one-hot adapter on top) and must give the single-adapter / un-nested form's output under the same equality; the nested forms also
run the sum-driven operands, the row's value carried by the double-quantised statistics (200 gate values per launch: the table has 256
entries).

The gate and up rows the reference is fed are READ from the plain entry point on the same operands, and that they are the intended
ones is asserted first (a precondition).  Every comparison is membership in the reference set under its equality (same bits; NaN
matches NaN); torch's own ops on the device (F.silu(g) * u + r, the rounded adds) are held to the same equality as a second
opinion that shares the device's exp.  Each test prints
    epilogue-values | section | family | dtype | rows checked | multi-member rows | mismatches
(profiles/epilogue_values.txt keeps the lines).  Outputs (and the split-K workspace) sit between guards."""
import copy

import numpy as np
import pytest
import torch

import epilogue_values as V
import fp4_constructed as C
import hipabi
import nf4_ref as R
import test_gpu_fp4_constructed as F4
import test_gpu_nf4_constructed as N4
import test_gpu_nested_batch as NBT
import test_gpu_nf4_multi_lora as ML
import test_gpu_nf4_wide_batch as WB
from gpu_util import NPDT, bits, dev, to_dev
from test_gpu_nested import gemv_nested
from test_gpu_nf4_fused import gemm_fused, gemv_fused

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NONE, GATED = hipabi.EPILOGUE_NONE, hipabi.EPILOGUE_SILU_MUL_PAIRS
GUARD = 4096
R12 = np.float32(1.0 / 12.0)
VARIANT_KEYS = ("gemv", "gemm_small", "gemm_wide", "gemv_nf4", "gemm_wide_nf4")


@pytest.fixture(autouse=True)
def _heuristics_restored():
    yield
    for k in VARIANT_KEYS:
        hipabi.set_variant(k, -1)


def src_of(dtype):
    """The 16-bit type whose patterns drive a dtype (f32 runs on the bf16 patterns: they are f32 values with a short mantissa)."""
    return NPDT[BF16 if dtype == F32 else dtype]


def t_of(pattern_bits, dtype):
    """uint16 patterns -> a device tensor of dtype holding exactly those values."""
    pattern_bits = np.ascontiguousarray(pattern_bits, np.uint16)
    if dtype == F32:
        return to_dev(V.values(pattern_bits, V.BF16))
    return to_dev(pattern_bits.view(np.int16)).view(dtype)


def t_vals(a, dtype):
    """f32 values -> a device tensor of dtype, converted on the host (the values are T values: exact)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).to(dev())


def vals(t):
    """A device tensor's values as f32 on the host, through its bit patterns (no conversion on the device)."""
    b = bits(t)
    return b.view(np.float32).reshape(t.shape) if t.dtype == F32 else V.values(b, NPDT[t.dtype]).reshape(t.shape)


def dev_differs(a, b):
    """Mask of the elements of two device tensors that differ under the reference's equality: same bits, or both NaN."""
    raw = {2: torch.int16, 4: torch.int32}[a.element_size()]
    a, b = a.contiguous(), b.contiguous()
    return ~((a.view(raw) == b.view(raw)) | (a.isnan() & b.isnan()))


def dev_mismatches(a, b):
    return int(dev_differs(a, b).sum())


def hex_at(t, idx):
    return hex(int(t[idx].view({2: torch.int16, 4: torch.int32}[t.element_size()]).item()) & ((1 << 8 * t.element_size()) - 1))


class Site:
    """One epilogue call site: a Family of one of the constructed files at a row count, depth and variant, with all-zero-code or
    one-code-per-row weights made on the device."""

    def __init__(self, kind, fam, B=None, K=None, up_cut=False):
        self.kind, self.fam = kind, copy.copy(fam)
        self.B = self.fam.B = fam.B if B is None else B
        self.K = self.fam.K = fam.K if K is None else K
        self.name = f"{kind} {fam.name} B{self.B} K{self.K}"
        self.batch = fam.entry in ("small", "ws", "gemm_fused", "gemm_lora")
        self.lora = fam.entry in ("lora", "gemm_lora")
        self.gated = (fam.gated and not fam.misaligned) if kind == "fp4" else fam.entry != "gemv"
        self.plain_only = kind == "nf4" and fam.entry == "gemv"  # the plain GEMV entry: a bias and nothing else
        self.dtypes, self.up_cut = fam.dtypes, up_cut

    def slices(self, n, rows_per_item=1):
        """Slices of n items (rows, or pairs of rows) that one launch takes: the split-K path covers M < 24 rows per CU."""
        step = n
        if self.fam.entry == "ws":
            step = (24 * torch.cuda.get_device_properties(0).multi_processor_count - 2) // rows_per_item
        edges = np.linspace(0, n, -(-n // step) + 1).astype(np.int64)  # near-equal parts: none falls below the path's 16 rows
        return [slice(int(lo), int(hi)) for lo, hi in zip(edges[:-1], edges[1:])]

    def __repr__(self):
        return self.name

    def direct_sum(self, dtype):
        """Whether a one-product sum is f32(x a): NF4, the adapter term, f32 activations and the generic kernel; the 16-bit FP4
        kernels form f32(f32(12 x a) * f32(1/12))."""
        return self.kind == "nf4" or dtype == F32 or self.fam.misaligned

    def chain(self, dtype):
        return (V.operand_batch, V.plain_batch) if self.batch else (V.operand_batch1, V.plain_batch1)

    # ---- operands ----
    def weight(self, M, a=None, through_weight=False):
        """P, A of an [M, K] weight of zero codes under unit scales; with `a` f32[M], row r has the code sign(a_r) * 1.0 at k = 0
        under the block scale |a_r| (the LoRA forms keep the zero weight, their values travel through the adapter, unless
        through_weight)."""
        K, bs = self.K, self.fam.bs
        zero, plus, minus = (0x00, 0x30, 0xB0) if self.kind == "fp4" else (0x77, 0xF7, 0x07)
        P = torch.full((M * K // 2,), zero, dtype=torch.uint8, device=dev())
        A = torch.ones(M * K // bs, dtype=torch.float32, device=dev())
        if a is not None and (through_weight or not self.lora):
            P.view(M, K // 2)[:, 0] = to_dev(np.where(np.signbit(a), minus, plus).astype(np.uint8))
            A.view(M, K // bs)[:, 0] = to_dev(np.abs(a).astype(np.float32))
        return P, A

    def x(self, s, dtype, through_weight=False):
        """[B, K] activations: ones where s is None, else one-hot rows with s_b at k = 0 (the LoRA forms: ones)."""
        x = torch.ones(self.B, self.K, dtype=dtype, device=dev())
        if s is not None and (through_weight or not self.lora):
            x.zero_()
            x[:, 0] = t_vals(s, dtype)
        return F4.placed(x, 1) if self.fam.misaligned else x

    def adapter(self, M, dtype, a=None, s=None):
        """lora_B T[M, R] and t f32[B, R]: all zero / ones, or lora_B[r][0] = a_r and t[b][0] = s_b with zeros elsewhere."""
        Rr = self.fam.Rr
        lB = torch.zeros(M, Rr, dtype=dtype, device=dev())
        t = torch.ones(self.B, Rr, dtype=torch.float32, device=dev())
        if a is not None:
            lB[:, 0] = t_vals(a, dtype)
            t.zero_()
            t[:, 0] = to_dev(np.asarray(s, np.float32))
        return lB, t

    def sums(self, dtype, a, s):
        """f32[B, M]: the kernels' finished row sums for row values a and batch-row factors s, zero sums being +0."""
        prod = np.asarray(s, np.float64)[:, None] * np.asarray(a, np.float64)[None, :]
        with np.errstate(over="ignore", under="ignore"):
            total = prod.astype(np.float32) if self.direct_sum(dtype) else (12.0 * prod).astype(np.float32) * R12
        return np.where(total == 0, np.float32(0.0), total).astype(np.float32)

    # ---- calls ----
    def run(self, ops, M, dtype, bias=None, residual=None, epilogue=NONE, plain=False, into=None, base_form=False):
        """One call into a guarded output (or `into`, a view of a guarded buffer the caller checks); returns [B, M or M / 2].
        plain: the plain entry point (the LoRA forms have none: their own entry without residual).  base_form: a LoRA site's
        fused entry without the adapter."""
        fam, B, K = self.fam, self.B, self.K
        n = B * (M // 2 if epilogue == GATED else M)
        buf = None
        if into is None:
            buf, into = C.guarded(n, dtype, GUARD, dev())
        out = into.view(B, -1)
        x, P, A = ops["x"], ops["P"], ops["A"]
        if self.kind == "fp4":
            kw, wsbuf = {}, None
            if fam.entry == "ws":
                asked = F4.ws_bytes(B, M, K, dtype)
                assert asked > 0, (self.name, "not a split-K shape")
                wsbuf, ws = C.guarded(asked, torch.uint8, 4096, dev())
                kw = dict(workspace=ws)
            fam.call(x, P, A, M, K, bias=bias, residual=residual, epilogue=epilogue, out=out, **kw)
            if wsbuf is not None:
                assert not C.untouched(wsbuf, 4096, 4096 + asked) and C.guards_intact(wsbuf, asked, 4096), (self.name, "workspace")
        else:
            fam.M = M
            with F4.forced(**fam.variants):
                if self.lora and not base_form:
                    fam.call(x, P, A, lB=ops["lB"], t=ops["t"], bias=bias, residual=residual, epilogue=epilogue, out=out if self.batch else into)
                elif plain and not self.batch:
                    R.gemv(x.reshape(-1), P, A, M, K, fam.bs, bias, out=into)
                elif plain:
                    rc = WB.call(x, P, A, out, B, M, K, bs=fam.bs, bias=bias)
                    assert rc == hipabi.OK, (rc, hipabi.last_error())
                elif self.batch:
                    gemm_fused(x, P, A, M, K, fam.bs, bias, residual, epilogue, out=out)
                else:
                    gemv_fused(x.reshape(-1), P, A, M, K, fam.bs, bias, residual, epilogue, out=into)
        if buf is not None:
            assert C.guards_intact(buf, n, GUARD), (self.name, "out guards")
        return out


class Tally:
    """Collects the comparisons of one test, prints its line and then asserts."""

    def __init__(self, section, site, dtype):
        self.head = f"epilogue-values | {section} | {site.name} | {NPDT[dtype]}"
        self.rows = self.multi = self.bad = self.torch_bad = 0
        self.examples, self.torch_examples, self.notes = [], [], []

    def add(self, got, want_set, describe=None):
        want_set = np.broadcast_to(want_set, want_set.shape[:1] + got.shape)
        ok = V.agrees(got, want_set)
        self.rows += ok.size
        self.multi += int(V.multi_member(want_set).sum())
        self.bad += int((~ok).sum())
        for idx in np.argwhere(~ok)[:4]:
            idx = tuple(int(i) for i in idx)
            self.examples.append((describe(idx) if describe else idx, "got", hex(int(got[idx].view(np.uint32))),
                                  "want", [hex(int(w.view(np.uint32))) for w in want_set[(slice(None),) + idx]]))

    def torch(self, out, theirs, describe):
        """torch's own ops on the device, under the same equality."""
        bad = dev_differs(out, theirs)
        n = int(bad.sum())
        self.torch_bad += n
        if n and len(self.torch_examples) < 8:
            for idx in bad.nonzero()[:4].tolist():
                idx = tuple(idx)
                self.torch_examples.append((describe(idx), "got", hex_at(out, idx), "torch", hex_at(theirs, idx)))

    def finish(self):
        print(f"{self.head} | {self.rows} | {self.multi} | {self.bad}" + (f" | torch's device ops differ at {self.torch_bad}" if self.torch_bad else "")
              + "".join(f" | {n}" for n in self.notes))
        assert self.bad == 0, (self.head, self.examples[:8])
        assert self.torch_bad == 0, (self.head, "torch's own ops on the device", self.torch_bad, self.torch_examples)
        assert self.rows > 0


def rows_identical(t):
    raw = t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
    return bool((raw == raw[:1]).all())


# ======================================================================================================================================
# the call sites
# ======================================================================================================================================
def fp4(name, table=F4.SCALE_FAMILIES):
    return next(f for f in table if f.name == name)


def nf4(name):
    return next(f for f in N4.SCALE_FAMILIES if f.name == name)


FP4_SITES = (
    [Site("fp4", fp4("gemv default")), Site("fp4", fp4("gemv generic")), Site("fp4", fp4("gemv f32-lds"))] +
    [Site("fp4", fp4(f"gemv regx-{it}")) for it in (1, 2, 4)] +
    [Site("fp4", fp4("gemv bands-5-2", F4.GUARD_FAMILIES)), Site("fp4", fp4("gemv bands-8-2", F4.GUARD_FAMILIES))] +
    [Site("fp4", fp4(n)) for n in ("small valu", "small mfma-rt1", "small mfma-rt2", "small mfma-direct", "small mfma-persist x-image",
                                   "small mfma-persist register-x", "small one-pass one-tile")] +
    [Site("fp4", fp4(f"wide cfg{cfg}")) for cfg in (1, 2, 3, 4)] +
    [Site("fp4", fp4("wide cfg1 two tiles")), Site("fp4", fp4("chunked 16-row launches")), Site("fp4", fp4("split-k"))])
# the families of the NF4 file's table cover the plain GEMV by layout; the fused entry's own layouts, ks 1 and the batched kernels
# forced by workgroup shape have none there
NF4_SITES = (
    [Site("nf4", N4.Family("gemv_fused table16", "fused", dtypes=N4.DTYPES, gemv_nf4=0)),
     Site("nf4", N4.Family("gemv_fused pair-table", "fused", dtypes=N4.DTYPES, gemv_nf4=1)),
     Site("nf4", N4.Family("gemv_fused ks1", "fused", K=1024, dtypes=N4.DTYPES)),
     Site("nf4", nf4("gemv generic")),  # x off 16-byte alignment: the fused entry refuses it, the plain entry adds the bias
     Site("nf4", nf4("gemm_fused 16-row kernel")),
     Site("nf4", N4.Family("gemm_fused wide v1", "gemm_fused", B=33, gemm_wide_nf4=1)),
     Site("nf4", N4.Family("gemm_fused wide v2", "gemm_fused", B=33, gemm_wide_nf4=2)),
     Site("nf4", N4.Family("gemm_fused one-tile", "gemm_fused", B=5, K=192)),
     Site("nf4", N4.Family("gemm_fused two chunks", "gemm_fused", B=100, K=192))] +
    [Site("nf4", nf4(n)) for n in ("gemv_lora", "gemv_lora ks1 R256", "gemm_lora 16-row kernel", "gemm_lora wide", "gemm_lora one-tile")])
SITES = FP4_SITES + NF4_SITES
# the cheapest shape per kernel source file, for the exhaustive run
EXHAUSTIVE_SITES = [
    Site("fp4", fp4("gemv default"), K=64), Site("fp4", fp4("small valu"), B=2, K=64), Site("fp4", fp4("small one-pass one-tile"), B=2, K=192),
    Site("nf4", N4.Family("gemv_fused", "fused", dtypes=N4.DTYPES), K=64), Site("nf4", N4.Family("gemm_fused one-tile", "gemm_fused"), B=2, K=192),
    Site("nf4", nf4("gemm_fused 16-row kernel"), B=2, K=512, up_cut=True)]


def cases(sites, gated_only=False, with_f32=False):
    out = [(s, d) for s in sites for d in s.dtypes if (with_f32 or d != F32) and (s.gated or not gated_only)]
    return pytest.mark.parametrize("site,dtype", out, ids=[f"{s.name}-{NPDT[d]}".replace(" ", "_") for s, d in out])


def test_every_listed_call_site_has_a_gated_case():
    names = {s.name for s, d in cases(SITES, gated_only=True).args[1]}
    assert len(names) == len(SITES) - 3  # all but the two generic kernels and the f32 LDS kernel, which have no gate|up epilogue
    assert {k for s in SITES for k in s.fam.variants} <= set(VARIANT_KEYS)


# ======================================================================================================================================
# bias-driven
# ======================================================================================================================================
def bias_driven(section, site, dtype, gate_bits, up_bits):
    gb, ub = np.repeat(gate_bits, up_bits.size), np.tile(up_bits, gate_bits.size)
    tally = Tally(section, site, dtype)
    for part in site.slices(gb.size, 2):
        bias_driven_launches(tally, site, dtype, gb[part], ub[part])
    tally.finish()


def bias_driven_launches(tally, site, dtype, gb, ub):
    npd, B = NPDT[dtype], site.B
    n = gb.size
    M = 2 * n
    bias_bits = np.empty(M, np.uint16)
    bias_bits[0::2], bias_bits[1::2] = gb, ub
    bias = t_of(bias_bits, dtype)
    P, A = site.weight(M)
    ops = dict(x=site.x(None, dtype), P=P, A=A)
    if site.lora:
        ops["lB"], ops["t"] = site.adapter(M, dtype)
    describe = lambda idx: ("gate", hex(int(gb[idx[-1]])), "up", hex(int(ub[idx[-1]])), "batch row", idx[0])  # noqa: E731

    # precondition: over +0 sums the plain entry point returns the bias patterns themselves (-0 + 0 is +0, a NaN stays a NaN)
    plain = site.run(ops, M, dtype, bias=bias, plain=True)
    assert rows_identical(plain), (site.name, "batch rows of equal operands differ")
    p0 = vals(plain[0])
    operand, _ = site.chain(dtype)
    arrived = V.same(p0, operand(np.zeros(M, np.float32), V.values(bias_bits, npd), npd))
    assert arrived.all(), (site.name, "the plain entry point did not return the bias patterns", [hex(int(b)) for b in bias_bits[~arrived][:8]])
    g0, u0 = p0[0::2], p0[1::2]
    torch_ref = torch.nn.functional.silu(plain[:, 0::2]) * plain[:, 1::2]

    out = site.run(ops, M, dtype, bias=bias, epilogue=GATED)
    tally.add(vals(out), V.gated(g0, u0, npd)[:, None, :], describe)
    tally.torch(out, torch_ref, describe)
    if site.lora:  # an all-zero adapter: the fused form's bits
        assert dev_mismatches(out, site.run(ops, M, dtype, bias=bias, epilogue=GATED, base_form=True)) == 0, (site.name, "zero adapter")

    # the residuals cycle along the pairs, one step further per batch row; with fewer batch rows than residuals, further launches
    # take the cycle on, so that every pair meets every residual
    rb = V.residual_patterns(npd)
    for shift in range(0, rb.size, B):
        idx = (np.arange(n)[None, :] + np.arange(B)[:, None] + shift) % rb.size
        res = t_of(rb[idx], dtype)
        out = site.run(ops, M, dtype, bias=bias, residual=res, epilogue=GATED)
        got = vals(out)
        for phase in range(min(B, rb.size)):
            want = V.gated(g0, u0, npd, V.values(rb[idx[phase]], npd))
            tally.add(got[phase::rb.size], want[:, None, :], lambda i, p=phase, idx=idx: describe(i) + ("residual", hex(int(rb[idx[p, i[-1]]]))))
        tally.torch(out, torch_ref + res, lambda i, idx=idx: describe(i) + ("residual", hex(int(rb[idx[i]]))))


@cases(EXHAUSTIVE_SITES, gated_only=True)
def test_gated_every_gate_pattern(site, dtype):
    """All 65536 gate patterns x U (the 16-row NF4 kernel at K = 512: four of U), without a residual and with every value of R."""
    U = V.up_patterns(NPDT[dtype])
    bias_driven("every gate pattern", site, dtype, np.arange(0x10000, dtype=np.uint32).astype(np.uint16), U[[1, 3, 6, 10]] if site.up_cut else U)


@cases(SITES, gated_only=True)
def test_gated_edge_set_every_call_site(site, dtype):
    """E_T x U x R at the family's own depth and row count."""
    bias_driven("edge set", site, dtype, V.edge_patterns(NPDT[dtype]), V.up_patterns(NPDT[dtype]))


# ======================================================================================================================================
# sum-driven
# ======================================================================================================================================
def row_values(site, dtype, with_off_grid=True):
    """f32 row values: every finite pattern of E_T, and (where the value travels through an f32 scale) the off-grid scales of both
    signs."""
    src = src_of(dtype)
    a = V.values(V.finite(V.edge_patterns(src), src), src)
    if with_off_grid and not site.lora:
        off = V.sum_row_scales(src)
        a = np.concatenate([a, off, -off])
    return a.astype(np.float32)


def batch_factors(site, dtype, through_weight=False):
    """The launches' factors, one per batch row, as many launches as it takes for every factor to reach the site (batch 1: one
    launch per factor).  The adapter's t is f32, so it also takes the off-grid values, both signs."""
    src = src_of(dtype)
    s = V.activation_scales(src)
    if site.lora and not through_weight:
        off = V.sum_row_scales(src)
        s = np.concatenate([s, off, -off])
    B = site.B if site.batch else 1
    return [s[(np.arange(B) + lo) % s.size] for lo in range(0, s.size, B)]


def sum_ops(site, M, dtype, a, s):
    P, A = site.weight(M, a)
    ops = dict(x=site.x(s, dtype), P=P, A=A)
    if site.lora:
        ops["lB"], ops["t"] = site.adapter(M, dtype, a, s)
    return ops


@cases(SITES, gated_only=True)
def test_gated_sum_driven(site, dtype):
    """Gate and up rows that come out of the sum (or the adapter term), without a bias and with one of 16 patterns of E_T."""
    npd = NPDT[dtype]
    ga = row_values(site, dtype)
    ua = V.values(V.finite(V.up_patterns(npd), npd), npd)
    tally = Tally("sum-driven gated", site, dtype)
    lost = set()
    for part in site.slices(ga.size * ua.size, 2):
        gated_sum_driven_launches(tally, lost, site, dtype, np.repeat(ga, ua.size)[part], np.tile(ua, ga.size)[part])
    if lost:
        mags = sorted(abs(v) for v in lost)
        tally.notes.append(f"{len(lost)} finite patterns did not arrive through the sum (|value| {mags[0]:.3g} .. {mags[-1]:.3g})")
        # what cannot be driven through a sum is a finding, never a silent gap: only the 16-bit FP4 kernels' f32(12 x a), which
        # overflows from f32 max / 12 on, may lose patterns
        top = float(np.finfo(np.float32).max) / 12.0
        assert site.kind == "fp4" and not site.direct_sum(dtype) and all(abs(v) > top * (1 - 2.0**-20) for v in lost), (site.name, sorted(lost)[:8])
    tally.finish()


def gated_sum_driven_launches(tally, lost, site, dtype, ga, ua):
    npd, B = NPDT[dtype], site.B
    n = ga.size
    M = 2 * n
    a = np.empty(M, np.float32)
    a[0::2], a[1::2] = ga, ua
    on_grid = V.same(V.rt(ga, npd), ga) & (ga != 0)  # the finite non-zero patterns of E_T among the gate rows (a zero sum is +0)
    pair = np.arange(n)
    sub = V.bias_subset(npd)
    bias_bits = np.empty(M, np.uint16)
    bias_bits[0::2], bias_bits[1::2] = sub[(2 * pair + pair // 16) % 16], sub[(2 * pair + 1 + pair // 16) % 16]
    rb = V.residual_patterns(npd)
    operand, _ = site.chain(dtype)
    for s in batch_factors(site, dtype):
        ops = sum_ops(site, M, dtype, a, s)
        total = site.sums(dtype, a, s)
        describe = lambda idx: ("gate value", float(a[2 * idx[-1]]), "up value", float(a[2 * idx[-1] + 1]), "factor", float(s[idx[0]]))  # noqa: E731
        for bias, bv in ((None, None), (t_of(bias_bits, dtype), V.values(bias_bits, npd))):
            plain = site.run(ops, M, dtype, bias=bias, plain=True)
            p = vals(plain)
            # precondition: the plain entry point returns the intended rows
            intended = operand(total, bv, npd)
            ok = V.same(p, intended)
            assert ok.all(), (site.name, "plain rows are not the restated sums", [(float(s[i]), float(a[j]), float(p[i, j]), float(intended[i, j])) for i, j in np.argwhere(~ok)[:8]])
            if bias is None:  # which finite patterns of E_T arrived unchanged through the sum under a unit factor
                for b in np.flatnonzero(s == 1.0):
                    lost.update(float(v) for v in np.unique(ga[on_grid & ~V.same(p[b, 0::2], ga)]))
            g, u = p[:, 0::2], p[:, 1::2]
            torch_ref = torch.nn.functional.silu(plain[:, 0::2]) * plain[:, 1::2]
            out = site.run(ops, M, dtype, bias=bias, epilogue=GATED)
            tally.add(vals(out), V.gated(g, u, npd), describe)
            tally.torch(out, torch_ref, describe)
            idx = (pair[None, :] + np.arange(B)[:, None]) % rb.size
            res = t_of(rb[idx], dtype)
            out = site.run(ops, M, dtype, bias=bias, residual=res, epilogue=GATED)
            tally.add(vals(out), V.gated(g, u, npd, V.values(rb[idx], npd)), describe)
            tally.torch(out, torch_ref + res, describe)


@cases(SITES, with_f32=True)
def test_plain_sum_bias_residual(site, dtype):
    """The plain chain: every pattern of E_T as bias meets every sum class, every value of R' as residual meets every sum class and
    |E_T| / |R'| bias patterns; once more with the residual aliasing out."""
    src = src_of(dtype)
    E = V.edge_patterns(src)
    mx, tiny = V.values([V.max_bits(src)], src)[0], V.values([1], src)[0]
    classes = np.array([0.0, 1.0, -1.0, mx, -mx, tiny, -tiny], np.float32)
    if not site.lora:
        off = V.sum_row_scales(src)
        classes = np.concatenate([classes, off, -off[4:]])
    tally = Tally("sum-driven plain", site, dtype)
    for part in site.slices(classes.size * E.size):
        plain_launches(tally, site, dtype, np.repeat(classes, E.size)[part], np.tile(E, classes.size)[part])
    tally.finish()


def plain_launches(tally, site, dtype, a, bias_bits):
    npd, src, B, M = NPDT[dtype], src_of(dtype), site.B, a.size
    bias, bv = t_of(bias_bits, dtype), V.values(bias_bits, src)
    rp = V.residual_prime_patterns(src)
    idx = (np.arange(M)[None, :] + np.arange(B)[:, None]) % rp.size
    res, rv = t_of(rp[idx], dtype), V.values(rp[idx], src)
    _, chain = site.chain(dtype)
    for s in batch_factors(site, dtype):
        ops = sum_ops(site, M, dtype, a, s)
        total = site.sums(dtype, a, s)
        total_dev = to_dev(total)
        describe = lambda i: ("row value", float(a[i[-1]]), "factor", float(s[i[0]]), "bias", hex(int(bias_bits[i[-1]])), "residual", hex(int(rp[idx[i]])))  # noqa: E731
        bare = site.run(ops, M, dtype, plain=True)
        tally.add(vals(bare), chain(total, npd)[None], describe)

        def torch_chain(with_res):
            if dtype == F32:
                t = total_dev + bias
            elif site.batch:
                t = (total_dev + bias.float()).to(dtype)
            else:
                t = bare + bias
            return t + res if with_res else t

        out = site.run(ops, M, dtype, bias=bias, plain=True)
        tally.add(vals(out), chain(total, npd, bv)[None], describe)
        tally.torch(out, torch_chain(False), describe)
        if site.plain_only:
            continue
        out = site.run(ops, M, dtype, bias=bias, residual=res)
        tally.add(vals(out), chain(total, npd, bv, rv)[None], describe)
        tally.torch(out, torch_chain(True), describe)
        if site.lora:  # a one-hot adapter over a zero weight against the un-adapted form: the same chain on a +0 sum
            base = site.run(ops, M, dtype, bias=bias, residual=res, base_form=True)
            tally.add(vals(base), chain(np.zeros_like(total), npd, bv, rv)[None], describe)
    if site.plain_only:
        return
    # h = h + Linear(a) in place (the last factor's operands)
    hbuf, h = C.guarded(B * M, dtype, GUARD, dev())
    h.copy_(res.reshape(-1))
    site.run(ops, M, dtype, bias=bias, residual=h.view(B, M), into=h)
    assert C.guards_intact(hbuf, B * M, GUARD)
    tally.add(vals(h.view(B, M)), chain(total, npd, bv, rv)[None], describe)


# ======================================================================================================================================
# the multi-adapter and the nested forms: the single-adapter / un-nested form's output on the same operand sets
# ======================================================================================================================================
MULTI_SITES = [s for s in NF4_SITES if s.lora]
FORM_LAUNCHES = ((GATED, False), (GATED, True), (NONE, True))  # (epilogue, with the residual)


def edge_set_operands(site, dtype):
    """The bias-driven edge set (E_T x U as bias pairs, R cycling as residual) over a zero weight; for the LoRA forms a one-hot
    adapter whose first rows carry every finite pattern of E_T into the f32 sum, under another factor per batch row."""
    npd, B = NPDT[dtype], site.B
    E, U = V.edge_patterns(npd), V.up_patterns(npd)
    n = E.size * U.size
    M = 2 * n
    bias_bits = np.empty(M, np.uint16)
    bias_bits[0::2], bias_bits[1::2] = np.repeat(E, U.size), np.tile(U, E.size)
    rb = V.residual_patterns(npd)
    res = {GATED: t_of(rb[(np.arange(n)[None, :] + np.arange(B)[:, None]) % rb.size], dtype),
           NONE: t_of(rb[(np.arange(M)[None, :] + np.arange(B)[:, None]) % rb.size], dtype)}
    P, A = site.weight(M)
    ops = dict(x=site.x(None, dtype), P=P, A=A)
    if site.lora:
        hot = V.values(V.finite(E, npd), npd)
        one_hot = np.zeros(M, np.float32)
        one_hot[:hot.size] = hot
        ops["lB"], ops["t"] = site.adapter(M, dtype, one_hot, V.activation_scales(npd)[np.arange(B) % 7])
    return M, ops, t_of(bias_bits, dtype), res


@cases(MULTI_SITES, gated_only=True)
def test_multi_adapter_forms_equal_the_single_adapter_or_the_fused_form(site, dtype):
    """*_lora_multi_nf4 on the edge set: a stack of an all-zero, the one-hot and another all-zero adapter, the ids mixing -1 and real
    adapters.  Row by row the single-adapter form's output, or the fused form's where the id names no adapter."""
    B, K, fam = site.B, site.K, site.fam
    M, ops, bias, res = edge_set_operands(site, dtype)
    P, A, t, lB1 = ops["P"], ops["A"], ops["t"], ops["lB"]
    stack = torch.stack([torch.zeros_like(lB1), lB1, torch.zeros_like(lB1)]).contiguous()
    id_sets = [[(-1, 1, 0, 2, 1, -1)[b % 6] for b in range(B)]] if site.batch else [[1], [-1], [2]]
    tally = Tally("multi-adapter", site, dtype)
    fam.M = M
    for ids, epilogue, with_res in [(i, e, w) for i in id_sets for e, w in FORM_LAUNCHES]:
        r = res[epilogue] if with_res else None
        width = M // 2 if epilogue == GATED else M
        buf, into = C.guarded(B * width, dtype, GUARD, dev())
        with F4.forced(**fam.variants):
            if site.batch:
                ML.gemm_multi(ops["x"], P, A, M, K, stack, ML.ids_t(ids), t, fam.bs, bias, r, epilogue, out=into.view(B, width))
            else:
                ML.gemv_multi(ops["x"].reshape(-1), P, A, M, K, stack, ML.ids_t(ids), t.reshape(-1), fam.bs, bias, r, epilogue, out=into)
        assert C.guards_intact(buf, B * width, GUARD)
        got = vals(into.view(B, width))
        for which in sorted(set(ids)):
            rows = [b for b in range(B) if ids[b] == which]
            if which < 0:
                want = site.run(ops, M, dtype, bias=bias, residual=r, epilogue=epilogue, base_form=True)
            else:
                want = site.run(dict(ops, lB=stack[which]), M, dtype, bias=bias, residual=r, epilogue=epilogue)
            tally.add(got[rows], vals(want)[rows][None], lambda i: ("id", which, "pair or row", i[-1]))
    tally.finish()


def nested_call(site, ops, stats, M, dtype, bias, r, epilogue):
    """The nested twin of the site's entry point on double-quantised statistics, into a guarded output: [B, M or M / 2]."""
    B, K, fam = site.B, site.K, site.fam
    q, nested, code, offset = stats
    width = M // 2 if epilogue == GATED else M
    buf, into = C.guarded(B * width, dtype, GUARD, dev())
    x, P, out = ops["x"], ops["P"], into.view(B, width)
    with F4.forced(**fam.variants):
        if site.lora and site.batch:
            NBT.gemm_lora_nested(x, P, q, nested, code, offset, M, K, ops["lB"], ops["t"], bias, r, epilogue, out=out, bs=fam.bs)
        elif site.lora:
            NBT.gemv_lora_nested(x.reshape(-1), P, q, nested, code, offset, M, K, ops["lB"], ops["t"].reshape(-1), bias, r, epilogue, out=into, bs=fam.bs)
        elif site.batch:
            NBT.gemm_nested(x, P, q, nested, code, offset, M, K, bias, r, epilogue, out=out, bs=fam.bs)
        else:
            gemv_nested(x.reshape(-1), P, q, nested, code, offset, M, K, fam.bs, bias, r, epilogue, out=into)
    assert C.guards_intact(buf, B * width, GUARD)
    return out


def statistics(absmax):
    q, nested, code, offset = N4.C.tabled_statistics(absmax)
    return to_dev(q), to_dev(nested), to_dev(code), offset


NESTED_SITES = [s for s in NF4_SITES if s.gated]


@cases(NESTED_SITES, gated_only=True)
def test_nested_forms_equal_the_un_nested_form(site, dtype):
    """*_nested_nf4 / *_lora_nested_nf4 on the edge set, the unit scales held as double-quantised statistics (one table entry, unit
    group scales, no offset): the un-nested form's output."""
    M, ops, bias, res = edge_set_operands(site, dtype)
    stats = statistics(np.ones(M * site.K // site.fam.bs, np.float32))
    tally = Tally("nested", site, dtype)
    for epilogue, with_res in FORM_LAUNCHES:
        r = res[epilogue] if with_res else None
        out = nested_call(site, ops, stats, M, dtype, bias, r, epilogue)
        want = site.run(ops, M, dtype, bias=bias, residual=r, epilogue=epilogue)
        tally.add(vals(out), vals(want)[None], lambda i: ("batch row", i[0], "pair or row", i[-1]))
    tally.finish()


NESTED_GATE_VALUES = 200  # per launch: with the up values and the unit scale, fewer than the 256 entries of the statistics' table


@cases(NESTED_SITES, gated_only=True)
def test_nested_forms_sum_driven(site, dtype):
    """The sum-driven operands through the nested forms: the row's value is the scale of its first block, carried by the statistics
    (a table entry per distinct scale), under one +-1.0 code and a one-hot activation with another factor per batch row - ties,
    overflow of T, sums that round to -0, f32-subnormal sums.  The un-nested form's output on the expanded scales; the LoRA forms
    carry an all-zero adapter here and their un-nested output must also be the fused form's."""
    npd, B, K, bs = NPDT[dtype], site.B, site.K, site.fam.bs
    off = V.sum_row_scales(npd)
    ga = np.concatenate([V.values(V.finite(V.edge_patterns(npd), npd), npd), off, -off]).astype(np.float32)
    ua = V.values(V.finite(V.up_patterns(npd), npd), npd)
    sub, rb = V.bias_subset(npd), V.residual_patterns(npd)
    tally = Tally("nested sum-driven", site, dtype)
    for lo in range(0, ga.size, NESTED_GATE_VALUES):
        g = ga[lo:lo + NESTED_GATE_VALUES]
        n = g.size * ua.size
        M = 2 * n
        a = np.empty(M, np.float32)
        a[0::2], a[1::2] = np.repeat(g, ua.size), np.tile(ua, g.size)
        P, A = site.weight(M, a, through_weight=True)
        absmax = np.ones((M, K // bs), np.float32)
        absmax[:, 0] = np.abs(a)
        assert np.array_equal(A.cpu().numpy(), absmax.reshape(-1)) and np.unique(absmax).size <= 256
        stats = statistics(absmax)
        pair = np.arange(n)
        bias_bits = np.empty(M, np.uint16)
        bias_bits[0::2], bias_bits[1::2] = sub[(2 * pair + pair // 16) % 16], sub[(2 * pair + 1 + pair // 16) % 16]
        bias = t_of(bias_bits, dtype)
        res = {GATED: t_of(rb[(pair[None, :] + np.arange(B)[:, None]) % rb.size], dtype),
               NONE: t_of(rb[(np.arange(M)[None, :] + np.arange(B)[:, None]) % rb.size], dtype)}
        for s in batch_factors(site, dtype, through_weight=True):
            ops = dict(x=site.x(s, dtype, through_weight=True), P=P, A=A)
            if site.lora:
                ops["lB"], ops["t"] = site.adapter(M, dtype)
            describe = lambda i: ("row value", float(a[i[-1]]), "or pair of", float(a[min(2 * i[-1], M - 2)]), "factor", float(s[i[0]]))  # noqa: E731
            for epilogue, b, with_res in ((GATED, None, False), (GATED, bias, True), (NONE, bias, True)):
                r = res[epilogue] if with_res else None
                out = nested_call(site, ops, stats, M, dtype, b, r, epilogue)
                want = site.run(ops, M, dtype, bias=b, residual=r, epilogue=epilogue)
                tally.add(vals(out), vals(want)[None], describe)
                if site.lora:
                    base = site.run(ops, M, dtype, bias=b, residual=r, epilogue=epilogue, base_form=True)
                    tally.add(vals(want), vals(base)[None], describe)
    tally.finish()
