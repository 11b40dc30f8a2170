"""Shared by tests/test_gpu_layer_operands.py (real kernels) and tests/test_layer_operands_host.py (CPU doubles in strict mode): how
an activation is PRESENTED to a layer, how the ops a layer calls are observed, and the sweep that holds a layer to the contract
"an activation may be any contiguous view".

An operand's address belongs to the call, not to the layer.  The fused ops of the C ABI read the activation in 16-byte pieces and refuse
any other address; the Python layers above them decide per call which op an activation goes to.  The sweep presents every activation

* ``fresh``    - a fresh allocation (what every other test of the suite passes),
* ``aligned``  - a contiguous view at a non-zero 16-byte-aligned offset inside a larger buffer,
* ``off1`` / ``off4`` - contiguous views one and four elements past a 16-byte boundary (for f32 four elements are 16 bytes: that view is
  a second aligned one, and ``data_ptr() % 16`` is asserted to be 0 for it),

and asserts, per layer and presentation: (1) no exception; (2) values, through the ``check`` the caller passes; (3) where the recorded
route equals the fresh call's, the same bits; (4) no lasting effect - after the off-alignment calls a fresh-allocation call on the same
layer object records the route, and gives the bits, of a layer object that never saw anything but fresh allocations.

A recorded route is the sequence of (op name, whether the activation the op was handed sat on a 16-byte boundary).  The second half is
part of the route because the plain GEMV ops - which the layers hand any address, on purpose - choose their kernel by it (the generic
kernel accumulates in another order than the fast ones): same op and same alignment class is what makes two calls run the same kernel.
"""
from __future__ import annotations

import torch

MAIN = (128, 512)     # K % 512 == 0: the 1..16-row matrix-core kernels and the VALU kernel; 1024 blocks of 64 = four nested groups
ONEPASS = (64, 576)   # K % 64 only: the one-pass kernels; 576 blocks = two nested groups and a partial one
SHAPES = [MAIN, ONEPASS]
ROWS = [1, (1, 1), 2, 8, 16, 17, 40, 64]  # (1, 1): one row as a 3-D [1, 1, K] activation
ROWS_FP4_MORE = [65, 128]
ROWS_F32 = [1, (1, 1), 2, 8]              # the FP4 GEMV, and the FP4 switch up to 8 rows
PLACEMENTS = ("fresh", "aligned", "off1", "off4")
RANK = 16

# (blocksize, K): FP4 layers under small_batch_fused; the 16-bit op takes a power-of-two blocksize >= 32, dequant any even one
BLOCKSIZE_CASES = [(16, 64), (96, 192), (32, 96), (128, 512), (256, 512)]
BLOCKSIZE_ROWS = [2, 8]
BLOCKSIZE_M = 24


def fused_blocksize(bs: int) -> bool:
    return bs >= 32 and bs & (bs - 1) == 0


def n_rows(rows) -> int:
    return 1 if isinstance(rows, tuple) else rows


def x_shape(rows, K):
    return rows + (K,) if isinstance(rows, tuple) else (rows, K)


def offset_elems(how: str, esize: int) -> int:
    return {"aligned": 3 * 16 // esize, "off1": 1, "off4": 4}[how]


def placed(t: torch.Tensor, how: str) -> torch.Tensor:
    """``t``'s values as a contiguous tensor presented ``how`` (see the module docstring), on ``t``'s device."""
    if how == "fresh":
        v, want = t.clone(), 0
    else:
        off, n = offset_elems(how, t.element_size()), t.numel()
        buf = torch.zeros(n + 64, dtype=t.dtype, device=t.device)
        assert buf.data_ptr() % 16 == 0
        buf[off:off + n] = t.reshape(-1)
        v, want = buf[off:off + n].view(t.shape), off * t.element_size() % 16
        assert v.data_ptr() == buf.data_ptr() + off * t.element_size() and v.contiguous() is v
    assert v.is_contiguous() and v.data_ptr() % 16 == want, (how, v.data_ptr() % 16, want)
    return v


class Recorder:
    """Stands in for ``ext`` in a module of the package: notes (op name, activation on a 16-byte boundary) and forwards to the real op
    (or to a CPU double).  Attributes that are no ops - ``ScalarType``, the epilogue constants - pass through."""

    def __init__(self, real):
        self._real = real
        self.route = []

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if isinstance(attr, type) or not callable(attr):
            return attr

        def op(*args, **kwargs):
            x = next((a for a in args if torch.is_tensor(a)), None)
            self.route.append((name, x is None or x.data_ptr() % 16 == 0))
            return attr(*args, **kwargs)
        return op

    def take(self):
        r, self.route = tuple(self.route), []
        return r


def ops(route):
    return [name for name, _ in route]


def show(route) -> str:
    return " + ".join(name if aligned else name + "(x off 16 B)" for name, aligned in route) or "-"


def install(monkeypatch, real):
    """One Recorder over ``ext`` in the three modules that route activations."""
    from torch_bnb_fp4 import fused, nested, quant_data

    rec = Recorder(real)
    for mod in (quant_data, fused, nested):
        monkeypatch.setattr(mod, "ext", rec)
    return rec


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    raw = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(raw), b.contiguous().view(raw)))


def random(shape, dtype, seed: int, device, scale: float = 1.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(device)


def sweep(rec, virgin, exposed, K, M_out, rows_list, dtype, device, residual=False, check=None, before=None, name=""):
    """Assertions 1..4 of the module docstring over ``rows_list`` x PLACEMENTS.  ``virgin`` only ever sees fresh allocations; ``exposed``
    is the same layer built a second time and sees every presentation.  ``check(rows, x, res, y, route)`` raises AssertionError or returns the
    worst |err| / tol; ``before(n)`` runs ahead of the calls at ``n`` rows (the adapter selection).  Returns (records, failures):
    a record is (rows, presentation, route, err/tol); nothing is raised here, so that one run names every failing cell."""
    records, failures = [], []

    def call(layer, x, res):
        rec.take()  # a check may have run layers of its own through the proxy
        return layer(x, residual=res) if residual else layer(x)

    def values(rows, how, x, res, y, route):
        ratio = None
        if check is not None:
            try:
                ratio = check(rows, x, res, y, route)
            except AssertionError as exc:
                failures.append(f"2 values | {name} | rows {rows} | {how} | {show(route)} | {str(exc)[:200]}")
        records.append((rows, how, route, ratio))

    for i, rows in enumerate(rows_list):
        n = n_rows(rows)
        x = random(x_shape(rows, K), dtype, 1000 + 7 * i + n, device)
        res = random(x_shape(rows, M_out), dtype, 2000 + 7 * i + n, device) if residual else None
        if before is not None:
            before(n)
        y0 = call(virgin, placed(x, "fresh"), None if res is None else placed(res, "fresh"))
        r0 = rec.take()
        assert tuple(y0.shape) == x_shape(rows, M_out) and y0.dtype == dtype
        values(rows, "fresh", x, res, y0, r0)
        for how in PLACEMENTS[1:]:
            try:  # the residual goes off alignment as well: every kernel reads it element-wise
                y = call(exposed, placed(x, how), None if res is None else placed(res, "off1"))
            except RuntimeError as exc:
                failures.append(f"1 no exception | {name} | rows {rows} | {how} | {show(rec.take())} | {str(exc)[:160]}")
                continue
            r = rec.take()
            values(rows, how, x, res, y, r)
            if r == r0 and not same_bits(y, y0):
                failures.append(f"3 bits | {name} | rows {rows} | {how} | {show(r)}")
        try:
            y1 = call(exposed, placed(x, "fresh"), None if res is None else placed(res, "fresh"))
        except RuntimeError as exc:
            failures.append(f"4 no lasting effect | {name} | rows {rows} | fresh again raised | {str(exc)[:160]}")
            rec.take()
            continue
        r1 = rec.take()
        records.append((rows, "fresh again", r1, None))
        if r1 != r0:
            failures.append(f"4 no lasting effect | {name} | rows {rows} | route {show(r0)} became {show(r1)}")
        elif not same_bits(y1, y0):
            failures.append(f"4 no lasting effect | {name} | rows {rows} | same route {show(r0)}, other bits")
    return records, failures


def report(name, dtype, records, failures, prefix="layer-operands"):
    """One line per (rows, presentation): the recorded route and the worst err/tol (profiles/layer_operands.txt keeps them)."""
    dt = str(dtype).replace("torch.", "")
    for rows, how, route, ratio in records:
        worst = "-" if ratio is None else f"{ratio:.3f}"
        print(f"{prefix} | {name} | {dt} | rows {rows} | {how} | {show(route)} | worst err/tol {worst}")
    for f in failures:
        print(f"{prefix} | FAIL | {dt} | {f}")
