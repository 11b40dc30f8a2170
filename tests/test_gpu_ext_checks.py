"""What the extension's 4-bit weight ops refuse before they launch anything, op by op, and that the checks leave good operands alone.

One table: every weight op of torch_bnb_fp4_ext x every mistake its signature allows -> (exception type, substring of the message).
The substrings are the ones the ops carried before their checks were gathered into one preamble (csrc/torch_ext.cpp: weight_op), so
the same-device rows of this file pass unchanged on the commit before it; where two ops worded one mistake differently the table
says so per op.  Each op's rows are followed by one valid call, compared with the C ABI entry point the op stands for (torch.equal).
No case hands a kernel bad operands: every mistake is one the host layer must catch.

Shapes are the smallest the ops accept: M = 16, K = 512, blocksize 64, bf16 for the batched ops; K = 64 for the batch-1 ops; rank 8
for LoRA; K = 1024 for the nested GEMV (M * K / 64 = 256 blocks, one whole group of 256).

The cross-device rows (an operand on a second GPU) are NEW behaviour of the preamble - before it only some ops looked at B's and
absmax's device and none at the bias's - and need two GPUs."""
import functools

import pytest
import torch

import hipabi
from gpu_util import dev
from test_gpu_nested import gemv_nested, nested_weight, table_dev
from test_gpu_nf4_fused import GATED, NONE, gemm_fused, gemv_fused, rand, weight
from test_gpu_nf4_lora import down, gemm_lora, gemv_lora
from test_gpu_nf4_small_batch import gemm as gemm_small_nf4
from test_gpu_nf4_wide_batch import gemm as gemm_wide_nf4

pytestmark = pytest.mark.gpu
BS, M, RANK = 64, 16, 8
DT, OTHER16 = torch.bfloat16, torch.float16


class Op:
    """One op of the extension: its operands by name in the order of its signature, its row limit, and which mistakes of the table
    are worded differently by it on the commit before the shared preamble (``wording``: mistake -> substring)."""

    def __init__(self, name, order, K, rows, max_rows, reference, wording=None, absmax="absmax"):
        self.name, self.order, self.K, self.rows, self.max_rows, self.reference = name, order, K, rows, max_rows, reference
        self.wording, self.absmax = wording or {}, absmax

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def operands(self):
        """Valid operands, made once and only read (a mistake replaces one entry of a shallow copy)."""
        K, rows = self.K, self.rows
        if self.name == "gemv_nf4_nested":
            P, q, nested, offset, _ = nested_weight(M, K, BS)
            a = dict(absmax_u8=q, nested_absmax=nested, code=table_dev(), offset=offset, nested_blocksize=256)
        else:
            P, absmax = weight(M, K)
            a = dict(absmax=absmax)
        a.update(A=rand((rows, K), DT, 5 + rows, 2.0), B=P.reshape(-1, 1).t(), P=P, blocksize=BS, Bshape=[M, K])
        if "bias" in self.order:
            a["bias"] = rand(M, DT, 7, 0.1)
        if "residual" in self.order:
            a.update(residual=rand((rows, M), DT, 9), epilogue=NONE)
        if "lora_B" in self.order:
            lA, a["lora_B"] = rand((RANK, K), DT, 11, K ** -0.5), rand((M, RANK), DT, 12, 0.05)
            a["t"] = down(a["A"], lA, torch.full((RANK,), 2.0, device=dev()))
        return a

    def __call__(self, a):
        import torch_bnb_fp4 as pkg

        return getattr(pkg.ext, self.name)(*[a[k] for k in self.order])


PLAIN = ("A", "B", "absmax", "blocksize", "Bshape", "bias")
FUSED = PLAIN + ("residual", "epilogue")
LORA = FUSED + ("lora_B", "t")
NESTED = ("A", "B", "absmax_u8", "nested_absmax", "code", "offset", "nested_blocksize", "blocksize", "Bshape", "bias", "residual", "epilogue")


def _flat(a, *names):
    return [None if a.get(n) is None else a[n].reshape(-1) for n in names]


OPS = [
    Op("gemv_fp4_fused", FUSED, 64, 1, 1,
       lambda a: hipabi.gemv_fused(a["A"].reshape(-1), a["P"], a["absmax"], M, a["Bshape"][1], BS, *_flat(a, "bias", "residual"), a["epilogue"]).reshape(1, -1),
       {"int8 B": "uint8", "B one byte short": "B holds"}),
    Op("gemm_small_fp4", PLAIN, 512, 4, 128, lambda a: hipabi.gemm_small(a["A"], a["P"], a["absmax"], M, a["Bshape"][1], BS, a["bias"])),
    Op("gemm_small_fp4_fused", FUSED, 512, 4, 128,
       lambda a: hipabi.gemm_small_fused(a["A"], a["P"], a["absmax"], M, a["Bshape"][1], BS, a["bias"], a["residual"], a["epilogue"])),
    Op("gemm_small_nf4", PLAIN, 512, 4, 16, lambda a: gemm_small_nf4(a["A"], a["P"], a["absmax"], M, a["Bshape"][1], a["bias"])),
    Op("gemm_wide_nf4", PLAIN, 512, 4, 128, lambda a: gemm_wide_nf4(a["A"], a["P"], a["absmax"], M, a["Bshape"][1], a["bias"])),
    Op("gemv_nf4_fused", FUSED, 64, 1, 1,
       lambda a: gemv_fused(a["A"].reshape(-1), a["P"], a["absmax"], M, a["Bshape"][1], BS, *_flat(a, "bias", "residual"), a["epilogue"]).reshape(1, -1),
       {"last dim is not K": "in_features"}),
    Op("gemm_nf4_fused", FUSED, 512, 4, 128,
       lambda a: gemm_fused(a["A"], a["P"], a["absmax"], M, a["Bshape"][1], BS, a["bias"], a["residual"], a["epilogue"])),
    Op("gemv_nf4_lora", LORA, 64, 1, 1,
       lambda a: gemv_lora(a["A"].reshape(-1), a["P"], a["absmax"], M, a["Bshape"][1], a["lora_B"], a["t"], BS, *_flat(a, "bias", "residual"),
                           a["epilogue"]).reshape(1, -1),
       {"last dim is not K": "in_features"}),
    Op("gemm_nf4_lora", LORA, 512, 4, 128,
       lambda a: gemm_lora(a["A"], a["P"], a["absmax"], M, a["Bshape"][1], a["lora_B"], a["t"], BS, a["bias"], a["residual"], a["epilogue"])),
    Op("gemv_nf4_nested", NESTED, 1024, 1, 1,
       lambda a: gemv_nested(a["A"].reshape(-1), a["P"], a["absmax_u8"], a["nested_absmax"], a["code"], a["offset"], M, a["Bshape"][1], BS,
                             *_flat(a, "bias", "residual"), a["epilogue"]).reshape(1, -1),
       {"absmax one scale short": "absmax_u8 holds"}, absmax="absmax_u8"),
    Op("gemv_fp4_partial", PLAIN[:-1], 64, 1, 1,
       lambda a: hipabi.gemv_partial(a["A"].reshape(-1), a["P"], a["absmax"], M, a["Bshape"][1], BS).reshape(1, -1)),
]


def _noncontiguous(t):
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    return wide[..., ::2]


# mistake -> (which ops it applies to, the operands with the mistake made, the message's substring unless the op words it otherwise)
MISTAKES = {
    "non-contiguous A": (lambda op: True, lambda op, a: dict(a, A=_noncontiguous(a["A"])), "contiguous"),
    "a CPU tensor": (lambda op: True, lambda op, a: dict(a, B=a["B"].cpu()), "must be a CUDA tensor"),
    "int8 B": (lambda op: True, lambda op, a: dict(a, B=a["B"].view(torch.int8)), "too small"),
    "B one byte short": (lambda op: True, lambda op, a: dict(a, B=a["P"][:-1].reshape(1, -1)), "too small"),
    "absmax one scale short": (lambda op: True, lambda op, a: dict(a, **{op.absmax: a[op.absmax][:-1]}), "too small"),
    "last dim is not K": (lambda op: True, lambda op, a: dict(a, A=rand((op.rows, op.K + 64), DT, 1)),
                          lambda op: "batch-1" if op.max_rows == 1 else "last dim"),
    "one row over the limit": (lambda op: op.max_rows > 1, lambda op, a: dict(a, A=rand((op.max_rows + 1, op.K), DT, 1)),
                               lambda op: f"covers 1..{op.max_rows}"),
    "two rows into a batch-1 op": (lambda op: op.max_rows == 1, lambda op, a: dict(a, A=rand((2, op.K), DT, 1)), "batch-1"),
    "bias of m - 1 elements": (lambda op: "bias" in op.order, lambda op, a: dict(a, bias=a["bias"][:-1]), "bias must"),
    "bias of the other 16-bit dtype": (lambda op: "bias" in op.order, lambda op, a: dict(a, bias=a["bias"].to(OTHER16)), "bias must"),
    "residual of the wrong numel": (lambda op: "residual" in op.order, lambda op, a: dict(a, residual=a["residual"].reshape(-1)[:-1]),
                                    "residual must hold"),
    "epilogue 7": (lambda op: "epilogue" in op.order, lambda op, a: dict(a, epilogue=7), "unknown epilogue"),
}


def rows_of(op):
    for mistake, (applies, make, substring) in MISTAKES.items():
        if applies(op):
            want = op.wording.get(mistake) or (substring(op) if callable(substring) else substring)
            yield mistake, make, RuntimeError, want


@pytest.mark.parametrize("op", OPS, ids=repr)
def test_every_mistake_is_refused_and_good_operands_reach_the_c_abi_untouched(op):
    good = op.operands()
    before = {k: v.clone() for k, v in good.items() if torch.is_tensor(v)}
    seen = 0
    for mistake, make, exc, substring in rows_of(op):
        with pytest.raises(exc) as info:
            op(make(op, dict(good)))
        assert substring in str(info.value), (op, mistake, substring, str(info.value))
        seen += 1
    assert seen >= 7, (op, seen)  # the table reached this op
    # the checks did not eat the operands: the same tensors still give the C ABI's bits, with every optional operand present
    for epilogue in (NONE, GATED) if "epilogue" in op.order else (NONE,):
        a = dict(good)
        if "epilogue" in op.order:
            a.update(epilogue=epilogue, residual=good["residual"][:, :M // 2].contiguous() if epilogue == GATED else good["residual"])
        got = op(a)
        assert torch.equal(got, op.reference(a).reshape(got.shape)), (op, epilogue)
        assert got.shape == (op.rows, M // 2 if epilogue == GATED else M)
    assert all(torch.equal(good[k], v) for k, v in before.items())


def test_the_table_covers_every_weight_op_of_the_extension():
    """Every exported op that takes a packed weight and its Bshape is in OPS (gemv_fp4 / gemv_nf4 and their *_bias forms reproduce
    the reference's own checks and are covered by tests/test_gpu_gemv.py and tests/test_gpu_nf4_gemv.py)."""
    import torch_bnb_fp4 as pkg

    takes_bshape = {n for n in dir(pkg.ext) if callable(getattr(pkg.ext, n)) and "Bshape" in (getattr(pkg.ext, n).__doc__ or "")}
    assert takes_bshape - {"gemv_fp4", "gemv_fp4_bias", "gemv_nf4", "gemv_nf4_bias"} == {op.name for op in OPS}


# ---- new behaviour: every operand on the activation's device ---------------------------------------------------------------------------
CROSS = [(op, name) for op in OPS for name in (("B", op.absmax) + tuple(n for n in ("bias", "residual", "lora_B", "t") if n in op.order))]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU to put an operand on")
@pytest.mark.parametrize("op,name", CROSS, ids=[f"{op}-{name}" for op, name in CROSS])
def test_new_an_operand_on_another_device_is_refused(op, name):
    good = op.operands()
    with pytest.raises(RuntimeError, match="device"):
        op(dict(good, **{name: good[name].to(torch.device("cuda", 1))}))
