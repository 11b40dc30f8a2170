"""Decode-step epilogue fusion on top of the reference's Linear surface.

The reference's op surface stops at the Linear: a decoder layer then pays separate launches for ``silu(gate(h)) * up(h)``
and for each residual add - where the reference itself already pays one for the bias (torch_bnb_fp4/__init__.py:603-613).
At batch 1 every one of those launches is a ~1.5 us kernel boundary next to GEMVs of 3-9 us, so they are folded into the
GEMV's epilogue (``fp4_hip_gemv_fused``):

* :class:`FusedFP4Linear` ``(x, residual=None)`` -> ``residual + Linear(x)`` in one launch;
* :meth:`FusedFP4Linear.gate_up` interleaves the rows of a gate and an up projection (rows of an FP4 weight are
  independent, so this is a row permutation of bytes and scales done once) and returns a layer computing
  ``silu(gate(x)) * up(x)`` in one launch.

Every intermediate is rounded to the activation dtype exactly where the separate torch ops would round it, so the result
equals the unfused sequence bit for bit (``exp`` is the device library's, as in torch's silu).  2..128 activation rows
(batched decode) take the same epilogues on the small-batch kernels (``fp4_hip_gemm_small_fused``); larger inputs, or shapes
the fused kernels do not cover, run the unfused sequence through :class:`QuantData`.

:class:`FusedNF4Linear` is the same layer over an NF4 weight (``fp4_hip_gemv_fused_nf4`` for one row,
``fp4_hip_gemm_fused_nf4`` for 2..64 rows); :class:`FusedFP4Linear` itself refuses NF4 weights.

:class:`LoRANF4Linear` is a :class:`FusedNF4Linear` with a LoRA adapter beside the 4-bit weight (QLoRA serving: the adapter cannot
be merged into NF4 without re-quantising): ``y = W x + B (s * A x)`` as two launches, the down projection ``t = s * A x`` in f32
(``fp4_hip_lora_down``) and the same fused kernels with ``B t`` added to their f32 row sums before the rounding
(``fp4_hip_gemv_lora_nf4`` / ``fp4_hip_gemm_lora_nf4``).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
from torch import nn

from ._ext import ext
from .nn import QuantState, fp4_code, nf4_code
from .quant_data import QuantData, aligned16, small_fp4_covers

EPILOGUE_NONE = 0
EPILOGUE_SILU_MUL_PAIRS = 1


def interleave_rows(a: Tuple[torch.Tensor, torch.Tensor], b: Tuple[torch.Tensor, torch.Tensor], shape: Sequence[int], blocksize: int
                    ) -> Tuple[torch.Tensor, torch.Tensor, Tuple[int, int]]:
    """Rows ``a0, b0, a1, b1, ...`` of two FP4 weights of the same ``[M, K]`` shape as one ``[2M, K]`` weight
    (``(packed, absmax)`` each).  ``K % blocksize == 0``, so a row is a contiguous run of bytes and of scales."""
    M, K = int(shape[0]), int(shape[1])
    if K % blocksize or K % 2:
        raise ValueError(f"interleave_rows needs in_features ({K}) divisible by the blocksize ({blocksize})")
    (pa, sa), (pb, sb) = a, b
    if pa.numel() != M * K // 2 or pb.numel() != M * K // 2 or sa.numel() != M * K // blocksize or sb.numel() != M * K // blocksize:
        raise ValueError("interleave_rows: both weights must have the given [M, K] shape")
    packed = torch.stack([pa.reshape(M, K // 2), pb.reshape(M, K // 2)], dim=1).reshape(-1, 1)
    absmax = torch.stack([sa.reshape(M, K // blocksize), sb.reshape(M, K // blocksize)], dim=1).reshape(-1)
    return packed, absmax, (2 * M, K)


def deinterleave_rows(packed: torch.Tensor, absmax: torch.Tensor, shape: Sequence[int], blocksize: int):
    """Inverse of :func:`interleave_rows`: the even rows and the odd rows of a ``[2M, K]`` FP4 weight as two ``[M, K]`` weights,
    ``((packed_a, absmax_a), (packed_b, absmax_b), (M, K))`` - what a checkpoint in bitsandbytes' layout stores for a gate and an
    up projection."""
    M2, K = int(shape[0]), int(shape[1])
    if M2 % 2 or K % blocksize or K % 2:
        raise ValueError(f"deinterleave_rows needs an even row count and in_features ({K}) divisible by the blocksize ({blocksize})")
    p = packed.reshape(M2 // 2, 2, K // 2)
    a = absmax.reshape(M2 // 2, 2, K // blocksize)
    return ((p[:, 0].reshape(-1, 1).contiguous(), a[:, 0].reshape(-1).contiguous()),
            (p[:, 1].reshape(-1, 1).contiguous(), a[:, 1].reshape(-1).contiguous()), (M2 // 2, K))


class FusedFP4Linear(nn.Module):
    """An FP4 Linear whose single-token path runs ``fp4_hip_gemv_fused``.

    ``epilogue == EPILOGUE_NONE``: ``forward(x, residual=None)`` = ``Linear(x) (+ residual)``.
    ``epilogue == EPILOGUE_SILU_MUL_PAIRS``: the weight holds interleaved gate / up rows, ``forward(x)`` =
    ``silu(gate(x)) * up(x)`` with ``out_features`` = half the weight's rows."""

    quant_type = "fp4"  # the code this class's kernels decode; a weight of the other code is refused

    @classmethod
    def _check_code(cls, *quant_datas) -> None:
        for qd in quant_datas:
            if getattr(qd, "quant_type", "fp4") != cls.quant_type:
                raise ValueError(f"{cls.__name__} runs the {cls.quant_type.upper()} fused-epilogue kernels; an "
                                 f"{getattr(qd, 'quant_type', 'fp4').upper()} weight cannot be decoded by them")

    @classmethod
    def _code(cls) -> torch.Tensor:
        return fp4_code()

    def __init__(self, quant_data: QuantData, epilogue: int = EPILOGUE_NONE):
        super().__init__()
        if epilogue not in (EPILOGUE_NONE, EPILOGUE_SILU_MUL_PAIRS):
            raise ValueError(f"unknown epilogue {epilogue}")
        self._check_code(quant_data)
        if epilogue == EPILOGUE_SILU_MUL_PAIRS and quant_data.M % 2:
            raise ValueError("the gate|up epilogue needs an even number of weight rows")
        self.quant_data = quant_data
        self.epilogue = epilogue
        self.in_features = int(quant_data.N)
        self.out_features = int(quant_data.M) // (2 if epilogue == EPILOGUE_SILU_MUL_PAIRS else 1)
        self._fused_ok = True  # cleared the first time the kernel reports the shape as not covered
        self._small_ok = True
        self.register_buffer("qweight", quant_data.A, persistent=True)
        self.register_buffer("absmax", quant_data.absmax, persistent=True)
        self.register_buffer("bias", None if quant_data.bias is None else quant_data.bias.detach(), persistent=True)

    # -- constructors ------------------------------------------------------------------------------------------------
    @classmethod
    def from_packed(cls, packed, absmax, shape, blocksize: int = 64, bias: Optional[torch.Tensor] = None,
                    epilogue: int = EPILOGUE_NONE, dtype: torch.dtype = torch.float16) -> "FusedFP4Linear":
        """``dtype``: the dtype the weight was quantised from (checkpoint metadata only; the kernels follow the activation)."""
        state = QuantState(absmax, shape, cls._code().to(packed.device), blocksize, dtype, cls.quant_type)
        return cls(QuantData(packed, state, state.shape, original_lin=None, bias=bias), epilogue)

    @classmethod
    def gate_up_from_packed(cls, gate, up, shape, blocksize: int = 64, gate_bias: Optional[torch.Tensor] = None,
                            up_bias: Optional[torch.Tensor] = None) -> "FusedFP4Linear":
        """``gate`` / ``up``: ``(packed, absmax)`` of two ``[M, K]`` projections -> one layer computing silu(gate(x)) * up(x)."""
        packed, absmax, full = interleave_rows(gate, up, shape, blocksize)
        if (gate_bias is None) != (up_bias is None):
            raise ValueError("gate and up must both carry a bias or neither")
        bias = None if gate_bias is None else torch.stack([gate_bias.reshape(-1), up_bias.reshape(-1)], dim=1).reshape(-1)
        return cls.from_packed(packed, absmax, full, blocksize, bias, EPILOGUE_SILU_MUL_PAIRS)

    @classmethod
    def from_linear(cls, layer) -> "FusedFP4Linear":
        """From a :class:`TorchFP4Linear` (shares its packed weight)."""
        qd = layer.quant_data
        cls._check_code(qd)
        return cls.from_packed(qd.A, qd.absmax, (qd.M, qd.N), qd.blocksize, qd.bias, dtype=getattr(qd.quant_state, "dtype", torch.float16))

    @classmethod
    def gate_up(cls, gate_layer, up_layer) -> "FusedFP4Linear":
        """From the gate and up :class:`TorchFP4Linear` of a gated MLP."""
        g, u = gate_layer.quant_data, up_layer.quant_data
        cls._check_code(g, u)
        if (g.M, g.N, g.blocksize) != (u.M, u.N, u.blocksize):
            raise ValueError("gate_up() needs two projections of the same shape and blocksize")
        return cls.gate_up_from_packed((g.A, g.absmax), (u.A, u.absmax), (g.M, g.N), g.blocksize, g.bias, u.bias)

    def _apply(self, fn, recurse=True):
        # Only device moves are honoured, exactly as in TorchFP4Linear._apply: the packed bytes and the f32 scales never
        # change dtype.  (nn.Module._apply would run model.half() / .to(torch.bfloat16) over the registered buffers and
        # round absmax to 16 bits - silently degraded scales in the running layer and in state_dict().)
        probe = fn(torch.empty(0, dtype=torch.float16, device=self.qweight.device))
        if probe.device != self.qweight.device:
            mv = lambda t: None if t is None else t.to(probe.device)
            for name in ("qweight", "absmax", "bias"):
                self._buffers[name] = mv(self._buffers[name])
            qd = self.quant_data
            qd.rebind(self.qweight, self.absmax, qd.code.to(probe.device), self.bias)
            self._buffers["absmax"] = qd.absmax
            if qd.bias is not None:
                self._buffers["bias"] = qd.bias
        return self

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self.quant_data.rebind(self.qweight, self.absmax, self.quant_data.code, self.bias)

    # -- forward -----------------------------------------------------------------------------------------------------
    def _unfused(self, x: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
        y = self.quant_data.forward(x)
        if self.epilogue == EPILOGUE_SILU_MUL_PAIRS:
            y = nn.functional.silu(y[..., 0::2]) * y[..., 1::2]
        return y if residual is None else y + residual

    # forward()'s ladder is this class's alone; a subclass over another code names its two ops and says what its batched op covers
    _gemv_op = "gemv_fp4_fused"
    _batched_op = "gemm_small_fp4_fused"

    def _batched_covers(self, rows: int, K: int, dtype: torch.dtype) -> bool:
        return small_fp4_covers(rows, K, self.quant_data.blocksize, dtype)

    def _gemv_wants_alignment(self) -> bool:
        """Whether the GEMV op refuses an activation off a 16-byte boundary (then it gets a copy).  ``fp4_hip_gemv_fused`` refuses it for
        gate|up only: with the plain epilogue it runs its generic kernel on any address, and keeps doing so."""
        return self.epilogue == EPILOGUE_SILU_MUL_PAIRS

    def _residual_in_kernel(self, rows: int, K: int) -> bool:
        """Whether the batched op adds the residual itself; where it does not, torch adds it to the op's output - T(t + r) either way."""
        return True

    def _fix_compute_dtype(self, x: torch.Tensor) -> None:
        qd = self.quant_data
        if not qd.compute_dtype_set and x.numel():
            qd.set_compute_type(x)
            if qd.bias is not None:
                self._buffers["bias"] = qd.bias  # the buffer follows the cast to the compute dtype

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        qd = self.quant_data
        K = x.shape[-1]
        self._fix_compute_dtype(x)
        if (self._fused_ok and x.numel() == K and K == self.in_features and x.ndim in (2, 3) and K % qd.blocksize == 0
                and x.dtype == qd.o_type):
            # an address belongs to the call: where the op would refuse it the call is made coverable, so that the refusals caught
            # below, which switch a route off for the life of the layer, are about the shape alone
            if self._gemv_wants_alignment():
                x = aligned16(x)
            elif not x.is_contiguous():
                x = x.contiguous()
            try:
                return getattr(ext, self._gemv_op)(x, qd._B_t, qd.absmax, qd.blocksize, qd._shape_list, qd.bias, residual, self.epilogue)
            except RuntimeError as exc:
                if "not available" not in str(exc):
                    raise
                self._fused_ok = False  # shape outside the fused kernel's coverage: unfused sequence from now on
        rows = x.numel() // K if K else 0
        if self._small_ok and K == self.in_features and x.dtype == qd.o_type and self._batched_covers(rows, K, x.dtype):
            in_kernel = residual is not None and self._residual_in_kernel(rows, K)
            try:  # batched decode: the same epilogues on the small-batch kernels
                y = getattr(ext, self._batched_op)(aligned16(x), qd._B_t, qd.absmax, qd.blocksize, qd._shape_list, qd.bias,
                                                   residual if in_kernel else None, self.epilogue)
                return y if in_kernel or residual is None else y + residual
            except RuntimeError as exc:
                if "not covered" not in str(exc):
                    raise
                self._small_ok = False
        return self._unfused(x, residual)

    def extra_repr(self) -> str:
        kind = "silu(gate)*up" if self.epilogue == EPILOGUE_SILU_MUL_PAIRS else "linear(+residual)"
        return f"in_features={self.in_features}, out_features={self.out_features}, epilogue={kind}"


class FusedNF4Linear(FusedFP4Linear):
    """:class:`FusedFP4Linear` over an NF4 weight: same constructors and ``forward(x, residual=None)``.

    One activation row runs ``fp4_hip_gemv_fused_nf4``; 2..64 rows of fp16 / bf16 against a blocksize-64 weight with
    ``K % 64 == 0`` run ``fp4_hip_gemm_fused_nf4`` (the range in which the one-pass NF4 kernels are ahead of dequant + GEMM,
    profiles/nf4_wide_batch.json); everything else, 65+ rows included, runs the unfused sequence through :class:`QuantData`
    and torch's silu / mul / add.  An op that reports a shape as not covered is not tried again.  One measured cell is left out
    of the fused residual add: more than 32 rows against rows of 8192 and more weights with the plain epilogue (a down
    projection; profiles/nf4_fused_epilogues.json: 55.5 vs 56.5 us at 64 rows, inside the replay-to-replay ranges) - there the
    op runs without the residual and torch adds it, the same bits."""

    quant_type = "nf4"

    @classmethod
    def _code(cls) -> torch.Tensor:
        return nf4_code()

    _gemv_op = "gemv_nf4_fused"
    _batched_op = "gemm_nf4_fused"

    def _batched_covers(self, rows: int, K: int, dtype: torch.dtype) -> bool:
        return 2 <= rows <= 64 and dtype in (torch.float16, torch.bfloat16) and self.quant_data.blocksize == 64 and K % 64 == 0

    def _gemv_wants_alignment(self) -> bool:
        return True  # fp4_hip_gemv_fused_nf4 has no generic kernel behind it: either epilogue refuses an address off 16 bytes

    def _residual_in_kernel(self, rows: int, K: int) -> bool:
        # the one cell in which the fused residual add measured no gain (profiles/nf4_fused_epilogues.json): more than 32 rows against
        # rows of 8192 and more weights with the plain epilogue - there the add stays torch's
        return not (self.epilogue == EPILOGUE_NONE and rows > 32 and K >= 8192)


LORA_RANK_MULTIPLE = 8  # the kernels read B and t in 16-byte units
LORA_MAX_RANK = 256


def lora_fused_ahead(rows: int, M: int, K: int, rank: int) -> bool:
    """Where ``lora_down`` + the fused adapter op measured ahead of the fused NF4 op plus the adapter as torch ops by more than both
    replay-to-replay ranges together (profiles/nf4_lora.json: Mistral-7B shapes, ranks 16..256, 1..64 rows, bf16 and fp16).  One
    row: every cell.  2..64 rows: the per-thread FMA chain over the rank in the store loops grows with ``M * rows * rank`` while
    torch's two dense products hardly do, so each rank band is trusted up to the largest ``M * rows * rank`` at which all of its
    measured cells were ahead; past it cells were level or behind (28672 x 4096, rank 64, 64 rows: 138 vs 115 us; rank 256: 315 vs
    125).  Against rows of 14336 weights torch's ``x @ A^T`` is slow and every cell was ahead, up to 4096 * 64 * 256."""
    if rows == 1:
        return True
    if K >= 14336:
        limit = 4096 * 64 * 256
    elif rank <= 32:
        limit = 14336 * 64 * 32
    elif rank <= 128:
        limit = 4096 * 64 * 64
    else:
        limit = 4096 * 8 * 256
    return M * rows * rank <= limit


def pad_adapter(lora_A: torch.Tensor, lora_B: torch.Tensor, scale: torch.Tensor):
    """Zero rows of A, zero columns of B and zero factors up to the next multiple of 8 of the rank.  Exact: a padded row of A gives
    t = 0 and a padded column of B multiplies it by 0."""
    r = lora_A.shape[0]
    pad = -r % LORA_RANK_MULTIPLE
    if pad:
        lora_A = torch.cat([lora_A, lora_A.new_zeros(pad, lora_A.shape[1])], 0)
        lora_B = torch.cat([lora_B, lora_B.new_zeros(lora_B.shape[0], pad)], 1)
        scale = torch.cat([scale, scale.new_zeros(pad)], 0)
    return lora_A.contiguous(), lora_B.contiguous(), scale.contiguous()


def stack_gate_up_adapters(gate_adapter, up_adapter):
    """``(A, B, scaling)`` of a gate and an up projection -> one adapter over the row-interleaved gate|up weight: A stacked to
    ``[r_g + r_u, K]``, B block-structured and row-interleaved like the weight (row 2i = ``[B_gate[i], 0]``, row 2i + 1 =
    ``[0, B_up[i]]``), one scale per adapter row."""
    (Ag, Bg, sg), (Au, Bu, su) = gate_adapter, up_adapter
    if Bg.shape[0] != Bu.shape[0] or Ag.shape[1] != Au.shape[1] or Ag.shape[0] != Bg.shape[1] or Au.shape[0] != Bu.shape[1]:
        raise ValueError("gate and up adapters must be (A [r, K], B [M, r]) pairs of two projections of the same [M, K] shape")
    rg, ru, M = Ag.shape[0], Au.shape[0], Bg.shape[0]
    A = torch.cat([Ag, Au.to(Ag)], 0)
    B = Bg.new_zeros(M, 2, rg + ru)
    B[:, 0, :rg] = Bg
    B[:, 1, rg:] = Bu.to(Bg)
    scale = torch.cat([torch.full((rg,), float(sg)), torch.full((ru,), float(su))]).to(device=Ag.device, dtype=torch.float32)
    return A, B.reshape(2 * M, rg + ru), scale


def lora_scaling(r: int, lora_alpha: float, use_rslora: bool = False) -> float:
    """peft's factor: ``alpha / r``, or ``alpha / sqrt(r)`` with rank-stabilised LoRA."""
    return float(lora_alpha) / (math.sqrt(r) if use_rslora else r)


class LoRAAdapterMixin:
    """One LoRA adapter held beside a 4-bit weight, shared by :class:`LoRANF4Linear` and
    :class:`~torch_bnb_fp4.nested.LoRANestedNF4Linear`: the buffers ``lora_A`` / ``lora_B`` / ``lora_scale`` padded to a multiple of 8
    (:func:`pad_adapter`), ``rank``, ``_lora_ok`` and the per-dtype casts."""

    def _init_adapter(self, lora_A: torch.Tensor, lora_B: torch.Tensor, scale, M: int, K: int, dev) -> None:
        if lora_A.ndim != 2 or lora_B.ndim != 2 or lora_A.shape[1] != K or lora_B.shape != (M, lora_A.shape[0]):
            raise ValueError(f"adapter shapes {tuple(lora_A.shape)} / {tuple(lora_B.shape)} do not fit a [{M}, {K}] weight (need A [r, K] "
                             "and B [M, r])")
        self.rank = int(lora_A.shape[0])
        if not torch.is_tensor(scale):
            scale = torch.full((self.rank,), float(scale))
        if scale.numel() != self.rank:
            raise ValueError(f"scale must be one factor or one per adapter row ({self.rank}), got {scale.numel()}")
        A, B, sc = pad_adapter(lora_A.detach().to(dev), lora_B.detach().to(dev), scale.detach().reshape(-1).to(device=dev, dtype=torch.float32))
        self.register_buffer("lora_A", A, persistent=True)
        self.register_buffer("lora_B", B, persistent=True)
        self.register_buffer("lora_scale", sc, persistent=True)
        self._lora_ok = A.shape[0] <= LORA_MAX_RANK  # cleared as well when lora_down reports a shape as not covered
        self._cast = {}  # activation dtype -> (A, B) in that dtype

    def _adapter(self, dtype: torch.dtype):
        # the adapter follows the activation dtype, as the bias does; the buffers stay as attached and every cast starts from them,
        # so a layer that meets two activation dtypes rounds the adapter once for each, never twice in a row
        if self.lora_A.dtype == dtype:
            return self.lora_A, self.lora_B
        cast = self._cast.get(dtype)
        if cast is None or cast[0].device != self.lora_A.device:
            cast = self._cast[dtype] = (self.lora_A.to(dtype), self.lora_B.to(dtype))
        return cast

    def _adapter_delta(self, x: torch.Tensor) -> torch.Tensor:
        """The adapter term in torch, in f32: ``(x.float() @ A.float().T * scale) @ B.float().T``."""
        A, B = self._adapter(x.dtype)
        return (x.float() @ A.float().t() * self.lora_scale) @ B.float().t()


class LoRANF4Linear(LoRAAdapterMixin, FusedNF4Linear):
    """A :class:`FusedNF4Linear` with a LoRA adapter: ``forward(x, residual=None)`` = epilogue of ``W x + B (s * A x)``.

    ``lora_A`` is ``[r, K]``, ``lora_B`` ``[M, r]`` over the weight's own rows (``M`` = all rows of an interleaved gate|up weight),
    ``scale`` a float or a float32 ``[r]`` tensor (one factor per adapter row).  Any rank works: A, B and the scales are zero-padded
    to a multiple of 8 here, which is exact.  The adapter follows the activation dtype (cast once per dtype from the tensors as attached).  Dropout is a
    training-time device; this layer is inference-only and has none.

    One activation row runs ``lora_down`` + ``gemv_nf4_lora``, 2..64 rows ``lora_down`` + ``gemm_nf4_lora``: the adapter term joins
    the f32 row sum before anything is rounded, one rounding fewer than peft's sequence.  Whatever the fused ops do not cover (65+
    rows, ranks above 256, shapes the NF4 fused kernels refuse), and the 2..64-row cells in which they did not measure ahead
    (:func:`lora_fused_ahead`: large ``M * rows * rank``), runs the base through the parent's kernels and the adapter in torch
    in f32, ``(x.float() @ A.float().T * scale) @ B.float().T``, added before one cast."""

    def __init__(self, quant_data: QuantData, epilogue: int, lora_A: torch.Tensor, lora_B: torch.Tensor, scale):
        super().__init__(quant_data, epilogue)
        self._init_adapter(lora_A, lora_B, scale, int(quant_data.M), self.in_features, self.qweight.device)

    # -- constructors ------------------------------------------------------------------------------------------------
    @classmethod
    def from_fused(cls, layer: FusedNF4Linear, lora_A, lora_B, scale) -> "LoRANF4Linear":
        """From a :class:`FusedNF4Linear` (shares its packed weight); ``lora_B`` covers the weight's own (interleaved) rows."""
        cls._check_code(layer.quant_data)
        return cls(layer.quant_data, layer.epilogue, lora_A, lora_B, scale)

    @classmethod
    def from_linear(cls, layer, lora_A, lora_B, scaling) -> "LoRANF4Linear":
        """From an NF4 :class:`TorchFP4Linear` (shares its packed weight) and one adapter."""
        return cls.from_fused(FusedNF4Linear.from_linear(layer), lora_A, lora_B, scaling)

    @classmethod
    def gate_up(cls, gate_layer, up_layer, gate_adapter, up_adapter) -> "LoRANF4Linear":
        """From the gate and up :class:`TorchFP4Linear` of a gated MLP and their ``(A, B, scaling)`` adapters."""
        return cls.gate_up_from_fused(FusedNF4Linear.gate_up(gate_layer, up_layer), gate_adapter, up_adapter)

    @classmethod
    def gate_up_from_fused(cls, layer: FusedNF4Linear, gate_adapter, up_adapter) -> "LoRANF4Linear":
        if layer.epilogue != EPILOGUE_SILU_MUL_PAIRS:
            raise ValueError("gate_up_from_fused() needs a gate|up layer (FusedNF4Linear.gate_up)")
        return cls.from_fused(layer, *stack_gate_up_adapters(gate_adapter, up_adapter))

    @classmethod
    def from_packed(cls, *args, **kwargs):
        raise TypeError("LoRANF4Linear needs an adapter: build a FusedNF4Linear.from_packed(...) and pass it to from_fused()")

    @classmethod
    def gate_up_from_packed(cls, *args, **kwargs):
        raise TypeError("LoRANF4Linear needs adapters: build a FusedNF4Linear.gate_up_from_packed(...) and pass it to gate_up_from_fused()")

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)  # device moves only
        for name in ("lora_A", "lora_B", "lora_scale"):
            self._buffers[name] = self._buffers[name].to(self.qweight.device)
        self._cast = {}
        return self

    # -- forward -----------------------------------------------------------------------------------------------------
    def _adapter_in_torch(self, x: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
        delta = self._adapter_delta(x)
        if self.epilogue == EPILOGUE_SILU_MUL_PAIRS:
            y = (self.quant_data.forward(x).float() + delta).to(x.dtype)
            y = nn.functional.silu(y[..., 0::2]) * y[..., 1::2]
        else:
            y = (FusedNF4Linear.forward(self, x).float() + delta).to(x.dtype)
        return y if residual is None else y + residual

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        qd = self.quant_data
        K = x.shape[-1]
        self._fix_compute_dtype(x)
        rows = x.numel() // K if K else 0
        if self._lora_ok and rows >= 1 and K == self.in_features and x.dtype == qd.o_type and K % qd.blocksize == 0:
            one = rows == 1 and x.ndim in (2, 3) and self._fused_ok
            many = (2 <= rows <= 64 and self._small_ok and x.dtype in (torch.float16, torch.bfloat16) and qd.blocksize == 64
                    and K % 64 == 0)
            if (one or many) and lora_fused_ahead(rows, int(qd.M), K, int(self.lora_A.shape[0])):
                A, B = self._adapter(x.dtype)
                x = aligned16(x)  # lora_down and both adapter ops read x in 16-byte pieces
                try:
                    t = ext.lora_down(x, A, self.lora_scale)
                except RuntimeError as exc:
                    if "not covered" not in str(exc):
                        raise
                    self._lora_ok = False
                    return self._adapter_in_torch(x, residual)
                # the parent's measured exception holds here as well (the store loop is the same one)
                in_kernel = residual is not None and self._residual_in_kernel(rows, K)
                try:
                    op = ext.gemv_nf4_lora if one else ext.gemm_nf4_lora
                    y = op(x, qd._B_t, qd.absmax, qd.blocksize, qd._shape_list, qd.bias, residual if in_kernel else None, self.epilogue, B, t)
                    return y if in_kernel or residual is None else y + residual
                except RuntimeError as exc:  # a refusal clears the flag of the op that refused, whatever its wording
                    if "not available" not in str(exc) and "not covered" not in str(exc):
                        raise
                    if one:
                        self._fused_ok = False  # outside the GEMV's fused coverage: the fallback from now on
                    else:
                        self._small_ok = False
        return self._adapter_in_torch(x, residual)

    def extra_repr(self) -> str:
        return super().extra_repr() + f", lora_rank={self.rank}"


# ---- several adapters in one batch, selected per row on the device ------------------------------------------------------------------
ADAPTER_SELECTION_CAPACITY = 64  # the rows the fused adapter ops cover; the torch fallback needs one id per row as well


class AdapterSelection:
    """Which adapter each sequence of the batch uses: one int32 device tensor of capacity 64, shared by all
    :class:`MultiLoRANF4Linear` layers of a model and read by their kernels on the device.

    ``set(ids)`` copies a host sequence or a tensor into it **in place** and records its length; ``-1`` (any value outside
    ``0 .. n_adapters - 1``) selects the bare base model for that row.  ``ids`` is the view ``forward`` uses.  The tensor is never
    reallocated after construction, so a step captured in a graph keeps reading it: ``set`` between two replays of the same length
    changes which sequence uses which adapter without a new capture.  ``names`` (optional) are the adapters' names in stack order for
    :meth:`set_by_name`.  The layers' torch fallback needs one id per row as well, so ``set`` with more ids than the capacity raises;
    a model that is also run at more than 64 rows (all of them on the fallback) builds its selection with a larger ``capacity``."""

    def __init__(self, device=None, names: Optional[Sequence[str]] = None, capacity: int = ADAPTER_SELECTION_CAPACITY):
        self._buf = torch.full((int(capacity),), -1, dtype=torch.int32, device=device)
        self._n = 0
        self.names = list(names) if names is not None else []

    @property
    def capacity(self) -> int:
        return int(self._buf.numel())

    @property
    def ids(self) -> torch.Tensor:
        return self._buf[: self._n]

    def __len__(self) -> int:
        return self._n

    def set(self, ids) -> "AdapterSelection":
        src = ids if torch.is_tensor(ids) else torch.tensor(list(ids), dtype=torch.int32)
        src = src.reshape(-1)
        if src.numel() > self.capacity:
            raise ValueError(f"AdapterSelection holds at most {self.capacity} ids (one per activation row), got {src.numel()}")
        if src.is_floating_point() or src.dtype == torch.bool:
            raise TypeError("adapter ids must be integers")
        n = int(src.numel())
        self._buf[:n].copy_(src)  # in place; converts to int32 and crosses devices as needed
        self._n = n
        return self

    def set_by_name(self, names: Sequence[Optional[str]]) -> "AdapterSelection":
        """``set`` with adapter names; ``None`` selects the base model only."""
        index = {name: i for i, name in enumerate(self.names)}
        unknown = [n for n in names if n is not None and n not in index]
        if unknown:
            raise KeyError(f"no adapter named {unknown[0]!r} (have {self.names})")
        return self.set([-1 if n is None else index[n] for n in names])

    def __repr__(self) -> str:
        return f"AdapterSelection(len={self._n}, capacity={self.capacity}, names={self.names})"


def pad_adapter_to(lora_A: torch.Tensor, lora_B: torch.Tensor, scale: torch.Tensor, rank: int):
    """:func:`pad_adapter` up to a given rank (zero rows of A, zero columns of B, zero factors): exact for the same reason."""
    pad = rank - lora_A.shape[0]
    if pad < 0:
        raise ValueError(f"cannot pad an adapter of rank {lora_A.shape[0]} to {rank}")
    if pad:
        lora_A = torch.cat([lora_A, lora_A.new_zeros(pad, lora_A.shape[1])], 0)
        lora_B = torch.cat([lora_B, lora_B.new_zeros(lora_B.shape[0], pad)], 1)
        scale = torch.cat([scale, scale.new_zeros(pad)], 0)
    return lora_A.contiguous(), lora_B.contiguous(), scale.contiguous()


class MultiLoRANF4Linear(FusedNF4Linear):
    """A :class:`FusedNF4Linear` with a stack of LoRA adapters and one adapter id per activation row, read on the device from an
    :class:`AdapterSelection`: row ``b`` of ``forward(x, residual=None)`` is what a :class:`LoRANF4Linear` holding adapter
    ``selection.ids[b]`` gives for that row, and what the bare :class:`FusedNF4Linear` gives where the id names no adapter.

    ``adapters`` is a list of ``(A [r_i, K], B [M, r_i], scale)`` as for :class:`LoRANF4Linear`.  They are zero-padded to one common
    rank - the largest rank rounded up to a multiple of 8 - which is exact, and stacked: ``lora_A_stack [n, R, K]``,
    ``lora_B_stack [n, M, R]``, ``lora_scale_stack [n, R]``.  The stacks follow the activation dtype, cast once per dtype.

    One activation row runs ``lora_down_multi`` + ``gemv_nf4_lora_multi``, 2..64 rows ``lora_down_multi`` + ``gemm_nf4_lora_multi``:
    one pass over the packed weight whatever the mix, and nothing about the selection is read on the host, so a captured step follows
    ``selection.set``.  The fused route is taken where :func:`lora_fused_ahead` takes it for the common rank; a common rank above 256,
    65+ rows, shapes the ops refuse and the other cells run the base through the parent's kernels and the adapters in torch in f32 as
    a loop over the stack with row masks, added before one cast (capturable as well, no ``rows * R * K`` temporary)."""

    def __init__(self, quant_data: QuantData, epilogue: int, adapters, selection: AdapterSelection):
        super().__init__(quant_data, epilogue)
        adapters = list(adapters)
        if not adapters:
            raise ValueError("MultiLoRANF4Linear needs at least one adapter")
        if not isinstance(selection, AdapterSelection):
            raise TypeError("selection must be an AdapterSelection")
        dev, M, K = self.qweight.device, int(quant_data.M), self.in_features
        triples = []
        for A, B, scale in adapters:
            if A.ndim != 2 or B.ndim != 2 or A.shape[1] != K or B.shape != (M, A.shape[0]):
                raise ValueError(f"adapter shapes {tuple(A.shape)} / {tuple(B.shape)} do not fit a [{M}, {K}] weight (need A [r, K] and B [M, r])")
            r = int(A.shape[0])
            if not torch.is_tensor(scale):
                scale = torch.full((r,), float(scale))
            if scale.numel() != r:
                raise ValueError(f"scale must be one factor or one per adapter row ({r}), got {scale.numel()}")
            triples.append((A.detach().to(dev), B.detach().to(dev), scale.detach().reshape(-1).to(device=dev, dtype=torch.float32)))
        self.ranks = [int(A.shape[0]) for A, _, _ in triples]
        rank = max(self.ranks) + (-max(self.ranks) % LORA_RANK_MULTIPLE)
        dtype = triples[0][0].dtype
        padded = [pad_adapter_to(A.to(dtype), B.to(dtype), s, rank) for A, B, s in triples]
        self.register_buffer("lora_A_stack", torch.stack([p[0] for p in padded]).contiguous(), persistent=True)
        self.register_buffer("lora_B_stack", torch.stack([p[1] for p in padded]).contiguous(), persistent=True)
        self.register_buffer("lora_scale_stack", torch.stack([p[2] for p in padded]).contiguous(), persistent=True)
        self.selection = selection
        self._lora_ok = rank <= LORA_MAX_RANK  # cleared as well when lora_down_multi reports a shape as not covered
        self._cast = {}  # activation dtype -> (A_stack, B_stack) in that dtype

    # -- constructors ------------------------------------------------------------------------------------------------
    @classmethod
    def from_fused(cls, layer: FusedNF4Linear, adapters, selection: AdapterSelection) -> "MultiLoRANF4Linear":
        """From a :class:`FusedNF4Linear` (shares its packed weight); every ``B`` covers the weight's own (interleaved) rows."""
        cls._check_code(layer.quant_data)
        return cls(layer.quant_data, layer.epilogue, adapters, selection)

    @classmethod
    def from_linear(cls, layer, adapters, selection: AdapterSelection) -> "MultiLoRANF4Linear":
        return cls.from_fused(FusedNF4Linear.from_linear(layer), adapters, selection)

    @classmethod
    def gate_up_from_fused(cls, layer: FusedNF4Linear, adapter_pairs, selection: AdapterSelection) -> "MultiLoRANF4Linear":
        """``adapter_pairs``: per adapter ``(gate_adapter, up_adapter)``, each ``(A, B, scaling)`` - stacked per adapter first."""
        if layer.epilogue != EPILOGUE_SILU_MUL_PAIRS:
            raise ValueError("gate_up_from_fused() needs a gate|up layer (FusedNF4Linear.gate_up)")
        return cls.from_fused(layer, [stack_gate_up_adapters(g, u) for g, u in adapter_pairs], selection)

    @classmethod
    def from_packed(cls, *args, **kwargs):
        raise TypeError("MultiLoRANF4Linear needs adapters: build a FusedNF4Linear.from_packed(...) and pass it to from_fused()")

    @classmethod
    def gate_up_from_packed(cls, *args, **kwargs):
        raise TypeError("MultiLoRANF4Linear needs adapters: build a FusedNF4Linear.gate_up_from_packed(...) and pass it to gate_up_from_fused()")

    @property
    def n_adapters(self) -> int:
        return int(self.lora_A_stack.shape[0])

    @property
    def rank(self) -> int:
        """The common (padded) rank of the stack."""
        return int(self.lora_A_stack.shape[1])

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)  # device moves only; the selection is shared and stays where it was built
        for name in ("lora_A_stack", "lora_B_stack", "lora_scale_stack"):
            self._buffers[name] = self._buffers[name].to(self.qweight.device)
        self._cast = {}
        return self

    # -- forward -----------------------------------------------------------------------------------------------------
    def _stacks(self, dtype: torch.dtype):
        if self.lora_A_stack.dtype == dtype:
            return self.lora_A_stack, self.lora_B_stack
        cast = self._cast.get(dtype)
        if cast is None or cast[0].device != self.lora_A_stack.device:
            cast = self._cast[dtype] = (self.lora_A_stack.to(dtype), self.lora_B_stack.to(dtype))
        return cast

    def _adapters_in_torch(self, x: torch.Tensor, residual: Optional[torch.Tensor], ids: torch.Tensor) -> torch.Tensor:
        A, B = self._stacks(x.dtype)
        xf = x.float().reshape(-1, x.shape[-1])
        delta = None
        for a in range(self.n_adapters):  # row masks: nothing about ids is read on the host
            mask = (ids == a).to(torch.float32).unsqueeze(1)
            d = mask * ((xf @ A[a].float().t() * self.lora_scale_stack[a]) @ B[a].float().t())
            delta = d if delta is None else delta + d
        delta = delta.reshape(*x.shape[:-1], delta.shape[-1])
        if self.epilogue == EPILOGUE_SILU_MUL_PAIRS:
            y = (self.quant_data.forward(x).float() + delta).to(x.dtype)
            y = nn.functional.silu(y[..., 0::2]) * y[..., 1::2]
        else:
            y = (FusedNF4Linear.forward(self, x).float() + delta).to(x.dtype)
        return y if residual is None else y + residual

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        qd = self.quant_data
        K = x.shape[-1]
        self._fix_compute_dtype(x)
        rows = x.numel() // K if K else 0
        ids = self.selection.ids
        if ids.numel() != rows:
            raise ValueError(f"the AdapterSelection holds {ids.numel()} ids, the batch has {rows} rows: call selection.set() with one id per row")
        if self._lora_ok and rows >= 1 and K == self.in_features and x.dtype == qd.o_type and K % qd.blocksize == 0:
            one = rows == 1 and x.ndim in (2, 3) and self._fused_ok
            many = (2 <= rows <= 64 and self._small_ok and x.dtype in (torch.float16, torch.bfloat16) and qd.blocksize == 64
                    and K % 64 == 0)
            if (one or many) and lora_fused_ahead(rows, int(qd.M), K, self.rank):
                A, B = self._stacks(x.dtype)
                x = aligned16(x)  # lora_down_multi and both adapter ops read x in 16-byte pieces
                try:
                    t = ext.lora_down_multi(x, A, self.lora_scale_stack, ids)
                except RuntimeError as exc:
                    if "not covered" not in str(exc):
                        raise
                    self._lora_ok = False
                    return self._adapters_in_torch(x, residual, ids)
                in_kernel = residual is not None and self._residual_in_kernel(rows, K)  # the parent's measured exception
                try:
                    op = ext.gemv_nf4_lora_multi if one else ext.gemm_nf4_lora_multi
                    y = op(x, qd._B_t, qd.absmax, qd.blocksize, qd._shape_list, qd.bias, residual if in_kernel else None, self.epilogue, B, ids, t)
                    return y if in_kernel or residual is None else y + residual
                except RuntimeError as exc:  # a refusal clears the flag of the op that refused, whatever its wording
                    if "not available" not in str(exc) and "not covered" not in str(exc):
                        raise
                    if one:
                        self._fused_ok = False
                    else:
                        self._small_ok = False
        return self._adapters_in_torch(x, residual, ids)

    def extra_repr(self) -> str:
        return super().extra_repr() + f", adapters={self.n_adapters}, lora_ranks={self.ranks}, common_rank={self.rank}"
