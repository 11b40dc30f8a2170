"""Nested (double-quantised) absmax: bitsandbytes' ``compress_statistics`` / ``bnb_4bit_use_double_quant=True`` (the QLoRA recipe).

The per-block absmax of a 4-bit weight is stored as uint8 codes into a 256-entry f32 table, with one f32 scale per 256 blocks and
one offset per weight::

    absmax[i] = fl32(fl32(nested_code[absmax_u8[i]] * nested_absmax[i // 256]) + offset)         (two roundings, never an FMA)

0.127 instead of 0.5 bit per weight at blocksize 64.  Two ways to run such a weight:

* expanded - ``ext.absmax_unnest`` once at load, then an ordinary :class:`TorchFP4Linear` (every kernel, switch and surgery applies);
* resident - :class:`NestedNF4Linear` keeps the statistics compressed on the device: one token goes to ``ext.gemv_nf4_nested``, whose
  result equals ``gemv_nf4_fused`` on the expanded absmax bit for bit; more rows expand into a temporary (``ext.qlinear_nf4_nested``)
  unless ``set_small_batch_fused(model, True, nf4=True, nf4_wide=True)`` has routed 2..64 rows to ``ext.gemm_nf4_nested``, the fused
  matrix-core kernels reading the compressed statistics (the bits of ``gemm_nf4_fused`` on the expanded absmax).
  :class:`LoRANestedNF4Linear` is such a layer with one LoRA adapter (``attach_lora`` / ``load_lora_adapter`` build it).

:class:`NestedNF4Linear` is deliberately not a :class:`TorchFP4Linear`: ``fuse_gated_mlps``, ``attach_lora_adapters``
(:class:`~torch_bnb_fp4.fused.MultiLoRANF4Linear`) and the tensor-parallel wrappers permute, concatenate or re-route rows, and a
compressed group spans rows.  They stay expand-first: call :func:`expand_nested` before them; ``fuse_gated_mlps`` and the
tensor-parallel wrappers ignore a module they do not recognise.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import nn

from ._ext import ext
from .dtypes import ScalarType
from .fused import LoRAAdapterMixin
from .quant_data import aligned16

NESTED_BLOCKSIZE = 256  # what every bitsandbytes file holds, and what the resident GEMV reads


def dynamic_map() -> torch.Tensor:
    """bitsandbytes' ``create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8)``, the table its double quantisation
    writes as ``nested_quant_map``: 256 strictly increasing f32 values in [-0.993, 1.0] with 0.0 at index 127.  Needed for the
    writing side only - a loaded file's table is used as it is."""
    data = []
    for i in range(7):
        boundaries = torch.linspace(0.1, 1, 2**i + 1)
        means = (boundaries[:-1] + boundaries[1:]) / 2.0
        data += ((10 ** (i - 6)) * means).tolist()
        data += (-(10 ** (i - 6)) * means).tolist()
    data += [0.0, 1.0]
    data.sort()
    return torch.tensor(data, dtype=torch.float32)


def nest_absmax(absmax: torch.Tensor, offset: Optional[float] = None, code: Optional[torch.Tensor] = None,
                nested_blocksize: int = NESTED_BLOCKSIZE) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, float]:
    """Double-quantise f32 ``absmax`` on its (GPU) device: ``(absmax_u8, nested_absmax, nested_code, offset)``.  The offset defaults
    to ``absmax.mean()`` and the table to :func:`dynamic_map`, as in bitsandbytes.  Lossy: :func:`unnest_absmax` returns each scale
    to within half the table's largest gap times its group's scale."""
    absmax = absmax.detach().float().reshape(-1).contiguous()
    if offset is None:
        offset = float(absmax.mean().item()) if absmax.numel() else 0.0
    code = (dynamic_map() if code is None else code).to(device=absmax.device, dtype=torch.float32).contiguous()
    q, nested = ext.absmax_nest(absmax, float(offset), code, int(nested_blocksize))
    return q, nested, code, float(offset)


def unnest_absmax(absmax_u8: torch.Tensor, nested_absmax: torch.Tensor, nested_code: torch.Tensor, offset: float,
                  nested_blocksize: int = NESTED_BLOCKSIZE) -> torch.Tensor:
    """The f32 absmax a nested state decodes to (``ext.absmax_unnest``; bit-exact to bitsandbytes' two-step decode)."""
    return ext.absmax_unnest(absmax_u8.reshape(-1).contiguous(), nested_absmax.float().contiguous(), nested_code.float().contiguous(),
                             float(offset), int(nested_blocksize))


def resident_covers(quant_type: str, M: int, K: int, blocksize: int, nested_blocksize: int) -> bool:
    """Whether ``ext.gemv_nf4_nested`` takes this weight: NF4, groups of 256, in_features % 32 == 0 and a power-of-two blocksize
    >= 32 that divides in_features (the fast path of the NF4 GEMV)."""
    return (quant_type == "nf4" and nested_blocksize == NESTED_BLOCKSIZE and M > 0 and K > 0 and K % 32 == 0 and blocksize >= 32
            and blocksize & (blocksize - 1) == 0 and K % blocksize == 0)


class NestedNF4Linear(nn.Module):
    """An NF4 Linear whose absmax stays double-quantised on the device.

    Buffers: ``qweight`` (packed, uint8 [M*K/2, 1]), ``absmax_u8`` (uint8 [nb]), ``nested_absmax`` (f32 [ceil(nb/256)]),
    ``nested_code`` (f32 [256]), ``code`` (the NF4 table) and ``bias``; ``offset`` is a Python float (it travels in the state dict as
    extra state).  ``forward(x, residual=None)``: one row of 2-D or 3-D input runs the nested GEMV with the bias and the residual
    in its epilogue (``T(T(T(sum) + bias) + residual)``); everything else expands the statistics into a temporary, runs NF4
    dequant + GEMM, and torch adds the residual.  With ``small_batch_fused_nf4`` / ``wide_batch_fused_nf4`` set
    (``set_small_batch_fused``; both OFF by default) 2..64 rows of fp16 / bf16 against a blocksize-64 weight with ``K % 64 == 0`` run
    ``ext.gemm_nf4_nested`` instead, in the cells the same switches open on an expanded layer and with the residual in the kernel
    except in the one cell :class:`~torch_bnb_fp4.fused.FusedNF4Linear` excludes; an op that answers "not covered" is not tried again."""

    def __init__(self, packed: torch.Tensor, absmax_u8: torch.Tensor, nested_absmax: torch.Tensor, nested_code: torch.Tensor,
                 offset: float, shape, blocksize: int = 64, bias: Optional[torch.Tensor] = None,
                 dtype: torch.dtype = torch.float16, code: Optional[torch.Tensor] = None, name: str = ""):
        super().__init__()
        M, K = int(shape[0]), int(shape[1])
        nb = -(-M * K // int(blocksize))
        if not resident_covers("nf4", M, K, int(blocksize), NESTED_BLOCKSIZE):
            raise ValueError(f"NestedNF4Linear: a {M}x{K} weight with blocksize {blocksize} is not covered by the nested GEMV (needs "
                             "in_features % 32 == 0 and a power-of-two blocksize >= 32 dividing in_features); expand it instead")
        if packed.dtype != torch.uint8 or packed.numel() != (M * K + 1) // 2:
            raise ValueError(f"NestedNF4Linear: packed must hold {(M * K + 1) // 2} uint8 bytes")
        if absmax_u8.dtype != torch.uint8 or absmax_u8.numel() != nb:
            raise ValueError(f"NestedNF4Linear: nested absmax must be {nb} uint8 codes, got {absmax_u8.numel()} of {absmax_u8.dtype}")
        if nested_absmax.numel() != -(-nb // NESTED_BLOCKSIZE) or nested_code.numel() != 256:
            raise ValueError(f"NestedNF4Linear: nested_absmax must hold {-(-nb // NESTED_BLOCKSIZE)} scales and nested_code 256 entries")
        self.in_features, self.out_features = K, M
        self.blocksize = int(blocksize)
        self.nested_blocksize = NESTED_BLOCKSIZE
        self.offset = float(offset)
        self.quant_dtype = dtype
        self.name = name
        dev = packed.device
        self.register_buffer("qweight", packed.reshape(-1, 1).contiguous(), persistent=True)
        self.register_buffer("absmax_u8", absmax_u8.reshape(-1).contiguous().to(dev), persistent=True)
        self.register_buffer("nested_absmax", nested_absmax.reshape(-1).float().contiguous().to(dev), persistent=True)
        self.register_buffer("nested_code", nested_code.reshape(-1).float().contiguous().to(dev), persistent=True)
        self.register_buffer("code", (ext.code_table("nf4") if code is None else code.float()).to(dev), persistent=True)
        self.register_buffer("bias", None if bias is None else bias.detach().to(dev), persistent=True)
        self._shape_list = [M, K]
        # opt-in (set_small_batch_fused(model, True, nf4=True, nf4_wide=True)), OFF by default as on a TorchFP4Linear: 2..16 rows with
        # K % 512 == 0, respectively 17..64 rows and 2..16 rows with K % 512 != 0, run ext.gemm_nf4_nested instead of the expand path
        self.small_batch_fused_nf4 = False
        self.wide_batch_fused_nf4 = False
        self._batched_ok = True  # cleared the first time the batched op reports the shape as not covered

    # -- state -----------------------------------------------------------------------------------------------------------------
    def get_extra_state(self):
        return {"offset": self.offset, "blocksize": self.blocksize, "shape": [self.out_features, self.in_features]}

    def set_extra_state(self, state):
        if [int(v) for v in state["shape"]] != [self.out_features, self.in_features] or int(state["blocksize"]) != self.blocksize:
            raise ValueError(f"NestedNF4Linear: the state is of a {state['shape']} weight with blocksize {state['blocksize']}, this "
                             f"layer holds {[self.out_features, self.in_features]} with blocksize {self.blocksize}")
        self.offset = float(state["offset"])

    def _apply(self, fn, recurse=True):
        # only device moves are honoured: bytes, codes and f32 scales never change dtype
        probe = fn(torch.empty(0, dtype=torch.float16, device=self.qweight.device))
        if probe.device != self.qweight.device:
            for name, buf in list(self._buffers.items()):
                self._buffers[name] = None if buf is None else buf.to(probe.device)
        return self

    # -- compute ---------------------------------------------------------------------------------------------------------------
    def expanded_absmax(self) -> torch.Tensor:
        return unnest_absmax(self.absmax_u8, self.nested_absmax, self.nested_code, self.offset, self.nested_blocksize)

    def dequantize(self, dtype: torch.dtype = torch.float16) -> torch.Tensor:
        """The [out_features, in_features] weight in ``dtype``: ``RN(nf4[nibble] * absmax)`` with the expanded absmax."""
        return ext.dequantize_nf4(self.qweight, self.expanded_absmax(), self.blocksize, self.out_features, self.in_features,
                                  ScalarType.from_torch_dtype(dtype).value)

    def _bias_for(self, x: torch.Tensor) -> Optional[torch.Tensor]:
        b = self.bias
        if b is not None and b.dtype != x.dtype:  # cast once to the activation dtype, as TorchFP4Linear does on its first call
            b = self._buffers["bias"] = b.to(x.dtype)
        return b

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        K, M = self.in_features, self.out_features
        if x.shape[-1] != K:
            raise ValueError(f"NestedNF4Linear: the activation's last dim is {x.shape[-1]}, in_features is {K}")
        if x.numel() == 0:
            return torch.empty(x.shape[:-1] + (M,), dtype=x.dtype, device=x.device)
        bias = self._bias_for(x)
        if x.numel() == K and x.dim() in (2, 3) and x.dtype in (torch.float16, torch.bfloat16, torch.float32):
            # the GEMV reads x in 16-byte pieces: an activation off that boundary is copied once (an address belongs to the call)
            return ext.gemv_nf4_nested(aligned16(x), self.qweight.t(), self.absmax_u8, self.nested_absmax, self.nested_code, self.offset,
                                       self.nested_blocksize, self.blocksize, self._shape_list, bias,
                                       None if residual is None else residual.contiguous(), 0)
        rows = x.numel() // K
        if self._batched_ok and self._batched_routed(rows, K, x.dtype):
            in_kernel = residual is not None and self._residual_in_kernel(rows, K)
            try:
                # the call is made coverable, so that a refusal caught below is about the shape, which belongs to the layer
                y = ext.gemm_nf4_nested(aligned16(x), self.qweight.t(), self.absmax_u8, self.nested_absmax, self.nested_code, self.offset,
                                        self.nested_blocksize, self.blocksize, self._shape_list, bias,
                                        residual.contiguous() if in_kernel else None, 0)
                return y if in_kernel or residual is None else y + residual
            except RuntimeError as exc:
                if "not covered" not in str(exc):
                    raise
                self._batched_ok = False  # not tried again: the expand path from now on
        return self._expand_path(x, bias, residual)

    def _expand_path(self, x: torch.Tensor, bias: Optional[torch.Tensor], residual: Optional[torch.Tensor]) -> torch.Tensor:
        y = ext.qlinear_nf4_nested(x, self.qweight, self.absmax_u8, self.nested_absmax, self.nested_code, self.offset,
                                   self.nested_blocksize, self.out_features, self.in_features, self.blocksize, bias)
        return y if residual is None else y + residual

    def _batched_covers(self, rows: int, K: int, dtype: torch.dtype) -> bool:
        """FusedNF4Linear._batched_covers: what ``ext.gemm_nf4_nested`` is routed for."""
        return 2 <= rows <= 64 and dtype in (torch.float16, torch.bfloat16) and self.blocksize == 64 and K % 64 == 0

    def _batched_routed(self, rows: int, K: int, dtype: torch.dtype) -> bool:
        """The cells the two switches open, the same ones as on an expanded :class:`TorchFP4Linear` (quant_data.py)."""
        if not self._batched_covers(rows, K, dtype):
            return False
        small = rows <= 16 and K % 512 == 0
        return self.small_batch_fused_nf4 if small else self.wide_batch_fused_nf4

    def _residual_in_kernel(self, rows: int, K: int) -> bool:
        # FusedNF4Linear._residual_in_kernel for the plain epilogue: the one cell in which the fused add measured no gain
        return not (rows > 32 and K >= 8192)

    def expand(self, use_codebook_dequant: bool = True):
        """The ordinary :class:`TorchFP4Linear` this layer decodes to (f32 absmax; same outputs, 4x the statistics)."""
        from .serialization import plain_linear

        return plain_linear(self.qweight, self.expanded_absmax(), self.code, (self.out_features, self.in_features), self.blocksize,
                            self.quant_dtype, "nf4", self.bias, use_codebook_dequant, self.name)

    def __repr__(self) -> str:
        return (f"NestedNF4Linear(in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"blocksize={self.blocksize}, nested_blocksize={self.nested_blocksize})")


class LoRANestedNF4Linear(LoRAAdapterMixin, NestedNF4Linear):
    """A :class:`NestedNF4Linear` with one LoRA adapter beside the resident weight: ``forward(x, residual=None)`` =
    ``W x + B (s * A x) (+ residual)``, the statistics still compressed on the device.

    ``lora_A`` is ``[r, K]``, ``lora_B`` ``[M, r]``, ``scale`` a float or a float32 ``[r]`` tensor; any rank works (zero-padded to a
    multiple of 8 by :func:`~torch_bnb_fp4.fused.pad_adapter`, which is exact) and the adapter follows the activation dtype, as in
    :class:`~torch_bnb_fp4.fused.LoRANF4Linear`, whose rank limits hold here.  One row runs ``lora_down`` + ``gemv_nf4_lora_nested``,
    2..64 rows ``lora_down`` + ``gemm_nf4_lora_nested`` where :func:`~torch_bnb_fp4.fused.lora_fused_ahead` allows it: the bits of
    ``gemv_nf4_lora`` / ``gemm_nf4_lora`` on the expanded absmax.  Everything else runs the base through :class:`NestedNF4Linear`'s
    own path and the adapter in torch in f32, ``(x.float() @ A.float().T * scale) @ B.float().T``, added before one cast."""

    def __init__(self, layer: NestedNF4Linear, lora_A: torch.Tensor, lora_B: torch.Tensor, scale):
        super().__init__(layer.qweight, layer.absmax_u8, layer.nested_absmax, layer.nested_code, layer.offset,
                         (layer.out_features, layer.in_features), layer.blocksize, layer.bias, layer.quant_dtype, layer.code, layer.name)
        self.small_batch_fused_nf4, self.wide_batch_fused_nf4 = layer.small_batch_fused_nf4, layer.wide_batch_fused_nf4
        self._init_adapter(lora_A, lora_B, scale, self.out_features, self.in_features, self.qweight.device)
        self._gemv_lora_ok = True
        self._gemm_lora_ok = True

    @classmethod
    def from_nested(cls, layer: NestedNF4Linear, lora_A, lora_B, scaling) -> "LoRANestedNF4Linear":
        """From a :class:`NestedNF4Linear` (shares its packed weight and statistics) and one adapter."""
        return cls(layer, lora_A, lora_B, scaling)

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)  # device moves only
        self._cast = {}
        return self

    def _adapter_in_torch(self, x: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
        y = (NestedNF4Linear.forward(self, x).float() + self._adapter_delta(x)).to(x.dtype)
        return y if residual is None else y + residual

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        from .fused import lora_fused_ahead

        K, M = self.in_features, self.out_features
        if x.shape[-1] != K:
            raise ValueError(f"LoRANestedNF4Linear: the activation's last dim is {x.shape[-1]}, in_features is {K}")
        if x.numel() == 0:
            return torch.empty(x.shape[:-1] + (M,), dtype=x.dtype, device=x.device)
        rows = x.numel() // K
        if self._lora_ok:
            one = (rows == 1 and x.dim() in (2, 3) and self._gemv_lora_ok
                   and x.dtype in (torch.float16, torch.bfloat16, torch.float32))
            many = self._gemm_lora_ok and self._batched_covers(rows, K, x.dtype)
            if (one or many) and lora_fused_ahead(rows, M, K, int(self.lora_A.shape[0])):
                A, B = self._adapter(x.dtype)
                xc = aligned16(x)  # lora_down and both adapter ops read x in 16-byte pieces
                try:
                    t = ext.lora_down(xc, A, self.lora_scale)
                except RuntimeError as exc:
                    if "not covered" not in str(exc):
                        raise
                    self._lora_ok = False
                    return self._adapter_in_torch(x, residual)
                in_kernel = residual is not None and (one or self._residual_in_kernel(rows, K))
                try:
                    op = ext.gemv_nf4_lora_nested if one else ext.gemm_nf4_lora_nested
                    y = op(xc, self.qweight.t(), self.absmax_u8, self.nested_absmax, self.nested_code, self.offset, self.nested_blocksize,
                           self.blocksize, self._shape_list, self._bias_for(x), residual.contiguous() if in_kernel else None, 0, B, t)
                    return y if in_kernel or residual is None else y + residual
                except RuntimeError as exc:  # a refusal clears the flag of the op that refused, whatever its wording
                    if "not available" not in str(exc) and "not covered" not in str(exc):
                        raise
                    if one:
                        self._gemv_lora_ok = False
                    else:
                        self._gemm_lora_ok = False
        return self._adapter_in_torch(x, residual)

    def expand(self, use_codebook_dequant: bool = True):
        """The :class:`~torch_bnb_fp4.fused.LoRANF4Linear` over the expanded weight, with this layer's adapter."""
        from .fused import LoRANF4Linear

        return LoRANF4Linear.from_linear(super().expand(use_codebook_dequant), self.lora_A, self.lora_B, self.lora_scale)

    def __repr__(self) -> str:
        return "LoRA" + super().__repr__()[:-1] + f", lora_rank={self.rank})"


def expand_nested(model: nn.Module, use_codebook_dequant: bool = True) -> nn.Module:
    """Replace every :class:`NestedNF4Linear` in ``model`` by its expanded :class:`TorchFP4Linear`, a
    :class:`LoRANestedNF4Linear` by a :class:`~torch_bnb_fp4.fused.LoRANF4Linear` with the same adapter (do this before
    ``fuse_gated_mlps``, ``attach_lora_adapters`` or tensor-parallel sharding; ``attach_lora`` and ``set_small_batch_fused`` take
    resident layers as they are).  The two NF4 switches are not carried over: call ``set_small_batch_fused`` again afterwards.
    Returns the model (a bare NestedNF4Linear returns its replacement)."""
    if isinstance(model, NestedNF4Linear):
        return model.expand(use_codebook_dequant)
    for parent in list(model.modules()):
        for child_name, child in list(parent._modules.items()):
            if isinstance(child, NestedNF4Linear):
                parent._modules[child_name] = child.expand(use_codebook_dequant)
    return model
