"""torch_bnb_fp4 for AMD Instinct MI355X (gfx950): FP4 Linear inference over bitsandbytes-format weights.

Same public surface as aredden/torch-bnb-fp4's ``torch_bnb_fp4`` package (reference
torch_bnb_fp4/__init__.py), backed by hand-written CDNA4 HIP kernels:

* functional ops      - :mod:`torch_bnb_fp4.functional`   (reference :87-337)
* dispatcher          - :class:`QuantData`                (reference :340-618)
* nn.Module shell     - :class:`TorchFP4Linear`           (reference :621-714)
* model surgery       - :func:`recursively_replace_with_fp4_linear` and helpers (reference :717-922)

Both bitsandbytes 4-bit codes are decoded: ``quant_type="fp4"`` (the reference's) and ``"nf4"`` (QLoRA's).
NF4 runs a fused GEMV for one token and, behind ``set_small_batch_fused(model, True, nf4=True)`` (``QuantData.small_batch_fused_nf4``,
off by default), a fused matrix-core kernel for 2..16 rows (``ext.gemm_small_nf4``; blocksize 64, in_features % 512 == 0, fp16 / bf16);
behind ``nf4_wide=True`` (``QuantData.wide_batch_fused_nf4``, off by default) a one-pass kernel for 17..64 rows, and for 2..16 rows where
in_features % 512 != 0 (``ext.gemm_wide_nf4``; blocksize 64, in_features % 64 == 0, fp16 / bf16); everything else is NF4 dequant + GEMM.
Double-quantised (nested) absmax - ``bnb_4bit_use_double_quant=True`` - loads either expanded to f32 once (the default: every kernel
above applies) or, with ``load_fp4_layers(..., nested="resident")``, stays compressed on the device in :class:`NestedNF4Linear`, whose
one-token path is a GEMV that reads the compressed statistics directly (:mod:`torch_bnb_fp4.nested`); the two NF4 switches above route
its 2..64-row calls to the same fused kernels reading the compressed statistics (``ext.gemm_nf4_nested``), and ``attach_lora`` gives
it an adapter (:class:`LoRANestedNF4Linear`).
bitsandbytes is optional: :mod:`torch_bnb_fp4.nn` provides attribute-compatible ``LinearFP4`` /
``Params4bit`` / ``QuantState`` and the quantiser runs on the GPU through this package.
"""
from ._ext import HIP_LIBRARY_PATH, ext
from .dtypes import ScalarType
from .functional import (
    dequantize_fp4,
    dequantize_fp4_codebook_invoke,
    dequantize_fp4_codebook_invoke_qtype,
    dequantize_fp4_qtype,
    gemm_4bit_inference,
    gemm_4bit_inference_qtype,
    quantize_fp4,
    dequantize_nf4,
    gemv_nf4,
    quantize_nf4,
)
from .comm import OneShotAllReduce
from .fused import AdapterSelection, FusedFP4Linear, FusedNF4Linear, LoRANF4Linear, MultiLoRANF4Linear
from .graphs import GraphedStep
from .linear import TorchFP4Linear
from .nested import LoRANestedNF4Linear, NestedNF4Linear, expand_nested
from .nn import Linear4bit, LinearFP4, LinearNF4, Params4bit, QuantState, nf4_code
from .quant_data import QuantData
from .serialization import fp4_linear_from_bnb_state, fp4_linear_to_bnb_state, load_fp4_layers, save_fp4_model
from .surgery import (
    FusedGatedMLP,
    attach_lora,
    attach_lora_adapters,
    check_if_name_contained_in_list,
    fuse_gated_mlps,
    load_lora_adapter,
    load_lora_adapters,
    recursively_replace_with_fp4_linear,
    set_small_batch_fused,
    swap_linear_with_bnb_linear,
    todevice_if_necessary,
)

__all__ = [
    "ScalarType",
    "dequantize_fp4",
    "dequantize_fp4_codebook_invoke_qtype",
    "dequantize_fp4_codebook_invoke",
    "gemm_4bit_inference",
    "gemm_4bit_inference_qtype",
    "dequantize_fp4_qtype",
    "quantize_fp4",
    "QuantData",
    "TorchFP4Linear",
    "swap_linear_with_bnb_linear",
    "check_if_name_contained_in_list",
    "todevice_if_necessary",
    "recursively_replace_with_fp4_linear",
    "LinearFP4",
    "Linear4bit",
    "Params4bit",
    "QuantState",
    "fp4_linear_to_bnb_state",
    "fp4_linear_from_bnb_state",
    "save_fp4_model",
    "load_fp4_layers",
    "set_small_batch_fused",
    "fuse_gated_mlps",
    "FusedGatedMLP",
    "FusedFP4Linear",
    "FusedNF4Linear",
    "OneShotAllReduce",
    "GraphedStep",
    "dequantize_nf4",
    "gemv_nf4",
    "quantize_nf4",
    "LinearNF4",
    "nf4_code",
    "LoRANF4Linear",
    "attach_lora",
    "load_lora_adapter",
    "AdapterSelection",
    "MultiLoRANF4Linear",
    "attach_lora_adapters",
    "load_lora_adapters",
    "NestedNF4Linear",
    "LoRANestedNF4Linear",
    "expand_nested",
]
__version__ = "0.1.0"
