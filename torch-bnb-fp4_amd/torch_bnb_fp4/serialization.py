"""bitsandbytes-format (de)serialisation of FP4 Linear layers.

A pre-quantised bitsandbytes checkpoint stores, per ``Linear4bit`` weight (key names as consumed by
``transformers/quantizers/quantizer_bnb_4bit.py:172-184``):

    <prefix>weight                                   uint8  [numel/2, 1]   packed nibbles
    <prefix>weight.absmax                            float32 [numel/blocksize]
    <prefix>weight.quant_map                         float32 [16]           the code (k/12)
    <prefix>weight.quant_state.bitsandbytes__fp4     uint8  [len]          utf-8 JSON: quant_type, blocksize, dtype, shape
    <prefix>bias                                     (optional)

An NF4 weight has the same entries with ``weight.quant_state.bitsandbytes__nf4``, ``"quant_type": "nf4"`` and the NF4 code as
``quant_map``; on load the map must equal this package's NF4 table bit for bit (custom maps are refused, not decoded).

A double-quantised weight (``bnb_4bit_use_double_quant=True``, the QLoRA recipe) stores its absmax nested - FP4 or NF4 alike:

    <prefix>weight.absmax                            uint8   [nb]                 codes into nested_quant_map
    <prefix>weight.nested_absmax                     float32 [ceil(nb/256)]       one scale per nested_blocksize blocks
    <prefix>weight.nested_quant_map                  float32 [256]                taken from the file as it is, never compared
    ... and the JSON gains nested_blocksize, nested_dtype ("float32") and nested_offset

    absmax[i] = fl32(fl32(nested_quant_map[absmax_u8[i]] * nested_absmax[i // nested_blocksize]) + nested_offset)

On load, ``nested="expand"`` (the default) decodes the statistics once (``ext.absmax_unnest``) into an ordinary
:class:`TorchFP4Linear`; ``nested="resident"`` keeps them compressed on the device in a :class:`~torch_bnb_fp4.nested.NestedNF4Linear`
for the NF4 weights the nested GEMV covers and expands the others.  An ill-formed nested state (a nested key beside an f32 absmax, a
missing map, wrong sizes, a missing JSON field, a nested_dtype other than float32) is refused with a ``ValueError`` that says what
is wrong.  Saving nested is opt-in (``save_fp4_model(..., nested=True)``); the default writes f32 absmax.

The reference cannot load or save its layers at all (its wrapped module is hidden in a python list,
torch_bnb_fp4/__init__.py:644); this module round-trips :class:`TorchFP4Linear` through exactly that format, so
FP4 safetensors written by bitsandbytes/transformers load straight into the MI355X path without re-quantising.
"""
from __future__ import annotations

import json
from typing import Dict, Mapping

import torch

from .linear import TorchFP4Linear
from .nested import NESTED_BLOCKSIZE, NestedNF4Linear, nest_absmax, resident_covers, unnest_absmax
from .nn import LinearFP4, Params4bit, QuantState, nf4_code

_STATE_KEY = "weight.quant_state.bitsandbytes__fp4"
_STATE_KEYS = {"fp4": _STATE_KEY, "nf4": "weight.quant_state.bitsandbytes__nf4"}


def _pack_json(d: dict) -> torch.Tensor:
    return torch.tensor(list(json.dumps(d).encode("utf-8")), dtype=torch.uint8)


def _unpack_json(t: torch.Tensor) -> dict:
    return json.loads(bytes(t.detach().cpu().to(torch.uint8).tolist()).decode("utf-8"))


def _bnb_entries(prefix: str, packed, absmax, code, blocksize: int, shape, dtype, bias, quant_type: str = "fp4",
                 nested=None) -> Dict[str, torch.Tensor]:
    """``nested`` = None (f32 ``absmax``), True (f32 ``absmax`` is double-quantised here: offset = its mean, the dynamic map, groups of
    256) or a ready ``(absmax_u8, nested_absmax, nested_code, offset)`` written as it is."""
    meta = {"quant_type": quant_type, "blocksize": int(blocksize), "dtype": str(dtype).replace("torch.", ""), "shape": [int(shape[0]), int(shape[1])]}
    extra = {}
    if nested is None:
        absmax = absmax.detach().float().cpu()
    else:
        q, nested_absmax, nested_code, offset = nest_absmax(absmax) if nested is True else nested
        absmax = q.detach().cpu().reshape(-1)
        extra = {prefix + "weight.nested_absmax": nested_absmax.detach().float().cpu().reshape(-1).clone(),
                 prefix + "weight.nested_quant_map": nested_code.detach().float().cpu().reshape(-1).clone()}
        meta.update({"nested_blocksize": NESTED_BLOCKSIZE, "nested_dtype": "float32", "nested_offset": float(offset)})
    out = {
        prefix + "weight": packed.detach().cpu().reshape(-1, 1),
        prefix + "weight.absmax": absmax,
        prefix + "weight.quant_map": code.detach().float().cpu().clone(),  # a gate|up pair shares one code tensor: one copy per entry
        prefix + _STATE_KEYS[quant_type]: _pack_json(meta),
        **extra,
    }
    if bias is not None:
        out[prefix + "bias"] = bias.detach().cpu()
    return out


def fp4_linear_to_bnb_state(layer: TorchFP4Linear, prefix: str = "", nested: bool = False) -> Dict[str, torch.Tensor]:
    """State-dict entries of one layer in bitsandbytes' 4-bit layout (tensors moved to the CPU).  ``nested=True`` double-quantises the
    absmax on the way out (lossy in the scales; needs the layer on a GPU)."""
    qd = layer.quant_data
    return _bnb_entries(prefix, qd.A, qd.absmax, qd.code, qd.blocksize, (qd.M, qd.N), qd.quant_state.dtype, layer.bias,
                        qd.quant_type, True if nested else None)


def nested_linear_to_bnb_state(layer: NestedNF4Linear, prefix: str = "", nested: bool = True) -> Dict[str, torch.Tensor]:
    """A :class:`NestedNF4Linear` in bitsandbytes' layout: ``nested=True`` writes its compressed statistics verbatim (it loads back
    bit for bit), ``nested=False`` the f32 absmax they decode to."""
    shape = (layer.out_features, layer.in_features)
    if nested:
        return _bnb_entries(prefix, layer.qweight, None, layer.code, layer.blocksize, shape, layer.quant_dtype, layer.bias, "nf4",
                            (layer.absmax_u8, layer.nested_absmax, layer.nested_code, layer.offset))
    return _bnb_entries(prefix, layer.qweight, layer.expanded_absmax(), layer.code, layer.blocksize, shape, layer.quant_dtype, layer.bias, "nf4")


def fused_linear_to_bnb_state(layer, prefix: str = "", pair_prefixes=None, dtype=None, nested: bool = False) -> Dict[str, torch.Tensor]:
    """A :class:`~torch_bnb_fp4.fused.FusedFP4Linear` (or its NF4 subclass, written under the ``__nf4`` key) in bitsandbytes' layout.  A plain one (residual epilogue) is one entry under
    ``prefix``; a gate|up one is DE-INTERLEAVED into the two projections it was built from and written under ``pair_prefixes``
    (the rows are a load-time permutation of the bnb bytes, not a new format) - without names for the pair it cannot be saved."""
    from .fused import EPILOGUE_SILU_MUL_PAIRS, deinterleave_rows

    qd = layer.quant_data
    if dtype is None:  # the dtype the weight was quantised from, as its quant_state recorded it
        dtype = getattr(qd.quant_state, "dtype", torch.float16)
    nest = True if nested else None
    if layer.epilogue != EPILOGUE_SILU_MUL_PAIRS:
        return _bnb_entries(prefix, qd.A, qd.absmax, qd.code, qd.blocksize, (qd.M, qd.N), dtype, layer.bias, qd.quant_type, nest)
    if not pair_prefixes:
        raise ValueError(f"{prefix or 'layer'}: a gate|up FusedFP4Linear can only be saved as its two projections; it is not inside a "
                         "FusedGatedMLP that remembers their names - save the unfused model (before fuse_gated_mlps) instead")
    (pg, ag), (pu, au), shape = deinterleave_rows(qd.A, qd.absmax, (qd.M, qd.N), qd.blocksize)
    bias = layer.bias
    bg = None if bias is None else bias.reshape(-1, 2)[:, 0].contiguous()
    bu = None if bias is None else bias.reshape(-1, 2)[:, 1].contiguous()
    out = _bnb_entries(pair_prefixes[0], pg, ag, qd.code, qd.blocksize, shape, dtype, bg, qd.quant_type, nest)
    out.update(_bnb_entries(pair_prefixes[1], pu, au, qd.code, qd.blocksize, shape, dtype, bu, qd.quant_type, nest))
    return out


def plain_linear(packed, absmax, code, shape, blocksize: int, dtype, quant_type: str, bias, use_codebook_dequant: bool = True,
                 name: str = "") -> TorchFP4Linear:
    """A :class:`TorchFP4Linear` over already-quantised tensors on their device (f32 absmax)."""
    M, K = int(shape[0]), int(shape[1])
    shell = LinearFP4(K, M, bias=bias is not None, device="meta")
    qs = QuantState(absmax, (M, K), code, blocksize, dtype, quant_type)
    shell._parameters["weight"] = Params4bit(packed, False, qs, blocksize, quant_type)
    if bias is not None:
        shell._parameters["bias"] = torch.nn.Parameter(bias, requires_grad=False)
    return TorchFP4Linear(shell, use_codebook_dequant=use_codebook_dequant, name=name)


_NESTED_KEYS = ("weight.nested_absmax", "weight.nested_quant_map")
_NESTED_FIELDS = ("nested_blocksize", "nested_dtype", "nested_offset")
NESTED_MODES = ("expand", "resident")


def _nested_parts(state, prefix: str, meta: dict, nb: int, dev):
    """None for a plain state; else ``(absmax_u8, nested_absmax, nested_code, offset, nested_blocksize)`` on ``dev`` of a WELL-FORMED
    nested state.  Anything in between - some of the nested entries without the others - raises."""
    where = prefix + "weight"
    keys = [k for k in _NESTED_KEYS if prefix + k in state]
    fields = [f for f in _NESTED_FIELDS if f in meta]
    absmax = state[prefix + "weight.absmax"]
    if not keys and not fields and absmax.dtype != torch.uint8:
        return None
    bad = lambda what: ValueError(f"{where}: ill-formed nested (double-quantised) absmax: {what}")
    if absmax.dtype != torch.uint8:
        raise bad(f"{', '.join(keys + fields)} present, but weight.absmax is {absmax.dtype} where nested statistics are uint8 codes")
    for k in _NESTED_KEYS:
        if prefix + k not in state:
            raise bad(f"weight.absmax is uint8 but {k} is missing")
    for f in _NESTED_FIELDS:
        if f not in meta:
            raise bad(f"the quant_state JSON has no {f}")
    if meta["nested_dtype"] != "float32":
        raise bad(f"nested_dtype is {meta['nested_dtype']!r}, only 'float32' is decoded")
    g = meta["nested_blocksize"]
    if not isinstance(g, int) or g < 64 or g > 4096 or g & (g - 1):
        raise bad(f"nested_blocksize is {g!r} (need a power of two in 64..4096)")
    try:
        offset = float(meta["nested_offset"])
    except (TypeError, ValueError):
        raise bad(f"nested_offset is {meta['nested_offset']!r}, not a number") from None
    nested_absmax, nested_code = state[prefix + _NESTED_KEYS[0]], state[prefix + _NESTED_KEYS[1]]
    if nested_absmax.dtype != torch.float32 or nested_code.dtype != torch.float32:
        raise bad(f"nested_absmax / nested_quant_map are {nested_absmax.dtype} / {nested_code.dtype}, float32 expected")
    if absmax.numel() != nb:
        raise bad(f"weight.absmax holds {absmax.numel()} codes, the recorded shape and blocksize need {nb}")
    if nested_absmax.numel() != -(-nb // g):
        raise bad(f"nested_absmax holds {nested_absmax.numel()} scales, {nb} blocks in groups of {g} need {-(-nb // g)}")
    if nested_code.numel() != 256:
        raise bad(f"nested_quant_map holds {nested_code.numel()} entries, 256 expected")
    return (absmax.to(dev).reshape(-1).contiguous(), nested_absmax.to(dev).reshape(-1).contiguous(),
            nested_code.to(dev).reshape(-1).contiguous(), offset, g)


def fp4_linear_from_bnb_state(state: Mapping[str, torch.Tensor], prefix: str = "", device="cuda",
                              use_codebook_dequant: bool = True, name: str = "", nested: str = "expand"):
    """Build a :class:`TorchFP4Linear` from bitsandbytes-format entries (no re-quantisation); FP4 or NF4.  A double-quantised
    weight is expanded (``nested="expand"``) or, with ``nested="resident"`` and an NF4 weight the nested GEMV covers, returned as a
    :class:`~torch_bnb_fp4.nested.NestedNF4Linear`; resident weights outside that coverage are expanded too (the returned type tells)."""
    if nested not in NESTED_MODES:
        raise ValueError(f"nested must be one of {NESTED_MODES}, got {nested!r}")
    found = [qt for qt, key in _STATE_KEYS.items() if prefix + key in state]
    if len(found) != 1:
        raise KeyError(f"{prefix + _STATE_KEY} (or its __nf4 twin) not found exactly once: not a bitsandbytes 4-bit weight")
    quant_type = found[0]
    meta = _unpack_json(state[prefix + _STATE_KEYS[quant_type]])
    if meta.get("quant_type") != quant_type:
        raise ValueError(f"quant_type {meta.get('quant_type')!r} does not match the entry's key ({quant_type})")
    M, K = (int(v) for v in meta["shape"])
    bs = int(meta["blocksize"])
    dev = torch.device(device)
    packed = state[prefix + "weight"].to(dev).reshape(-1, 1).contiguous()
    code = state[prefix + "weight.quant_map"].to(dev).float().contiguous()
    parts = _nested_parts(state, prefix, meta, -(-M * K // bs), dev)
    if parts is not None and nested == "resident" and resident_covers(quant_type, M, K, bs, parts[4]):
        if packed.dtype != torch.uint8 or packed.numel() != (M * K + 1) // 2 or code.numel() != 16:
            raise ValueError("inconsistent FP4 state: packed/absmax/quant_map sizes do not match the recorded shape")
        if not torch.equal(code.cpu().view(torch.int32), nf4_code().view(torch.int32)):
            raise ValueError(f"{prefix}weight.quant_map is not bitsandbytes' NF4 code: custom quant maps are not supported")
        bias = state.get(prefix + "bias")
        return NestedNF4Linear(packed, parts[0], parts[1], parts[2], parts[3], (M, K), bs, None if bias is None else bias.to(dev),
                               getattr(torch, meta.get("dtype", "float16")), code, name)
    if parts is not None:
        absmax = unnest_absmax(parts[0], parts[1], parts[2], parts[3], parts[4])
    else:
        absmax = state[prefix + "weight.absmax"].to(dev).float().contiguous()
    if packed.dtype != torch.uint8 or packed.numel() != (M * K + 1) // 2 or absmax.numel() != -(-M * K // bs) or code.numel() != 16:
        raise ValueError("inconsistent FP4 state: packed/absmax/quant_map sizes do not match the recorded shape")
    if quant_type == "nf4" and not torch.equal(code.cpu().view(torch.int32), nf4_code().view(torch.int32)):
        raise ValueError(f"{prefix}weight.quant_map is not bitsandbytes' NF4 code: custom quant maps are not supported")
    bias = state.get(prefix + "bias")
    shell = LinearFP4(K, M, bias=bias is not None, device="meta")
    qs = QuantState(absmax, (M, K), code, bs, getattr(torch, meta.get("dtype", "float16")), quant_type)
    shell._parameters["weight"] = Params4bit(packed, False, qs, bs, quant_type)
    if bias is not None:
        shell._parameters["bias"] = torch.nn.Parameter(bias.to(dev), requires_grad=False)
    return TorchFP4Linear(shell, use_codebook_dequant=use_codebook_dequant, name=name)


def save_fp4_model(model: torch.nn.Module, path: str, nested: bool = False) -> None:
    """``nested=False`` (the default) writes f32 absmax for every layer - a :class:`~torch_bnb_fp4.nested.NestedNF4Linear` as the
    scales it decodes to.  ``nested=True`` writes bitsandbytes' double-quantised layout instead: a NestedNF4Linear verbatim (it loads
    back bit for bit), an f32-absmax layer through ``ext.absmax_nest`` with offset = absmax.mean(), groups of 256 and the dynamic
    8-bit map - which is LOSSY: each scale moves by up to half the map's largest gap times its group's scale, so a model saved this
    way does not reproduce the outputs of the model it was saved from (it reproduces itself: what is loaded is what was written).

    Write every FP4 layer of ``model`` (bitsandbytes layout) and every other tensor of its ``state_dict`` to one safetensors
    file.  :class:`TorchFP4Linear` layers are written as they are; the fused layers of :mod:`torch_bnb_fp4.fused` are written as
    the plain projections they were built from (a gated MLP's interleaved gate|up weight is de-interleaved under the two names
    the unfused model uses), so the file always loads into a fresh, UNFUSED model with :func:`load_fp4_layers` - after which
    ``fuse_gated_mlps`` can be applied again.  A fused layer that cannot be expressed that way raises instead of being written as
    tensors no loader would recognise."""
    from safetensors.torch import save_file

    from .fused import FusedFP4Linear
    from .surgery import FusedGatedMLP

    # Tensor-parallel wrappers hold ONE RANK'S shard (row slices, re-packed column ranges, shard-wise concatenations): written as they
    # are they would read back as complete but wrong-sized plain layers, without the collective and without forward(x, residual).
    try:
        from . import parallel as _par

        tp_types = (_par.ColumnParallelFP4Linear, _par.RowParallelFP4Linear, _par.FusedColumnParallelFP4)
    except Exception:  # torch.distributed not built in: no such modules can exist in the model either
        tp_types = ()
    for name, mod in model.named_modules():
        if tp_types and isinstance(mod, tp_types):
            raise ValueError(f"save_fp4_model: '{name}' is a {type(mod).__name__} holding one rank's shard of its weight; save the "
                             "unsharded model (before the tensor-parallel layers are built) and shard again after loading")

    tensors: Dict[str, torch.Tensor] = {}
    fp4_prefixes = []
    gated = {}  # prefix of a FusedGatedMLP's gate_up child -> (prefix for gate, prefix for up, dtype)
    for name, mod in model.named_modules():
        if isinstance(mod, FusedGatedMLP):
            base = name + "." if name else ""
            gated[base + "gate_up."] = (base + mod.projection_names[0] + ".", base + mod.projection_names[1] + ".", mod.quant_dtype)
    for name, mod in model.named_modules():
        prefix = name + "." if name else ""
        if isinstance(mod, TorchFP4Linear):
            fp4_prefixes.append(prefix)
            tensors.update(fp4_linear_to_bnb_state(mod, prefix, nested))
        elif isinstance(mod, NestedNF4Linear):
            fp4_prefixes.append(prefix)
            tensors.update(nested_linear_to_bnb_state(mod, prefix, nested))
        elif isinstance(mod, FusedFP4Linear):
            fp4_prefixes.append(prefix)
            g = gated.get(prefix)
            tensors.update(fused_linear_to_bnb_state(mod, prefix, None if g is None else g[:2], None if g is None else g[2], nested))
    for key, val in model.state_dict().items():
        if not any(key.startswith(p) for p in fp4_prefixes):
            tensors[key] = val.detach().cpu().contiguous()
    save_file({k: v.contiguous() for k, v in tensors.items()}, path)


def load_fp4_layers(model: torch.nn.Module, path: str, device="cuda", use_codebook_dequant: bool = True,
                    strict: bool = True, nested: str = "expand") -> torch.nn.Module:
    """Replace, in ``model``, every ``nn.Linear`` for which ``path`` holds a bitsandbytes FP4 weight by a
    :class:`TorchFP4Linear` built from the stored bytes; the file's other tensors are loaded into the model.  Tensors of the
    file that the model has no place for raise a ``KeyError`` (``strict=False``: they are listed in ``model.fp4_unexpected_keys``
    instead) - a checkpoint is never half-applied silently.  Double-quantised weights: ``nested="expand"`` (default) decodes their
    statistics once into ordinary layers; ``nested="resident"`` keeps them compressed (:class:`~torch_bnb_fp4.nested.NestedNF4Linear`)
    where the nested GEMV covers the weight and expands the rest, whose names are listed in ``model.fp4_nested_expanded``."""
    from safetensors.torch import load_file

    state = load_file(path)
    prefixes = sorted(k[: -len(key)] for k in state for key in _STATE_KEYS.values() if k.endswith(key))
    consumed = set()
    nested_expanded = []
    if nested not in NESTED_MODES:
        raise ValueError(f"nested must be one of {NESTED_MODES}, got {nested!r}")
    for prefix in prefixes:
        parent_name, _, child = prefix.rstrip(".").rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        layer = fp4_linear_from_bnb_state(state, prefix, device, use_codebook_dequant, name=prefix.rstrip("."), nested=nested)
        if nested == "resident" and prefix + _NESTED_KEYS[0] in state and not isinstance(layer, NestedNF4Linear):
            nested_expanded.append(prefix.rstrip("."))
        if child:
            parent._modules[child] = layer
        else:
            model = layer
        consumed.update(k for k in state if k.startswith(prefix))
    rest = {k: v for k, v in state.items() if k not in consumed}
    unexpected = []
    if rest and isinstance(model, torch.nn.Module):
        unexpected = list(model.load_state_dict(rest, strict=False).unexpected_keys)
    if unexpected and strict:
        raise KeyError(f"load_fp4_layers: {len(unexpected)} tensor(s) of {path} have no place in the model (saved from a model with a "
                       f"different structure?): {unexpected[:8]}{' ...' if len(unexpected) > 8 else ''}")
    if isinstance(model, torch.nn.Module):
        model.fp4_unexpected_keys = unexpected
        model.fp4_nested_expanded = nested_expanded
    return model
