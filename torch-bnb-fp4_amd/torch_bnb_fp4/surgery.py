"""Model surgery: nn.Linear -> FP4 layer -> :class:`TorchFP4Linear`.

Counterpart of the reference's module-walking helpers (torch_bnb_fp4/__init__.py:717-922) with
the same names, keyword arguments and defaults.  The nn.Linear -> FP4 step, which the reference
delegates to bitsandbytes (``bnb.nn.LinearFP4`` + ``Params4bit.cuda()``), uses this package's own
:class:`~torch_bnb_fp4.nn.LinearFP4` and HIP quantiser, so no bitsandbytes install is needed.
"""
from __future__ import annotations

import logging
from typing import List, Optional, TypeVar

import torch
from torch import nn

from .functional import quantize_fp4
from .linear import TorchFP4Linear
from .nn import FP4_LINEAR_TYPES, LinearFP4, Params4bit, QuantState, fp4_code

T_Model = TypeVar("T_Model", bound=nn.Module)
log = logging.getLogger(__name__)


@torch.no_grad()
def swap_linear_with_bnb_linear(linear: nn.Linear, dtype=torch.float16, quant_type: str = "fp4") -> LinearFP4:
    """New (still dense) ``LinearFP4`` holding clones of ``linear``'s weight and bias; it quantises
    when moved to a GPU (reference :717-747).  ``quant_type="nf4"`` (not in the reference) quantises to NF4."""
    # built on the meta device: nn.Linear.__init__ would otherwise allocate and randomly initialise a full dense
    # weight on the CPU only to have it replaced (18 s of a 7B model's 224 layers)
    fp4 = LinearFP4(input_features=linear.in_features, output_features=linear.out_features,
                    bias=linear.bias is not None, compute_dtype=dtype, device="meta", quant_type=quant_type)
    fp4.weight = Params4bit(linear.weight.data.clone().detach(), False, None, fp4.blocksize, quant_type)
    if linear.bias is not None:
        fp4.bias = nn.Parameter(linear.bias.data.clone().detach(), requires_grad=False)
    fp4.requires_grad_(False)
    return fp4


def check_if_name_contained_in_list(name: str, names_list) -> bool:
    """True when any entry of ``names_list`` is a substring of ``name`` (reference :750-756)."""
    return any(entry in name for entry in names_list)


def todevice_if_necessary(module, device):
    """Make sure an FP4 layer's weight really is packed uint8 on ``device``; quantise it directly
    if moving the module did not (reference :759-778)."""
    if module.weight.data.dtype != torch.uint8 and isinstance(module, FP4_LINEAR_TYPES):
        module = module.to(device)
        w = module.weight
        if not (w.data.device == torch.device(device) and w.data.dtype == torch.uint8):
            log.debug("layer was not quantised by the device move; quantising its weight directly")
            if getattr(module, "quant_type", "fp4") == "nf4":
                module.weight = Params4bit.quantized_from(w.data, device, module.blocksize, "nf4")
                return module
            dense = w.data.to(device=device, dtype=torch.float16)
            packed, absmax = quantize_fp4(dense, module.blocksize)
            state = QuantState(absmax, dense.shape, fp4_code().to(device), module.blocksize, w.data.dtype)
            module.weight = Params4bit(packed, False, state, module.blocksize, "fp4")
    return module


def _device_is_gpu(device) -> bool:
    kind = device.type if hasattr(device, "type") else str(device).split(":")[0]
    return kind == "cuda"


def _to_fp4_linear(layer: nn.Module, device, as_dtype, use_codebook_dequant: bool, name: str, quant_type: str = "fp4") -> TorchFP4Linear:
    """nn.Linear or FP4 layer -> TorchFP4Linear on ``device`` (a dense nn.Linear is quantised to ``quant_type``)."""
    if not isinstance(layer, FP4_LINEAR_TYPES):
        layer = swap_linear_with_bnb_linear(layer, dtype=as_dtype, quant_type=quant_type)
    layer = layer.to(device)
    if getattr(layer.weight, "quant_state", None) is None:
        layer = todevice_if_necessary(layer, device)
    return TorchFP4Linear(lin=layer, use_codebook_dequant=use_codebook_dequant, name=name)


def recursively_replace_with_fp4_linear(
    module: T_Model,
    as_dtype=torch.float16,
    use_codebook_dequant=True,
    device: torch.device = torch.device("cuda" if torch.cuda.is_available() else "cpu"),
    return_final_module: bool = True,
    only_replace_bnb_layers: bool = False,
    ignore_layer_names: List[str] = ["lm_head"],
    parent="",
    debug: bool = False,
    quant_type: str = "fp4",
) -> Optional[T_Model]:
    """Replace every nn.Linear / FP4 linear below ``module`` by a :class:`TorchFP4Linear`.

    Same contract as the reference (:781-922): children whose *own* name contains an entry of
    ``ignore_layer_names`` are skipped together with their subtree; ``only_replace_bnb_layers``
    leaves plain nn.Linear alone; a root that is itself a Linear is converted and returned;
    ``named_children()`` dedupes shared modules, so a Linear object reused in several slots is
    swapped only in the first one (the reference's sanity model relies on exactly that).
    ``quant_type`` (not in the reference): the code dense nn.Linear layers are quantised to, ``"fp4"`` or ``"nf4"``;
    layers that are already 4-bit keep their own.
    """
    assert _device_is_gpu(device), "Device type must be cuda!"
    prefix = parent + "." if parent != "" else ""
    swapped_dense = False
    for name, child in module.named_children():
        child_name = prefix + name
        if check_if_name_contained_in_list(name, ignore_layer_names):
            if debug:
                print(f"Ignoring name: {child_name}, as it is in the ignore list")
            continue
        if isinstance(child, (nn.Linear,) + FP4_LINEAR_TYPES):
            is_fp4 = isinstance(child, FP4_LINEAR_TYPES)
            if not is_fp4 and only_replace_bnb_layers:
                if debug:
                    print(f"Ignoring {child_name}, as only_replace_bnb_layers=True")
                continue
            if debug:
                print(f"Replacing {'FP4 layer ' if is_fp4 else ''}{child_name} with TorchFP4Linear.")
            module._modules[name] = _to_fp4_linear(child, device, as_dtype, use_codebook_dequant, child_name, quant_type)
            swapped_dense |= not is_fp4
        elif isinstance(child, nn.Module):
            recursively_replace_with_fp4_linear(child, as_dtype=as_dtype, use_codebook_dequant=use_codebook_dequant,
                                                device=device, return_final_module=False,
                                                only_replace_bnb_layers=only_replace_bnb_layers,
                                                ignore_layer_names=ignore_layer_names, parent=child_name, debug=debug,
                                                quant_type=quant_type)
    if isinstance(module, (nn.Linear,) + FP4_LINEAR_TYPES):
        is_fp4 = isinstance(module, FP4_LINEAR_TYPES)
        if is_fp4 or not only_replace_bnb_layers:
            if debug:
                print(f"Replacing {parent} with TorchFP4Linear.")
            module = _to_fp4_linear(module, device, as_dtype, use_codebook_dequant, parent, quant_type)
            swapped_dense |= not is_fp4
        elif debug:
            print(f"Ignoring {parent}, as only_replace_bnb_layers=True")
    if swapped_dense:
        torch.cuda.empty_cache()  # the dense copies are gone; give their blocks back (:919-920)
    if return_final_module:
        return module


def set_small_batch_fused(module: nn.Module, enabled: bool = True, nf4: bool = False, nf4_wide: bool = False) -> int:
    """Route 2..128 activation rows of every :class:`TorchFP4Linear` below ``module`` to the fused small-batch kernels
    (``enabled=True``) or back to the reference's dispatch, dequant + GEMM for every batch > 1
    (torch_bnb_fp4/__init__.py:592,616-617; the default, so that a converted model behaves like the reference's).
    Not part of the reference surface.  Returns the number of layers touched.  Batched decode through Mistral-7B shapes:
    3 237 tok/s fused vs 963 tok/s through the reference dispatch at 8 sequences (profiles/).  NF4 layers are left on
    dequant + GEMM (the FP4 small-batch kernels decode FP4 only) and not counted, unless ``nf4=True``: then every NF4 layer's
    ``small_batch_fused_nf4`` is set as well - 2..16 rows of fp16 / bf16 activations go to the fused NF4 matrix-core kernel
    (blocksize 64, K % 512 == 0; anything else stays on dequant + GEMM) - and those layers are counted too.  ``nf4_wide=True``
    sets every NF4 layer's ``wide_batch_fused_nf4``: 17..64 rows, and 2..16 rows where K % 512 != 0, go to the one-pass NF4
    kernel (``ext.gemm_wide_nf4``; blocksize 64, K % 64 == 0); an NF4 layer is counted once whichever of the two is set.
    A resident :class:`~torch_bnb_fp4.nested.NestedNF4Linear` (NF4, statistics compressed on the device) takes the two NF4 switches
    the same way and is counted like an NF4 layer: the same cells then run ``ext.gemm_nf4_nested`` instead of its expand path."""
    from .nested import NestedNF4Linear

    n = 0
    for m in module.modules():
        if isinstance(m, NestedNF4Linear):
            if nf4 or nf4_wide:
                if nf4:
                    m.small_batch_fused_nf4 = bool(enabled)
                if nf4_wide:
                    m.wide_batch_fused_nf4 = bool(enabled)
                n += 1
            continue
        if not isinstance(m, TorchFP4Linear):
            continue
        if not m.quant_data.nf4:
            m.quant_data.small_batch_fused = bool(enabled)
            n += 1
        elif nf4 or nf4_wide:
            if nf4:
                m.quant_data.small_batch_fused_nf4 = bool(enabled)
            if nf4_wide:
                m.quant_data.wide_batch_fused_nf4 = bool(enabled)
            n += 1
    return n



class FusedGatedMLP(nn.Module):
    """``down(silu(gate(x)) * up(x))`` with the gate and up projections as ONE launch whose epilogue applies the activation
    and the product (:mod:`torch_bnb_fp4.fused`); what :func:`fuse_gated_mlps` puts in place of a Llama / Mistral style MLP.
    An NF4 gate / up pair becomes a :class:`~torch_bnb_fp4.fused.FusedNF4Linear`; a pair of different codes is refused."""

    def __init__(self, gate: TorchFP4Linear, up: TorchFP4Linear, down: nn.Module, names=("gate_proj", "up_proj")):
        super().__init__()
        from .fused import FusedFP4Linear, FusedNF4Linear

        self.gate_up = (FusedNF4Linear if gate.quant_data.nf4 and up.quant_data.nf4 else FusedFP4Linear).gate_up(gate, up)
        self.down_proj = down
        # the two projections' names in the unfused model: save_fp4_model writes the interleaved weight back under them
        # (bitsandbytes layout, one entry per projection), so that the file loads into a fresh, unfused model
        self.projection_names = (str(names[0]), str(names[1]))
        self.quant_dtype = gate.quant_data.quant_state.dtype

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.down_proj(self.gate_up(x))


def fuse_gated_mlps(module: nn.Module, gate: str = "gate_proj", up: str = "up_proj", down: str = "down_proj", act: str = "act_fn",
                    nf4: bool = False) -> int:
    """After :func:`recursively_replace_with_fp4_linear`: replace every sub-module that looks like a SiLU-gated MLP (children
    ``gate`` / ``up`` / ``down`` with the first two :class:`TorchFP4Linear` of equal shape, activation ``act`` a SiLU) by a
    :class:`FusedGatedMLP`.  Single-token calls then pay one launch for gate + up + activation + product instead of four; other
    shapes run the unfused sequence.  Returns how many were replaced.  Not in the reference (its surface stops at the Linear).
    NF4 MLPs are left alone unless ``nf4=True`` (then their gate / up pair becomes a ``FusedNF4Linear``); a pair whose two
    projections use different codes is never fused.  Resident :class:`~torch_bnb_fp4.nested.NestedNF4Linear` projections are
    ignored: a compressed group spans rows, so interleaving them would re-quantise (``expand_nested`` first)."""
    count = 0
    for name, child in list(module.named_children()):
        g, u, d, a = (getattr(child, n, None) for n in (gate, up, down, act))
        silu = isinstance(a, nn.SiLU) or "silu" in type(a).__name__.lower() or a is nn.functional.silu
        if (isinstance(g, TorchFP4Linear) and isinstance(u, TorchFP4Linear) and isinstance(d, nn.Module) and silu
                and g.quant_data.nf4 == u.quant_data.nf4 and (nf4 or not g.quant_data.nf4)  # NF4 pairs on request, mixed pairs never
                and (g.quant_data.M, g.quant_data.N, g.quant_data.blocksize) == (u.quant_data.M, u.quant_data.N, u.quant_data.blocksize)
                ):
            module._modules[name] = FusedGatedMLP(g, u, d, names=(gate, up))
            count += 1
        else:
            count += fuse_gated_mlps(child, gate, up, down, act, nf4)
    return count


# ---- LoRA adapters beside NF4 weights (QLoRA serving) ---------------------------------------------------------------------------------
def _adapter_tensors(adapter_state) -> dict:
    """peft's saved keys -> {module path: {"A": tensor, "B": tensor}}.  Keys look like
    ``base_model.model.<path>.lora_A.weight`` or, with an adapter-name segment, ``base_model.model.<path>.lora_A.<name>.weight``."""
    out = {}
    for key, tensor in adapter_state.items():
        parts = key.split(".")
        which = next((i for i, p in enumerate(parts) if p in ("lora_A", "lora_B")), None)
        if which is None or parts[-1] != "weight" or len(parts) - which not in (2, 3):
            raise KeyError(f"not a LoRA adapter key: {key!r} (expected <path>.lora_A.weight / <path>.lora_B.weight)")
        path = parts[:which]
        if path[:2] == ["base_model", "model"]:
            path = path[2:]
        slot = out.setdefault(".".join(path), {})
        if parts[which][-1] in slot:
            raise KeyError(f"two tensors for {'.'.join(path)}.{parts[which]}: one adapter at a time")
        slot[parts[which][-1]] = tensor
    for path, slot in out.items():
        if set(slot) != {"A", "B"}:
            raise KeyError(f"adapter for {path!r} lacks lora_{'B' if 'A' in slot else 'A'}")
    return out


def _resolve(model: nn.Module, path: str):
    """(parent module, child name, child) for a dotted path, or None.  A path into a :class:`FusedGatedMLP` names one of the two
    projections it replaced: then the child is the FusedGatedMLP itself."""
    parent, parts = model, path.split(".")
    for i, name in enumerate(parts):
        if isinstance(parent, FusedGatedMLP) and i == len(parts) - 1 and name in parent.projection_names:
            return parent, name, parent
        child = parent._modules.get(name) if isinstance(parent, nn.Module) else None
        if child is None:
            return None
        if i == len(parts) - 1:
            return parent, name, child
        parent = child
    return None


def attach_lora(model: nn.Module, adapter_state, r: int, lora_alpha: float, use_rslora: bool = False, target_modules=None) -> int:
    """Attach a saved LoRA adapter to the NF4 layers of ``model``: every NF4 :class:`TorchFP4Linear` (or
    :class:`~torch_bnb_fp4.fused.FusedNF4Linear`) an adapter key names becomes a :class:`~torch_bnb_fp4.fused.LoRANF4Linear`, and
    the gate|up layer of an NF4 :class:`FusedGatedMLP` (``fuse_gated_mlps(model, nf4=True)``) takes the gate and the up adapter
    stacked (a projection without one gets a zero adapter).  A resident :class:`~torch_bnb_fp4.nested.NestedNF4Linear` becomes a
    :class:`~torch_bnb_fp4.nested.LoRANestedNF4Linear` and is counted too, its statistics still compressed (several adapters at
    once, :func:`attach_lora_adapters`, stay expand-first: ``expand_nested`` before them).  ``adapter_state`` uses peft's saved key names, with or without the
    ``base_model.model.`` prefix and an adapter-name segment; the factor is ``lora_alpha / r`` (``/ sqrt(r)`` with
    ``use_rslora``).  ``target_modules`` (names, as in peft's config) restricts which keys are used; a key that is used but has no
    NF4 home in ``model`` raises, and a call that raises leaves ``model`` as it was.  Adapters are not merged: 4-bit weights cannot absorb them without re-quantising.  Returns the
    number of layers replaced.  peft itself is not needed."""
    from .fused import FusedNF4Linear, LoRANF4Linear, lora_scaling
    from .nested import LoRANestedNF4Linear, NestedNF4Linear

    scaling = lora_scaling(r, lora_alpha, use_rslora)
    adapters = _adapter_tensors(adapter_state)
    if target_modules is not None:
        names = [target_modules] if isinstance(target_modules, str) else list(target_modules)
        adapters = {p: t for p, t in adapters.items() if any(p == n or p.endswith("." + n) for n in names)}
    gated = {}  # id(FusedGatedMLP) -> (module, {"gate": adapter, "up": adapter})
    plan = []  # (parent, attribute, new layer): every key is checked and every layer built before the model is touched
    for path, slot in adapters.items():
        found = _resolve(model, path) or (_resolve(model, path[len("model."):]) if path.startswith("model.") else None)
        if found is None:
            raise KeyError(f"adapter key for {path!r}: the model has no such module")
        parent, name, child = found
        A, B = slot["A"], slot["B"]
        if A.shape[0] != r or B.shape[1] != r:
            raise ValueError(f"adapter for {path!r} has rank {A.shape[0]} / {B.shape[1]}, the config says r = {r}")
        if isinstance(child, FusedGatedMLP):
            if not isinstance(child.gate_up, FusedNF4Linear):
                raise ValueError(f"adapter key for {path!r}: the fused MLP there is not NF4")
            which = "gate" if name == child.projection_names[0] else "up"
            gated.setdefault(id(child), (child, {}))[1][which] = (A, B, scaling)
        elif isinstance(child, TorchFP4Linear) and child.quant_data.nf4:
            plan.append((parent, name, LoRANF4Linear.from_linear(child, A, B, scaling)))
        elif type(child) is FusedNF4Linear:
            plan.append((parent, name, LoRANF4Linear.from_fused(child, A, B, scaling)))
        elif type(child) is NestedNF4Linear:
            plan.append((parent, name, LoRANestedNF4Linear.from_nested(child, A, B, scaling)))
        else:
            raise ValueError(f"adapter key for {path!r}: {type(child).__name__} is not an NF4 layer (quantise the model with "
                             f"quant_type='nf4' first; an adapter is attached once)")
    for mlp, pair in gated.values():
        gu = mlp.gate_up
        if isinstance(gu, LoRANF4Linear):
            raise ValueError("this fused MLP already carries an adapter")
        M, K = gu.out_features, gu.in_features
        ref = next(iter(pair.values()))[0]
        zero = (ref.new_zeros(r, K), ref.new_zeros(M, r), 0.0)
        plan.append((mlp, "gate_up", LoRANF4Linear.gate_up_from_fused(gu, pair.get("gate", zero), pair.get("up", zero))))
    for parent, name, layer in plan:
        parent._modules[name] = layer
    return len(plan)


def load_lora_adapter(model: nn.Module, directory: str) -> int:
    """:func:`attach_lora` from a directory in peft's layout: ``adapter_model.safetensors`` and ``adapter_config.json`` (``r``,
    ``lora_alpha``, ``use_rslora``, ``target_modules``)."""
    import json
    import os

    from safetensors.torch import load_file

    with open(os.path.join(directory, "adapter_config.json")) as f:
        cfg = json.load(f)
    state = load_file(os.path.join(directory, "adapter_model.safetensors"))
    return attach_lora(model, state, int(cfg["r"]), float(cfg["lora_alpha"]), bool(cfg.get("use_rslora", False)),
                       cfg.get("target_modules"))


def attach_lora_adapters(model: nn.Module, adapters, target_modules=None):
    """Attach several saved LoRA adapters at once, selectable per sequence: ``adapters`` is an ordered mapping
    ``name -> (adapter_state, r, lora_alpha, use_rslora)``.  Every NF4 layer that some adapter's keys name becomes a
    :class:`~torch_bnb_fp4.fused.MultiLoRANF4Linear` holding all of them in the mapping's order (the gate|up layer of an NF4
    :class:`FusedGatedMLP` takes each adapter's gate and up parts stacked); an adapter that does not cover a target module gets a
    zero slice there.  Key mapping, ``target_modules`` and the rule that a used key without an NF4 home raises (leaving ``model`` as
    it was) are :func:`attach_lora`'s.  Returns the one :class:`~torch_bnb_fp4.fused.AdapterSelection` all new layers share; it
    carries the adapters' ``names`` (``selection.set_by_name([...])``) and ``n_layers``, the number of layers replaced."""
    return _attach_adapter_stack(model, [(name, *spec, target_modules) for name, spec in adapters.items()])


def _attach_adapter_stack(model: nn.Module, entries):
    """attach_lora_adapters over ``(name, adapter_state, r, lora_alpha, use_rslora, target_modules)`` entries, each with its own
    ``target_modules`` (load_lora_adapters reads them per adapter)."""
    from .fused import AdapterSelection, FusedNF4Linear, LoRANF4Linear, MultiLoRANF4Linear, lora_scaling

    names = [e[0] for e in entries]
    if not names:
        raise ValueError("attach_lora_adapters needs at least one adapter")
    targets = {}  # resolved (id(parent), attribute) -> [parent, attribute, child, {adapter index: (A, B, scaling)}]
    for index, (name, state, r, lora_alpha, use_rslora, wanted) in enumerate(entries):
        scaling = lora_scaling(r, lora_alpha, use_rslora)
        tensors = _adapter_tensors(state)
        if wanted is not None:
            wanted = [wanted] if isinstance(wanted, str) else list(wanted)
            tensors = {p: t for p, t in tensors.items() if any(p == n or p.endswith("." + n) for n in wanted)}
        for path, slot in tensors.items():
            found = _resolve(model, path) or (_resolve(model, path[len("model."):]) if path.startswith("model.") else None)
            if found is None:
                raise KeyError(f"adapter {name!r}, key for {path!r}: the model has no such module")
            parent, attr, child = found
            A, B = slot["A"], slot["B"]
            if A.shape[0] != r or B.shape[1] != r:
                raise ValueError(f"adapter {name!r} for {path!r} has rank {A.shape[0]} / {B.shape[1]}, the config says r = {r}")
            if isinstance(child, FusedGatedMLP):
                if not isinstance(child.gate_up, FusedNF4Linear):
                    raise ValueError(f"adapter key for {path!r}: the fused MLP there is not NF4")
                if isinstance(child.gate_up, (LoRANF4Linear, MultiLoRANF4Linear)):
                    raise ValueError("this fused MLP already carries an adapter")
                which = "gate" if attr == child.projection_names[0] else "up"
                entry = targets.setdefault((id(child), "gate_up"), [child, "gate_up", child.gate_up, {}])
                entry[3].setdefault(index, {})[which] = (A, B, scaling)
            elif (isinstance(child, TorchFP4Linear) and child.quant_data.nf4) or type(child) is FusedNF4Linear:
                targets.setdefault((id(parent), attr), [parent, attr, child, {}])[3][index] = (A, B, scaling)
            else:
                raise ValueError(f"adapter key for {path!r}: {type(child).__name__} is not an NF4 layer (quantise the model with "
                                 f"quant_type='nf4' first; adapters are attached once)")
    if not targets:
        raise ValueError("no adapter key names a target module")
    device = next(iter(targets.values()))[2].quant_data.A.device
    selection = AdapterSelection(device, names)
    plan = []
    for parent, attr, child, per_adapter in targets.values():
        ref = next(iter(per_adapter.values()))
        if attr == "gate_up" and isinstance(parent, FusedGatedMLP):
            M, K = child.out_features, child.in_features
            ref = next(iter(ref.values()))[0]
            zero = (ref.new_zeros(1, K), ref.new_zeros(M, 1), 0.0)
            pairs = [(per_adapter.get(i, {}).get("gate", zero), per_adapter.get(i, {}).get("up", zero)) for i in range(len(names))]
            plan.append((parent, attr, MultiLoRANF4Linear.gate_up_from_fused(child, pairs, selection)))
        else:
            qd = child.quant_data
            zero = (ref[0].new_zeros(1, int(qd.N)), ref[0].new_zeros(int(qd.M), 1), 0.0)
            stack = [per_adapter.get(i, zero) for i in range(len(names))]
            make = MultiLoRANF4Linear.from_linear if isinstance(child, TorchFP4Linear) else MultiLoRANF4Linear.from_fused
            plan.append((parent, attr, make(child, stack, selection)))
    for parent, attr, layer in plan:
        parent._modules[attr] = layer
    selection.n_layers = len(plan)
    return selection


def load_lora_adapters(model: nn.Module, directories):
    """:func:`attach_lora_adapters` from directories in peft's layout (``adapter_model.safetensors`` + ``adapter_config.json``):
    ``directories`` is an ordered mapping ``name -> directory`` or a sequence of directories (named by their last path component).
    Each adapter's own ``target_modules`` restricts its keys."""
    import json
    import os

    from safetensors.torch import load_file

    if not hasattr(directories, "items"):
        directories = {os.path.basename(os.path.normpath(d)): d for d in directories}
    entries = []
    for name, directory in directories.items():
        with open(os.path.join(directory, "adapter_config.json")) as f:
            cfg = json.load(f)
        state = load_file(os.path.join(directory, "adapter_model.safetensors"))
        entries.append((name, state, int(cfg["r"]), float(cfg["lora_alpha"]), bool(cfg.get("use_rslora", False)), cfg.get("target_modules")))
    return _attach_adapter_stack(model, entries)
