"""The adapter store of multi-LoRA serving: slot stacks for every projection group of every layer, and the PEFT loader.

With `EngineConfig.max_loras > 0` the model allocates, per layer and per weight tensor of `LlamaTransformerLayerWeight`
(fused: qkv, o, up_gate, down; `fuse_qkv=False`: q, k, v instead of qkv), the zero-filled stacks of kernels/lora.LoraGroup —
before the KV pool is sized, so the pool is sized with them. An adapter is a PEFT directory (`adapter_config.json` +
`adapter_model.safetensors`) or a state dict + config of the same content; loading copies its matrices into one free slot
(rank below `max_lora_rank`: zero-padded; a target module that is absent: stays zero), unloading zeroes the slot. `peft` is
not imported. Everything the LoRA layer path cannot serve is refused here, on the host, with the reason.
"""
import json
import os
import re
from typing import Dict, List, Optional

import torch

from .kernels.lora import LoraBatch, LoraGroup, LoraStaging, SUPPORTED_RANKS, group_supported

# PEFT target modules under `self_attn` (the others — up_proj, gate_proj, down_proj — live under `mlp`)
_ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
_KEY = re.compile(r"^base_model\.model\.model\.layers\.(\d+)\.(self_attn|mlp)\.(\w+)\.lora_([AB])\.weight$")


class LoraError(ValueError):
    """An adapter (or a LoRA configuration) this engine refuses; the message says why."""


def layer_groups(cfg, fuse_qkv: bool):
    """[(attribute of the layer weight, PEFT module names of its parts, part widths, K)] for one layer."""
    h, hq, hkv, inter = cfg.hidden_size, cfg.num_q_heads * cfg.head_dim, cfg.num_kv_heads * cfg.head_dim, cfg.ffn_inter_dim
    attn = ([("qkv_proj", ("q_proj", "k_proj", "v_proj"), (hq, hkv, hkv), h)] if fuse_qkv else
            [("q_proj", ("q_proj",), (hq,), h), ("k_proj", ("k_proj",), (hkv,), h), ("v_proj", ("v_proj",), (hkv,), h)])
    return attn + [("o_proj", ("o_proj",), (h,), hq),
                   ("up_gate_proj", ("up_proj", "gate_proj"), (inter, inter), h),      # [up ; gate], as the weight
                   ("down_proj", ("down_proj",), (h,), inter)]


class LoraLayer:
    """The groups of one transformer layer, by the attribute name of the weight tensor they update."""

    def __init__(self, groups: Dict[str, LoraGroup]):
        self.groups = groups

    def __getattr__(self, name):
        try:
            return self.__dict__["groups"][name]
        except KeyError:
            raise AttributeError(name) from None


class LoraStore:
    def __init__(self, model_config, max_loras: int, max_lora_rank: int, dtype: torch.dtype, device, fuse_qkv: bool = True):
        if max_loras <= 0:
            raise LoraError("max_loras must be > 0 for an adapter store")
        if max_lora_rank not in SUPPORTED_RANKS:
            raise LoraError(f"max_lora_rank must be one of {list(SUPPORTED_RANKS)}, got {max_lora_rank}")
        self.model_config, self.max_loras, self.r_max = model_config, int(max_loras), int(max_lora_rank)
        self.dtype, self.device = dtype, device
        spec = layer_groups(model_config, fuse_qkv)
        for attr, _, widths, k in spec:
            if not group_supported(k, widths, self.r_max):
                raise LoraError(f"the LoRA kernels do not take the {attr} projection of this model (K = {k} must be a "
                                f"multiple of 128, the output parts {list(widths)} multiples of 16)")
        self.layers: List[LoraLayer] = [
            LoraLayer({attr: LoraGroup(names, widths, k, self.max_loras, self.r_max, dtype, device)
                       for attr, names, widths, k in spec})
            for _ in range(model_config.num_layers)]
        # PEFT module name -> (group attribute, part index)
        self._where = {name: (attr, i) for attr, names, _, _ in spec for i, name in enumerate(names)}
        self._slots: Dict[str, int] = {}

    # ---- bookkeeping ------------------------------------------------------------------------------------------------
    def names(self) -> Dict[str, int]:
        """Loaded adapters: name -> slot."""
        return dict(self._slots)

    def slot_of(self, name: str) -> int:
        try:
            return self._slots[name]
        except KeyError:
            raise LoraError(f"unknown LoRA adapter {name!r} (loaded: {sorted(self._slots)})") from None

    def nbytes(self) -> int:
        return sum(g.nbytes() for layer in self.layers for g in layer.groups.values())

    # ---- loading ----------------------------------------------------------------------------------------------------
    @staticmethod
    def read_peft_dir(path: str):
        cfg_path = os.path.join(path, "adapter_config.json")
        st_path = os.path.join(path, "adapter_model.safetensors")
        if not os.path.isfile(cfg_path) or not os.path.isfile(st_path):
            raise LoraError(f"{path} is not a PEFT adapter directory (adapter_config.json + adapter_model.safetensors)")
        with open(cfg_path, "r", encoding="utf-8") as f:
            config = json.load(f)
        from safetensors.torch import load_file
        return load_file(st_path, device="cpu"), config

    def _check_config(self, name: str, config: dict) -> int:
        if config.get("peft_type", "LORA") != "LORA":
            raise LoraError(f"adapter {name!r}: peft_type {config.get('peft_type')!r} is not LORA")
        for flag in ("use_dora", "use_rslora"):
            if config.get(flag):
                raise LoraError(f"adapter {name!r}: {flag} adapters are not supported")
        if config.get("modules_to_save"):
            raise LoraError(f"adapter {name!r}: modules_to_save ({config['modules_to_save']}) is not supported: an adapter "
                            "may only add low-rank updates to the layer projections")
        if config.get("bias", "none") != "none":
            raise LoraError(f"adapter {name!r}: bias={config.get('bias')!r} is not supported (only 'none')")
        r = config.get("r")
        if not isinstance(r, int) or isinstance(r, bool) or r <= 0:
            raise LoraError(f"adapter {name!r}: adapter_config.json needs a positive integer rank 'r'")
        if r > self.r_max:
            raise LoraError(f"adapter {name!r}: rank {r} exceeds max_lora_rank ({self.r_max})")
        if config.get("rank_pattern") or config.get("alpha_pattern"):
            raise LoraError(f"adapter {name!r}: rank_pattern / alpha_pattern are not supported (one rank and alpha)")
        alpha = config.get("lora_alpha", r)
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)):
            raise LoraError(f"adapter {name!r}: lora_alpha must be a number")
        targets = config.get("target_modules") or []
        if isinstance(targets, str):
            targets = [targets]
        for t in targets:
            leaf = str(t).split(".")[-1]
            if leaf in ("embed_tokens", "lm_head"):
                raise LoraError(f"adapter {name!r}: embedding / lm_head adapters ({t}) are not supported")
            if leaf not in self._where:
                raise LoraError(f"adapter {name!r}: unknown target module {t!r} (known: {sorted(self._where)})")
        return r

    def load(self, name: str, path: Optional[str] = None, *, state_dict: Optional[dict] = None,
             config: Optional[dict] = None) -> int:
        """Copy the adapter into a free slot and return the slot. Everything is checked before anything is written."""
        if not isinstance(name, str) or not name:
            raise LoraError("an adapter name is a non-empty string")
        if name in self._slots:
            raise LoraError(f"a LoRA adapter named {name!r} is already loaded")
        if (path is None) == (state_dict is None):
            raise LoraError("load_lora takes a PEFT directory or a state_dict + config, not both")
        if path is not None:
            state_dict, config = self.read_peft_dir(path)
        if config is None:
            raise LoraError("load_lora with a state_dict needs its adapter config")
        r = self._check_config(name, config)
        free = [s for s in range(self.max_loras) if s not in self._slots.values()]
        if not free:
            raise LoraError(f"no free LoRA slot for {name!r}: {self.max_loras} adapters are loaded (max_loras)")
        cfg = self.model_config
        todo = {}       # (layer, module) -> [A, B]
        for key, tensor in state_dict.items():
            if "embed_tokens" in key or "lm_head" in key:
                raise LoraError(f"adapter {name!r}: embedding / lm_head adapters ({key}) are not supported")
            m = _KEY.match(key)
            if m is None:
                raise LoraError(f"adapter {name!r}: unexpected tensor {key!r}")
            layer, block, module, ab = int(m.group(1)), m.group(2), m.group(3), m.group(4)
            if module not in self._where or (block == "self_attn") != (module in _ATTN):
                raise LoraError(f"adapter {name!r}: unknown target module {block}.{module} ({key})")
            if layer >= cfg.num_layers:
                raise LoraError(f"adapter {name!r}: {key} names layer {layer}, the model has {cfg.num_layers}")
            todo.setdefault((layer, module), [None, None])[0 if ab == "A" else 1] = tensor
        for (layer, module), (a, b) in todo.items():
            attr, part = self._where[module]
            g = self.layers[layer].groups[attr]
            n_begin, n_end, _ = g.parts[part]
            if a is None or b is None:
                raise LoraError(f"adapter {name!r}: layer {layer} {module} has only one of lora_A / lora_B")
            if tuple(a.shape) != (r, g.k) or tuple(b.shape) != (n_end - n_begin, r):
                raise LoraError(f"adapter {name!r}: layer {layer} {module} has lora_A {tuple(a.shape)} / lora_B "
                                f"{tuple(b.shape)}, this model needs ({r}, {g.k}) / ({n_end - n_begin}, {r})")
        slot = free[0]
        self._zero_slot(slot)
        for (layer, module), (a, b) in todo.items():
            attr, part = self._where[module]
            g = self.layers[layer].groups[attr]
            n_begin, n_end, t_off = g.parts[part]
            g.a_stack[slot, t_off:t_off + r].copy_(a.to(self.dtype))
            g.b_stack[slot, n_begin:n_end, :r].copy_(b.to(self.dtype))
        scale = float(config.get("lora_alpha", r)) / r
        for layer in self.layers:
            for g in layer.groups.values():
                g.scale[slot:slot + 1].fill_(scale)     # (a device fill: no host-to-device copy per group)
        self._slots[name] = slot
        return slot

    def _zero_slot(self, slot: int):
        for layer in self.layers:
            for g in layer.groups.values():
                g.a_stack[slot].zero_()
                g.b_stack[slot].zero_()
                g.scale[slot:slot + 1].zero_()

    def unload(self, name: str) -> int:
        """Zero the adapter's slot and free it; returns the slot."""
        slot = self.slot_of(name)
        self._zero_slot(slot)
        del self._slots[name]
        return slot


class LoraStep:
    """What a LoRA step hands to the layers (LlamaInferState.lora): the row grouping on the device and the slot stacks."""
    __slots__ = ("batch", "layers")

    def __init__(self, batch: LoraBatch, layers: List[LoraLayer]):
        self.batch, self.layers = batch, layers


def rows_of_sequences(seq_slots: List[int], prefill_lens: List[int]) -> List[int]:
    """Per-row slots of a step: every token of a prompt (or chunk) takes its sequence's slot, a decoding sequence has
    one row. `seq_slots` is aligned with the step's sequences (prefill sequences first), `prefill_lens` with the first."""
    rows: List[int] = []
    for i, s in enumerate(seq_slots):
        rows += [s] * (prefill_lens[i] if i < len(prefill_lens) else 1)
    return rows


def parse_lora_modules(specs) -> Dict[str, str]:
    """["NAME=PATH", ...] -> {name: path} (EngineConfig.lora_modules, --lora)."""
    out = {}
    for spec in specs or ():
        name, sep, path = str(spec).partition("=")
        if not sep or not name or not path:
            raise LoraError(f"--lora takes NAME=PATH, got {spec!r}")
        if name in out:
            raise LoraError(f"--lora names {name!r} twice")
        out[name] = path
    return out
