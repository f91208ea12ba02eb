"""Shared builders of the multi-LoRA tests (tests/test_lora_host.py, tests/test_gpu_lora.py): adapters in PEFT layout and
exactly merged checkpoints. No device is touched here."""
import json
import os

import torch

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP = ("up_proj", "gate_proj", "down_proj")


def module_shapes(cfg: dict) -> dict:
    """PEFT target module -> (N, K) of the projection it adapts."""
    h, inter = cfg["hidden_size"], cfg["intermediate_size"]
    hd = h // cfg["num_attention_heads"]
    kv = cfg.get("num_key_value_heads", cfg["num_attention_heads"]) * hd
    return dict(q_proj=(h, h), k_proj=(kv, h), v_proj=(kv, h), o_proj=(h, h), up_proj=(inter, h), gate_proj=(inter, h),
                down_proj=(h, inter))


def peft_key(layer: int, module: str, ab: str) -> str:
    block = "self_attn" if module in ATTN else "mlp"
    return f"base_model.model.model.layers.{layer}.{block}.{module}.lora_{ab}.weight"


def weight_key(layer: int, module: str) -> str:
    block = "self_attn" if module in ATTN else "mlp"
    return f"model.layers.{layer}.{block}.{module}.weight"


def adapter_config(rank: int, alpha=None, modules=ATTN + MLP, **extra) -> dict:
    cfg = dict(peft_type="LORA", r=rank, lora_alpha=rank if alpha is None else alpha, target_modules=list(modules),
               bias="none", use_dora=False, use_rslora=False, modules_to_save=None)
    cfg.update(extra)
    return cfg


def random_adapter(cfg: dict, rank: int, seed: int, dtype=torch.float16, modules=ATTN + MLP, std=0.05) -> dict:
    g = torch.Generator().manual_seed(seed)
    shapes, sd = module_shapes(cfg), {}
    for layer in range(cfg["num_hidden_layers"]):
        for m in modules:
            n, k = shapes[m]
            sd[peft_key(layer, m, "A")] = (torch.randn(rank, k, generator=g) * std).to(dtype)
            sd[peft_key(layer, m, "B")] = (torch.randn(n, rank, generator=g) * std).to(dtype)
    return sd


def grid_adapter(cfg: dict, rank: int, seed: int, dtype=torch.float16, modules=ATTN + MLP, density=0.25) -> dict:
    """A and B in {0, +-1/8}, sparse: every entry of B.A is a multiple of 1/64 of magnitude <= rank / 64."""
    g = torch.Generator().manual_seed(seed)
    shapes, sd = module_shapes(cfg), {}

    def mat(*shape):
        sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
        keep = torch.rand(shape, generator=g) < density
        return (sign * keep / 8.0).to(dtype)
    for layer in range(cfg["num_hidden_layers"]):
        for m in modules:
            n, k = shapes[m]
            sd[peft_key(layer, m, "A")] = mat(rank, k)
            sd[peft_key(layer, m, "B")] = mat(n, rank)
    return sd


def snap_projections(sd: dict, dtype) -> dict:
    """The seven projection weights of every layer on the grid of multiples of 1/64 in [-3/64, 3/64]."""
    out = dict(sd)
    for key, w in sd.items():
        if key.endswith("_proj.weight"):
            out[key] = (torch.round(w.float() * 64).clamp(-3, 3) / 64).to(dtype)
    return out


def merge(sd: dict, adapter: dict, config: dict, cfg: dict, dtype) -> dict:
    """W + (alpha / r) B.A for every adapted projection; asserts that the merged weight is EXACTLY representable in
    `dtype` (then the oracle on the merged checkpoint is the exact target of the adapter path)."""
    scale = config["lora_alpha"] / config["r"]
    out = dict(sd)
    for layer in range(cfg["num_hidden_layers"]):
        for m in ATTN + MLP:
            a, b = adapter.get(peft_key(layer, m, "A")), adapter.get(peft_key(layer, m, "B"))
            if a is None:
                continue
            exact = sd[weight_key(layer, m)].double() + scale * (b.double() @ a.double())
            merged = exact.to(dtype)
            assert torch.equal(merged.double(), exact), f"layer {layer} {m}: W + B.A is not representable in {dtype}"
            out[weight_key(layer, m)] = merged
    return out


def write_peft_dir(path: str, adapter: dict, config: dict) -> str:
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "adapter_config.json"), "w", encoding="utf-8") as f:
        json.dump(config, f)
    save_file({k: v.contiguous() for k, v in adapter.items()}, os.path.join(path, "adapter_model.safetensors"))
    return path
