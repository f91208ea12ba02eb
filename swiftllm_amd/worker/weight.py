"""Weight containers and checkpoint readers for LLaMA.

Behaviour follows swiftllm/worker/weight.py:10-272: the same HuggingFace tensor names, the same
shape checks, safetensors (single file or `model.safetensors.index.json`) preferred over
`pytorch_model.bin` (single or indexed, mmap), dummy weights ~ U(-1e-3, 1e-3) for profiling runs,
`up_proj`/`gate_proj` concatenated into `up_gate_proj` = [up ; gate] (weight.py:133), and the
"rope_scaling is a dict => Llama-3.2 => lm_head tied to the embedding" sniff (weight.py:199-213).
Differences: dtype and device are parameters (the reference hard-codes fp16 / "cuda"), and q/k/v can
additionally be concatenated into one `qkv_proj` for a single fused projection GEMM. Beyond the reference: the Llama-shaped
families of model_config.py — q_proj / o_proj sized by num_q_heads * head_dim (Qwen3, Mistral-Nemo), Qwen3's per-head
q_norm / k_norm, Qwen2's q/k/v_proj biases, and a tied lm_head selected by `tie_word_embeddings`. A mixture-of-experts layer
(Qwen3-MoE, Mixtral) has a `router` [E, H] and two stacked expert tensors in place of up_gate_proj / down_proj:
`expert_up_gate` [E, 2 I, H] (each expert [up ; gate]) and `expert_down` [E, H, I] — one copy in HBM, never packed.
"""
import json
import os
from typing import Callable, Dict, List, NamedTuple, Tuple

import torch


class WeightSpec(NamedTuple):
    attr: str               # attribute the tensor is stored under
    key: str                # tensor name in the checkpoint
    shape: Tuple[int, ...]


def _q_size(cfg) -> int:
    """Width of q_proj's output: num_q_heads * head_dim, which Qwen3 and Mistral-Nemo decouple from hidden_size."""
    return cfg.num_q_heads * cfg.head_dim


def layer_weight_specs(cfg, layer_id: int) -> List[WeightSpec]:
    h, kv, qs = cfg.hidden_size, cfg.num_kv_heads * cfg.head_dim, _q_size(cfg)
    inter = cfg.ffn_inter_dim
    pre = f"model.layers.{layer_id}."
    if getattr(cfg, "num_experts", 0):
        ffn = [WeightSpec("router", pre + _moe_names(cfg)[0] + "gate.weight", (cfg.num_experts, h))]
    else:
        ffn = [WeightSpec("up_proj", pre + "mlp.up_proj.weight", (inter, h)),
               WeightSpec("gate_proj", pre + "mlp.gate_proj.weight", (inter, h)),
               WeightSpec("down_proj", pre + "mlp.down_proj.weight", (h, inter))]
    return [
        WeightSpec("attn_norm", pre + "input_layernorm.weight", (h,)),
        WeightSpec("q_proj", pre + "self_attn.q_proj.weight", (qs, h)),
        WeightSpec("k_proj", pre + "self_attn.k_proj.weight", (kv, h)),
        WeightSpec("v_proj", pre + "self_attn.v_proj.weight", (kv, h)),
        WeightSpec("o_proj", pre + "self_attn.o_proj.weight", (h, qs)),
        WeightSpec("ffn_norm", pre + "post_attention_layernorm.weight", (h,)),
    ] + ffn + layer_family_specs(cfg, layer_id)


def _moe_names(cfg):
    """(module prefix, up, gate, down) as the published checkpoints of the family name an expert's tensors."""
    if cfg.model_type == "mixtral":
        return "block_sparse_moe.", "w3", "w1", "w2"
    return "mlp.", "up_proj", "gate_proj", "down_proj"


def expert_weight_specs(cfg, layer_id: int) -> List[tuple]:
    """Per expert of a mixture-of-experts layer: (WeightSpec, stacked attribute, first row inside the stack). The stacks
    are expert_up_gate [E, 2 I, H] (rows e * 2 I: up, e * 2 I + I: gate) and expert_down [E, H, I] (rows e * H)."""
    h, inter = cfg.hidden_size, cfg.moe_inter_dim
    mod, up, gate, down = _moe_names(cfg)
    out = []
    for e in range(cfg.num_experts):
        pre = f"model.layers.{layer_id}.{mod}experts.{e}."
        out += [(WeightSpec("up_proj", pre + up + ".weight", (inter, h)), "expert_up_gate", e * 2 * inter),
                (WeightSpec("gate_proj", pre + gate + ".weight", (inter, h)), "expert_up_gate", e * 2 * inter + inter),
                (WeightSpec("down_proj", pre + down + ".weight", (h, inter)), "expert_down", e * h)]
    return out


def layer_family_specs(cfg, layer_id: int) -> List[WeightSpec]:
    """The per-layer tensors Llama does not have: Qwen3's per-head q/k RMSNorm weights, Qwen2's q/k/v_proj biases. They
    are vectors — not projection_tensors(), never packed."""
    kv, qs, d = cfg.num_kv_heads * cfg.head_dim, _q_size(cfg), cfg.head_dim
    pre = f"model.layers.{layer_id}.self_attn."
    out = []
    if getattr(cfg, "qk_norm", False):
        out += [WeightSpec("q_norm", pre + "q_norm.weight", (d,)), WeightSpec("k_norm", pre + "k_norm.weight", (d,))]
    if getattr(cfg, "qkv_bias", False):
        out += [WeightSpec("q_bias", pre + "q_proj.bias", (qs,)), WeightSpec("k_bias", pre + "k_proj.bias", (kv,)),
                WeightSpec("v_bias", pre + "v_proj.bias", (kv,))]
    return out


def global_weight_specs(cfg, model_version: str) -> List[WeightSpec]:
    v, h = cfg.vocab_size, cfg.hidden_size
    head_key = "model.embed_tokens.weight" if model_version == "llama3.2" else "lm_head.weight"
    return [
        WeightSpec("wte", "model.embed_tokens.weight", (v, h)),
        WeightSpec("lm_head", head_key, (v, h)),
        WeightSpec("final_norm", "model.norm.weight", (h,)),
    ]


Getter = Callable[[WeightSpec], torch.Tensor]


def _fill(obj, specs: List[WeightSpec], getter: Getter, dtype: torch.dtype, device: torch.device):
    for spec in specs:
        t = getter(spec)
        assert isinstance(t, torch.Tensor), f"Weight {spec.key} is not a tensor"
        assert tuple(t.shape) == tuple(spec.shape), \
            f"Shape of weight {spec.key} does not match: {tuple(t.shape)} vs {spec.shape}"
        setattr(obj, spec.attr, t.to(device=device, dtype=dtype).contiguous())


class LlamaTransformerLayerWeight:
    """Weights of one transformer block: attn_norm, q/k/v/o_proj, ffn_norm, up_gate_proj, down_proj
    (and qkv_proj = [q ; k ; v] when fused). Qwen3: q_norm, k_norm [head_dim]. Qwen2: q_bias, k_bias, v_bias — with the
    fused projection they are three slices of one qkv_bias = [q ; k ; v]."""

    def __init__(self, layer_id: int, model_config, dtype: torch.dtype):
        self.layer_id = layer_id
        self.model_config = model_config
        self.dtype = dtype
        self.qkv_proj = None
        self.q_norm = self.k_norm = None
        self.qkv_bias = self.q_bias = self.k_bias = self.v_bias = None
        # a mixture-of-experts layer: router [E, H], expert_up_gate [E, 2 I, H], expert_down [E, H, I]; such a layer has no
        # up_gate_proj / down_proj attribute
        # (up_gate_proj / down_proj are NOT pre-set here: a dense layer's attributes keep the order they always had, which
        # is the order callers walk vars(layer) in when they re-initialise the weights from one seeded generator)
        self.router = self.expert_up_gate = self.expert_down = None

    def alloc_experts(self, device: torch.device):
        cfg = self.model_config
        e, h, inter = cfg.num_experts, cfg.hidden_size, cfg.moe_inter_dim
        self.expert_up_gate = torch.empty((e, 2 * inter, h), dtype=self.dtype, device=device)
        self.expert_down = torch.empty((e, h, inter), dtype=self.dtype, device=device)

    def slice_qkv_bias(self):
        """q_bias / k_bias / v_bias as views of the assembled qkv_bias (what the kernel receives)."""
        cfg = self.model_config
        qs, kv = _q_size(cfg), cfg.num_kv_heads * cfg.head_dim
        self.q_bias, self.k_bias, self.v_bias = self.qkv_bias[:qs], self.qkv_bias[qs:qs + kv], self.qkv_bias[qs + kv:]

    def load(self, getter: Getter, device: torch.device, fuse_qkv: bool):
        _fill(self, layer_weight_specs(self.model_config, self.layer_id), getter, self.dtype, device)
        if getattr(self.model_config, "num_experts", 0):
            # every expert goes to its place inside the stacks: no second copy of the expert weights at any time
            self.alloc_experts(device)
            for spec, attr, row in expert_weight_specs(self.model_config, self.layer_id):
                t = getter(spec)
                assert isinstance(t, torch.Tensor), f"Weight {spec.key} is not a tensor"
                assert tuple(t.shape) == tuple(spec.shape), \
                    f"Shape of weight {spec.key} does not match: {tuple(t.shape)} vs {spec.shape}"
                stack = getattr(self, attr)
                stack.view(-1, stack.shape[-1])[row:row + spec.shape[0]].copy_(t)
        else:
            self.up_gate_proj = torch.cat((self.up_proj, self.gate_proj), dim=0).contiguous()
            del self.up_proj, self.gate_proj
        if fuse_qkv:
            self.qkv_proj = torch.cat((self.q_proj, self.k_proj, self.v_proj), dim=0).contiguous()
            del self.q_proj, self.k_proj, self.v_proj
            if self.q_bias is not None:
                self.qkv_bias = torch.cat((self.q_bias, self.k_bias, self.v_bias), dim=0).contiguous()
                self.slice_qkv_bias()


class LlamaWeight:
    """All weights of the model: wte, lm_head, final_norm and `layers`."""

    def __init__(self, model_config, dtype: torch.dtype, model_version: str = "llama"):
        self.model_config = model_config
        self.dtype = dtype
        self.model_version = model_version
        self.layers = [LlamaTransformerLayerWeight(i, model_config, dtype)
                       for i in range(model_config.num_layers)]

    def load(self, getter: Getter, device: torch.device, fuse_qkv: bool = False):
        _fill(self, global_weight_specs(self.model_config, self.model_version), getter, self.dtype,
              device)
        if self.model_version == "llama3.2":
            self.lm_head = self.wte     # tied: one copy in HBM
        for layer in self.layers:
            layer.load(getter, device, fuse_qkv)


    def projection_tensors(self) -> list:
        """Every weight matrix a decode step streams through a GEMM (lm_head + the per-layer projections that exist
        under the current fuse_qkv setting) — the tensors pack_decode_weights gives a second, MFMA-ordered copy."""
        out = [getattr(self, "lm_head", None)]
        for layer in self.layers:
            out += [getattr(layer, a, None) for a in ("qkv_proj", "q_proj", "k_proj", "v_proj", "o_proj",
                                                      "up_gate_proj", "down_proj")]
        return [t for t in out if t is not None]


# ---- checkpoint readers --------------------------------------------------------------------------
def _dummy_getter(dtype: torch.dtype, device: torch.device) -> Getter:
    def get(spec: WeightSpec) -> torch.Tensor:
        return torch.empty(spec.shape, dtype=dtype, device=device).uniform_(-0.001, 0.001)
    return get


def _safetensors_getter(model_path: str, files: List[str], device: torch.device) -> Getter:
    import safetensors
    index_path = os.path.join(model_path, "model.safetensors.index.json")
    if os.path.exists(index_path):
        with open(index_path, "r", encoding="utf-8") as f:
            where: Dict[str, str] = json.load(f)["weight_map"]
        locate = where.__getitem__
    else:
        assert len(files) == 1, \
            "model.safetensors.index.json not found, but there are multiple .safetensors files"
        locate = lambda key: files[0]   # noqa: E731
    dev = str(device)

    def get(spec: WeightSpec) -> torch.Tensor:
        # opening a safetensors file only parses its header: cheap enough to do per tensor
        with safetensors.safe_open(os.path.join(model_path, locate(spec.key)), framework="pt",
                                   device=dev) as f:
            return f.get_tensor(spec.key)
    return get


def _torch_bin_getter(model_path: str, device: torch.device) -> Getter:
    index_path = os.path.join(model_path, "pytorch_model.bin.index.json")
    if os.path.exists(index_path):
        with open(index_path, "r", encoding="utf-8") as f:
            where: Dict[str, str] = json.load(f)["weight_map"]
        locate = where.__getitem__
    else:
        locate = lambda key: "pytorch_model.bin"    # noqa: E731
    opened: Dict[str, dict] = {}    # unpickling is slow: each shard is opened once (mmap)

    def get(spec: WeightSpec) -> torch.Tensor:
        name = locate(spec.key)
        if name not in opened:
            opened[name] = torch.load(os.path.join(model_path, name), map_location="cpu", mmap=True,
                                      weights_only=True)
        return opened[name][spec.key]
    return get


# ---- streaming safetensors loader (§8f rank 4: 16 GB of weights -> HBM) -------------------------------------
# The per-tensor path above (what the reference does, weight.py:235-268) costs three passes per weight: file ->
# pageable host tensor, synchronous pageable H2D copy, then torch.cat of q/k/v and up/gate on the device (with
# 2x transient HBM). This one parses the safetensors headers itself, mmaps the files and moves raw bytes:
# reader threads fill a ring of pinned staging buffers (numpy memcpy releases the GIL), each chunk goes to its
# FINAL position inside the destination tensor — the fused [q;k;v] and [up;gate] matrices are assembled in
# place, no cat — with an async copy on a side stream. Falls back to the per-tensor path for anything unusual
# (dtype conversion needed, non-safetensors checkpoints).
_ST_DTYPES = {"F16": torch.float16, "BF16": torch.bfloat16, "F32": torch.float32}
_STAGE_BYTES = 64 << 20
_STAGE_BUFFERS = 8


def _read_safetensors_index(model_path: str, files: List[str]) -> Dict[str, tuple]:
    """tensor name -> (file path, dtype string, shape, absolute begin, absolute end)."""
    import struct
    table = {}
    for name in files:
        path = os.path.join(model_path, name)
        with open(path, "rb") as f:
            (hlen,) = struct.unpack("<Q", f.read(8))
            header = json.loads(f.read(hlen))
        base = 8 + hlen
        for key, meta in header.items():
            if key == "__metadata__":
                continue
            b, e = meta["data_offsets"]
            table[key] = (path, meta["dtype"], tuple(meta["shape"]), base + b, base + e)
    return table


def _stream_safetensors(weight: "LlamaWeight", model_path: str, files: List[str], device: torch.device,
                        fuse_qkv: bool) -> bool:
    """Fill `weight` from the safetensors files. Returns False (nothing touched) when the fast path does not
    apply; raises on malformed checkpoints exactly like the per-tensor path (shape / missing-key asserts)."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    cfg, dtype = weight.model_config, weight.dtype
    table = _read_safetensors_index(model_path, files)
    h, kv, inter, qs = cfg.hidden_size, cfg.num_kv_heads * cfg.head_dim, cfg.ffn_inter_dim, _q_size(cfg)

    # destination plan: (checkpoint key, expected shape, destination tensor, first destination row)
    plan = []
    def dest(shape):
        return torch.empty(shape, dtype=dtype, device=device)
    for spec in global_weight_specs(cfg, weight.model_version):
        if spec.attr == "lm_head" and weight.model_version == "llama3.2":
            continue        # tied to wte below
        t = dest(spec.shape)
        setattr(weight, spec.attr, t)
        plan.append((spec.key, spec.shape, t, 0))
    if weight.model_version == "llama3.2":
        weight.lm_head = weight.wte
    for layer in weight.layers:
        specs = {s.attr: s for s in layer_weight_specs(cfg, layer.layer_id)}
        moe = "router" in specs
        for attr in ("attn_norm", "o_proj", "ffn_norm", "router" if moe else "down_proj"):
            t = dest(specs[attr].shape)
            setattr(layer, attr, t)
            plan.append((specs[attr].key, specs[attr].shape, t, 0))
        if moe:                                             # every expert at its final offset inside the two stacks
            layer.alloc_experts(device)
            for spec, attr, row in expert_weight_specs(cfg, layer.layer_id):
                plan.append((spec.key, spec.shape, getattr(layer, attr), row))
        else:
            layer.up_gate_proj = dest((2 * inter, h))       # [up ; gate] (reference weight.py:133)
            plan.append((specs["up_proj"].key, specs["up_proj"].shape, layer.up_gate_proj, 0))
            plan.append((specs["gate_proj"].key, specs["gate_proj"].shape, layer.up_gate_proj, inter))
        if fuse_qkv:
            layer.qkv_proj = dest((qs + 2 * kv, h))         # [q ; k ; v]
            for attr, row in (("q_proj", 0), ("k_proj", qs), ("v_proj", qs + kv)):
                plan.append((specs[attr].key, specs[attr].shape, layer.qkv_proj, row))
        else:
            for attr in ("q_proj", "k_proj", "v_proj"):
                t = dest(specs[attr].shape)
                setattr(layer, attr, t)
                plan.append((specs[attr].key, specs[attr].shape, t, 0))
        for attr in ("q_norm", "k_norm"):                   # Qwen3
            if attr in specs:
                t = dest(specs[attr].shape)
                setattr(layer, attr, t)
                plan.append((specs[attr].key, specs[attr].shape, t, 0))
        if "q_bias" in specs:                               # Qwen2
            if fuse_qkv:
                layer.qkv_bias = dest((qs + 2 * kv,))       # [q ; k ; v], assembled in place like qkv_proj
                layer.slice_qkv_bias()
                for attr, row in (("q_bias", 0), ("k_bias", qs), ("v_bias", qs + kv)):
                    plan.append((specs[attr].key, specs[attr].shape, layer.qkv_bias, row))
            else:
                for attr in ("q_bias", "k_bias", "v_bias"):
                    t = dest(specs[attr].shape)
                    setattr(layer, attr, t)
                    plan.append((specs[attr].key, specs[attr].shape, t, 0))

    # validate before moving a byte
    esize = torch.empty((), dtype=dtype).element_size()
    for key, shape, _, _ in plan:
        assert key in table, f"Weight {key} not found in the checkpoint"
        _, st_dtype, st_shape, b, e = table[key]
        assert tuple(st_shape) == tuple(shape), f"Shape of weight {key} does not match: {tuple(st_shape)} vs {shape}"
        if _ST_DTYPES.get(st_dtype) != dtype or e - b != esize * int(np.prod(shape)):
            return False    # needs a dtype conversion: per-tensor path

    maps = {}
    def src_bytes(path):
        if path not in maps:
            maps[path] = np.memmap(path, dtype=np.uint8, mode="r")
        return maps[path]

    # work list of (source view, destination byte view) chunks of at most _STAGE_BYTES
    chunks = []
    for key, shape, t, row in plan:
        path, _, _, b, e = table[key]
        row_bytes = esize * (int(np.prod(shape[1:])) if len(shape) > 1 else 1)
        dst = t.view(torch.uint8).view(-1)
        off = row * row_bytes
        for c in range(0, e - b, _STAGE_BYTES):
            n = min(_STAGE_BYTES, e - b - c)
            chunks.append((path, b + c, n, dst, off + c))

    if device.type != "cuda":
        for path, b, n, dst, off in chunks:
            dst[off:off + n] = torch.from_numpy(np.array(src_bytes(path)[b:b + n], copy=True))
        return True

    stage = [torch.empty(_STAGE_BYTES, dtype=torch.uint8).pin_memory() for _ in range(_STAGE_BUFFERS)]
    stage_np = [b.numpy() for b in stage]
    free_at = [None] * _STAGE_BUFFERS                       # event after the last H2D out of each buffer
    copy_stream = torch.cuda.Stream(device=device)

    def fill(i, slot):
        path, b, n, _, _ = chunks[i]
        np.copyto(stage_np[slot][:n], src_bytes(path)[b:b + n])     # page-in + memcpy, GIL released
        return i, slot

    with ThreadPoolExecutor(max_workers=_STAGE_BUFFERS) as pool:
        pending = []
        nxt = 0
        def submit(slot):
            nonlocal nxt
            if nxt < len(chunks):
                if free_at[slot] is not None:
                    free_at[slot].synchronize()
                pending.append(pool.submit(fill, nxt, slot))
                nxt += 1
        for slot in range(_STAGE_BUFFERS):
            submit(slot)
        while pending:
            i, slot = pending.pop(0).result()
            _, _, n, dst, off = chunks[i]
            with torch.cuda.stream(copy_stream):
                dst[off:off + n].copy_(stage[slot][:n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            free_at[slot] = ev
            submit(slot)
    copy_stream.synchronize()
    return True


def pack_decode_weights(weight: "LlamaWeight") -> int:
    """Give every projection the decode GEMMs stream a second copy in MFMA-fragment order (kernels/linear.py:
    pack_weight) — the packed copy is what decode-sized calls read (6.0-6.3 instead of 5.3-5.8 TB/s), the row-major
    one stays for prefill (hipBLASLt). Costs one more copy of the projection weights in HBM (15 GB for Llama-3-8B of
    the 288 GB). Returns the bytes added. Call again after changing weights in place."""
    from .kernels.linear import pack_weight, packable
    added = 0
    for t in weight.projection_tensors():
        if packable(t):
            added += pack_weight(t).numel() * t.element_size()
    return added


def detect_model_version(model_path: str) -> str:
    """'llama3.2' (lm_head tied to the embedding) when config.json carries a dict-valued rope_scaling, else 'llama'. The
    other families (mistral, qwen2, qwen3) say it themselves: `tie_word_embeddings`."""
    cfg_path = os.path.join(model_path, "config.json")
    if os.path.exists(cfg_path):
        with open(cfg_path, "r", encoding="utf-8") as f:
            config = json.load(f)
        if config.get("model_type", "llama") != "llama":
            return "llama3.2" if config.get("tie_word_embeddings") else "llama"
        if isinstance(config.get("rope_scaling"), dict):
            return "llama3.2"
    return "llama"


def load_weights(model_config, dtype: torch.dtype, model_path: str, use_dummy: bool = False,
                 model_version: str = "auto", device="cuda", fuse_qkv: bool = False,
                 streaming: bool = True) -> LlamaWeight:
    """Read (or synthesise) every weight of the model onto `device` in `dtype`. `streaming=False` forces the
    reference's tensor-by-tensor safetensors path."""
    device = torch.device(device)
    if model_version == "auto":
        if getattr(model_config, "model_type", "llama") != "llama":
            model_version = "llama3.2" if model_config.tie_word_embeddings else "llama"
        else:
            model_version = detect_model_version(model_path)
    weight = LlamaWeight(model_config, dtype, model_version)
    if use_dummy:
        getter = _dummy_getter(dtype, device)
    else:
        st_files = sorted(n for n in os.listdir(model_path) if n.endswith(".safetensors"))
        if st_files and streaming:
            index_path = os.path.join(model_path, "model.safetensors.index.json")
            assert os.path.exists(index_path) or len(st_files) == 1, \
                "model.safetensors.index.json not found, but there are multiple .safetensors files"
            if _stream_safetensors(weight, model_path, st_files, device, fuse_qkv):
                return weight
            weight = LlamaWeight(model_config, dtype, model_version)     # start over on the per-tensor path
        getter = (_safetensors_getter(model_path, st_files, device) if st_files
                  else _torch_bin_getter(model_path, device))
    weight.load(getter, device, fuse_qkv)
    return weight
