"""LlamaModelConfig — architecture hyper-parameters read from a HuggingFace `config.json`.

Mirrors swiftllm/model_config.py:5-46 (attribute names, defaults, kv-slot size formula). Beyond the reference it also
reads the Llama-shaped families whose differences sit between the q/k/v projections and attention: Mistral (optional
`head_dim`, optional `sliding_window`), Qwen2 / Qwen2.5 (bias on q/k/v_proj) and dense Qwen3 (per-head RMSNorm on q and k,
`head_dim` given in the config), and the mixture-of-experts variants whose attention is one of those: Qwen3-MoE (dense
Qwen3's attention) and Mixtral (Mistral's), with the expert geometry in `num_experts`, `num_experts_per_tok`,
`moe_inter_dim` and `norm_topk_prob` (all zero / false for a dense model). What those checkpoints may ask for and this project does not build is refused here, with
the reason, before any memory is touched."""
import json
import os

import torch

MODEL_TYPES = ("llama", "mistral", "qwen2", "qwen3")
MOE_TYPES = ("mixtral", "qwen2_moe", "qwen3_moe")
# the mixture-of-experts variants that are built, and the dense family each takes its attention (and its parsing) from
MOE_FAMILY = {"qwen3_moe": "qwen3", "mixtral": "mistral"}
# what csrc/moe.hip takes: one wave routes a token (4 experts a lane), one lane holds a slot
MOE_MAX_EXPERTS = 256
MOE_MAX_TOP_K = 16
# the attention kernels' tiles: q heads per kv head, and head_dim
GROUP_SIZES = (1, 2, 4, 8)
HEAD_DIMS = (32, 64, 128)


class LlamaModelConfig:
    """LLaMA 1/2/3, Mistral, Qwen2 / Qwen2.5, dense Qwen3, Qwen3-MoE and Mixtral configuration. Attribute names follow the reference so
    layer/kernel code and user scripts that poke at `model.model_config` keep working."""

    def __init__(self, model_config: dict):
        model_type = model_config["model_type"]
        if model_type in MOE_TYPES and model_type not in MOE_FAMILY:
            raise ValueError(f"model_type {model_type!r} is a mixture-of-experts variant with a shared expert next to the "
                             "routed ones; the shared expert is not built (qwen3_moe and mixtral are)")
        if model_type not in MODEL_TYPES + tuple(MOE_FAMILY):
            raise AssertionError(f"unsupported model_type {model_type!r}")
        if model_config["hidden_act"] != "silu":
            raise AssertionError(f"unsupported hidden_act {model_config['hidden_act']!r}")
        self.model_type = model_type
        self.num_layers = model_config["num_hidden_layers"]
        self.num_q_heads = model_config["num_attention_heads"]
        self.num_kv_heads = model_config.get("num_key_value_heads", self.num_q_heads)
        self.hidden_size = model_config["hidden_size"]
        self.head_dim = self.hidden_size // self.num_q_heads
        self.vocab_size = model_config["vocab_size"]
        self.max_position_embeddings = model_config["max_position_embeddings"]
        self.ffn_inter_dim = model_config.get("intermediate_size", 0) if model_type in MOE_FAMILY else model_config["intermediate_size"]
        self.rope_theta = model_config.get("rope_theta", 10000)
        self.rotary_base = model_config.get("rope_theta", model_config.get("rotary_base", 10000))
        self.rms_norm_eps = model_config["rms_norm_eps"]
        scaling = model_config.get("rope_scaling", 1.0)
        self.rope_scaling = 1.0 if scaling is None else scaling
        # q/k/v_proj carry a bias; q and k get a per-head RMSNorm before rotary; lm_head is the embedding
        self.qkv_bias = self.qk_norm = self.tie_word_embeddings = False
        self.sliding_window = None      # the window that capped max_position_embeddings, when one applies
        # mixture-of-experts FFN: experts, experts per token, an expert's intermediate size, top-k weights renormalised
        self.num_experts = self.num_experts_per_tok = self.moe_inter_dim = 0
        self.norm_topk_prob = False
        if model_type != "llama":
            self._init_family(model_config)
        if model_type in MOE_FAMILY:
            self._init_moe(model_config)
        self.q_size = self.num_q_heads * self.head_dim

    @property
    def is_moe(self) -> bool:
        return self.num_experts > 0

    def _init_moe(self, c: dict):
        """Qwen3-MoE and Mixtral: the expert geometry, and the refusals."""
        kind = self.model_type
        qwen = kind == "qwen3_moe"
        # (transformers 5 names the count num_local_experts when it writes either family; the published Qwen3-MoE configs
        # say num_experts)
        experts = c.get("num_experts") or c.get("num_local_experts")
        top_k = c.get("num_experts_per_tok")
        inter = c.get("moe_intermediate_size" if qwen else "intermediate_size")
        if not experts or not top_k or not inter:
            raise ValueError(f"{kind}: a mixture-of-experts config without "
                             f"{'num_experts' if qwen else 'num_local_experts'} / num_experts_per_tok / "
                             f"{'moe_intermediate_size' if qwen else 'intermediate_size'}")
        self.num_experts, self.num_experts_per_tok, self.moe_inter_dim = int(experts), int(top_k), int(inter)
        self.norm_topk_prob = bool(c.get("norm_topk_prob", False)) if qwen else True
        self.ffn_inter_dim = self.moe_inter_dim         # (no dense FFN in these models: the width an expert has)
        if c.get("mlp_only_layers"):
            raise ValueError(f"{kind}: mlp_only_layers {c['mlp_only_layers']} mixes dense and sparse layers; every layer "
                             "must be a mixture-of-experts layer")
        if c.get("decoder_sparse_step", 1) != 1:
            raise ValueError(f"{kind}: decoder_sparse_step {c['decoder_sparse_step']} mixes dense and sparse layers; only "
                             "decoder_sparse_step 1 is built")
        if self.num_experts_per_tok > self.num_experts:
            raise ValueError(f"{kind}: num_experts_per_tok {self.num_experts_per_tok} exceeds the {self.num_experts} experts")
        if self.num_experts > MOE_MAX_EXPERTS or self.num_experts_per_tok > MOE_MAX_TOP_K:
            raise ValueError(f"{kind}: {self.num_experts} experts, top-{self.num_experts_per_tok}; the routing kernel is built "
                             f"for at most {MOE_MAX_EXPERTS} experts and top-{MOE_MAX_TOP_K}")
        if self.hidden_size % 64 or self.moe_inter_dim % 32 or self.hidden_size // 16 > 65535 or self.moe_inter_dim // 16 > 65535:
            raise ValueError(f"{kind}: hidden_size {self.hidden_size}, expert intermediate size {self.moe_inter_dim}; the expert "
                             "GEMMs are built for hidden_size % 64 == 0 and an intermediate size % 32 == 0 (16-column blocks "
                             "within a 65535-block grid)")

    def _init_family(self, c: dict):
        """Mistral, Qwen2 and Qwen3: the fields Llama's parsing above does not read, and the refusals."""
        kind = MOE_FAMILY.get(self.model_type, self.model_type)
        if c.get("head_dim") is not None:
            self.head_dim = int(c["head_dim"])
        self.qkv_bias = kind == "qwen2"
        self.qk_norm = kind == "qwen3"
        self.tie_word_embeddings = bool(c.get("tie_word_embeddings", False))
        # transformers 5 writes rope_theta (and the rope type) into rope_parameters
        rope = c.get("rope_parameters") or {}
        if "rope_theta" not in c and rope.get("rope_theta") is not None:
            self.rope_theta = self.rotary_base = rope["rope_theta"]
        for field in ("rope_scaling", "rope_parameters"):
            spec = c.get(field)
            if isinstance(spec, dict):
                rope_type = spec.get("rope_type", spec.get("type", "default"))
                if rope_type not in (None, "default"):
                    raise ValueError(f"{kind}: {field} asks for rope_type {rope_type!r}; only the default rotary embedding "
                                     "is built (no YaRN, linear, dynamic or long-rope scaling)")
        self.rope_scaling = 1.0
        if c.get("attention_bias") and kind != "qwen2":
            raise ValueError(f"{kind}: attention_bias is true, which puts a bias on o_proj as well; the o_proj bias is not built")
        if c.get("mlp_bias"):
            raise ValueError(f"{kind}: mlp_bias is true; biases on the MLP projections are not built")
        if self.num_kv_heads <= 0 or self.num_q_heads % self.num_kv_heads or self.num_q_heads // self.num_kv_heads not in GROUP_SIZES:
            raise ValueError(f"{kind}: {self.num_q_heads} query heads over {self.num_kv_heads} key/value heads is a ratio of "
                             f"{self.num_q_heads / max(self.num_kv_heads, 1):g}; the attention kernels are built for the "
                             f"ratios {GROUP_SIZES}")
        if self.head_dim not in HEAD_DIMS:
            raise ValueError(f"{kind}: head_dim {self.head_dim}; the attention kernels are built for head_dim in {HEAD_DIMS}")
        # Inside the window, windowed and full attention are the same function: serve the window and nothing beyond it
        # (the engine refuses requests that outgrow the rope table). No windowed attention kernel is built.
        window = c.get("sliding_window")
        if window is not None and (kind == "mistral" or c.get("use_sliding_window")) and window < self.max_position_embeddings:
            print(f"[ModelConfig] {kind}: sliding_window {window} < max_position_embeddings {self.max_position_embeddings}: "
                  f"serving contexts up to {window} tokens (no windowed attention beyond the window)", flush=True)
            self.max_position_embeddings = self.sliding_window = int(window)

    def get_kvslot_size(self, dtype: torch.dtype = torch.float16) -> int:
        """Bytes of KV cache one token occupies (K and V, all layers); `dtype` is the POOL's element type (1 byte for
        torch.float8_e4m3fn)."""
        return 2 * self.num_layers * self.num_kv_heads * self.head_dim * dtype.itemsize

    @staticmethod
    def load_from_model_path(model_path: str) -> "LlamaModelConfig":
        with open(os.path.join(model_path, "config.json"), "r", encoding="utf-8") as f:
            return LlamaModelConfig(json.load(f))
