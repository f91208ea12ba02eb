"""Layer geometry of the checkpoints the README admits, as published in each one's config.json, and the (N, K) of the
projections a decode step streams. Data only: tests/test_family_shapes_host.py holds it to LlamaModelConfig, and
tests/test_gpu_family_shapes.py takes its GEMM shapes from it. Test helper: the product never imports it."""

#                     family     hidden  q heads  kv heads  head_dim  intermediate  vocabulary
GEOMETRIES = {
    "Llama-3-8B":        ("llama",   4096, 32, 8, 128, 14336, 128256),
    "Qwen3-0.6B":        ("qwen3",   1024, 16, 8, 128,  3072, 151936),
    "Qwen3-1.7B":        ("qwen3",   2048, 16, 8, 128,  6144, 151936),
    "Qwen3-4B":          ("qwen3",   2560, 32, 8, 128,  9728, 151936),
    "Qwen3-8B":          ("qwen3",   4096, 32, 8, 128, 12288, 151936),
    "Qwen3-32B":         ("qwen3",   5120, 64, 8, 128, 25600, 151936),
    "Qwen2.5-3B":        ("qwen2",   2048, 16, 2, 128, 11008, 151936),
    "Qwen2.5-72B":       ("qwen2",   8192, 64, 8, 128, 29568, 152064),
    "Mistral-7B":        ("mistral", 4096, 32, 8, 128, 14336,  32000),
    "Mistral-Nemo":      ("mistral", 5120, 32, 8, 128, 14336, 131072),
    "Mistral-Small-24B": ("mistral", 5120, 32, 8, 128, 32768, 131072),
}
FIELDS = ("family", "hidden", "q_heads", "kv_heads", "head_dim", "intermediate", "vocab")
PROJECTIONS = ("qkv", "o", "up_gate", "down", "lm_head")


def geometry(name: str) -> dict:
    return dict(zip(FIELDS, GEOMETRIES[name]))


def projection_shapes(name: str) -> dict:
    """(N, K) of every projection of the checkpoint: out features, in features."""
    g = geometry(name)
    q_size, kv_size = g["q_heads"] * g["head_dim"], g["kv_heads"] * g["head_dim"]
    return dict(qkv=(q_size + 2 * kv_size, g["hidden"]), o=(g["hidden"], q_size),
                up_gate=(2 * g["intermediate"], g["hidden"]), down=(g["hidden"], g["intermediate"]),
                lm_head=(g["vocab"], g["hidden"]))


def config_json(name: str) -> dict:
    """The fields of the checkpoint's config.json that LlamaModelConfig reads, in config.json's own names. (Llama and
    Qwen2 configs publish no head_dim: it is hidden / heads there.)"""
    g = geometry(name)
    cfg = dict(model_type=g["family"], hidden_act="silu", num_hidden_layers=2, hidden_size=g["hidden"],
               num_attention_heads=g["q_heads"], num_key_value_heads=g["kv_heads"], intermediate_size=g["intermediate"],
               vocab_size=g["vocab"], rms_norm_eps=1e-5 if g["family"] in ("llama", "mistral") else 1e-6,
               max_position_embeddings=4096, tie_word_embeddings=False)
    if g["family"] in ("qwen3", "mistral"):
        cfg["head_dim"] = g["head_dim"]
    return cfg
