"""References for the model families beyond Llama (Mistral, Qwen2 / Qwen2.5, dense Qwen3).

`qk_prep_ref`: the contract of swl_qk_prep_rotary (csrc/qk_prep.hip) restated in plain torch, fp64 — bias, per-head
RMSNorm, rotate-half rotary, and for every output element the two products of its rotation (the bound of
tests/test_gpu_qk_prep.py is relative to them). tests/test_qk_prep_host.py ties it to HuggingFace's Qwen3RMSNorm +
apply_rotary_pos_emb before any GPU is involved.

`make_hf_checkpoint`: a seeded tiny HuggingFace model of one family whose parameters are rounded to the tested 16-bit
dtype first (so both sides hold the same values), written by HF's own save_pretrained, with the tokenizer of
oracle.synth; returns the fp32 eager model — the independent reference of tests/test_gpu_model_families.py."""
import copy
import os

import torch

from oracle import synth


def _prep_heads(x, bias, w, eps, cos, sin):
    """x [T, N, D] fp64 -> (y, mag): y the rotated heads, mag = |a| + |b| of the two products behind each element."""
    T, N, D = x.shape
    f = x if bias is None else x + bias.view(1, N, D)
    if w is not None:
        r = 1.0 / torch.sqrt(f.pow(2).sum(-1, keepdim=True) / D + eps)
        f = f * r * w.view(1, 1, D)
    f0, f1 = f[..., :D // 2], f[..., D // 2:]
    c, s = cos[:, None, :], sin[:, None, :]
    a0, b0, a1, b1 = f0 * c, f1 * s, f1 * c, f0 * s
    return torch.cat((a0 - b0, a1 + b1), -1), torch.cat((a0.abs() + b0.abs(), a1.abs() + b1.abs()), -1)


def qk_prep_ref(q, k, v, cos_table, sin_table, pos_idx=None, q_bias=None, k_bias=None, v_bias=None, q_norm=None, k_norm=None,
                eps=0.0):
    """fp64 restatement of swl_qk_prep_rotary. q [T, H, D], k / v [T, KVH, D]; tables [rows, D/2]; pos_idx int [T] or None
    (row t); a negative row keeps the token's q, k and v. Returns dict(q, k, v, q_mag, k_mag, live): fp64 results (v is
    float(v) + float(bias), or v itself), the rotation's |a| + |b| per element, and the mask of rows that are not inert."""
    d = torch.float64
    T = q.shape[0]
    pos = torch.arange(T) if pos_idx is None else pos_idx.long().cpu()
    live = pos >= 0
    rows = pos.clamp(min=0)
    cos, sin = cos_table.to(d)[rows], sin_table.to(d)[rows]
    opt = lambda t: None if t is None else t.to(d)     # noqa: E731
    qy, qm = _prep_heads(q.to(d), opt(q_bias), opt(q_norm), eps, cos, sin)
    ky, km = _prep_heads(k.to(d), opt(k_bias), opt(k_norm), eps, cos, sin)
    vy = None
    if v is not None:
        vy = v.to(d) if v_bias is None else v.to(d) + v_bias.to(d).view(1, v.shape[1], v.shape[2])
        vy = torch.where(live[:, None, None], vy, v.to(d))
    m = live[:, None, None]
    return dict(q=torch.where(m, qy, q.to(d)), k=torch.where(m, ky, k.to(d)), v=vy, q_mag=qm, k_mag=km, live=live)


def ulp_of(y: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of `dtype` at |y| (fp64), floored at the dtype's smallest subnormal."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(y.abs().clamp(min=2.0 ** (emin - mant)))).clamp(min=emin)
    return torch.exp2(e - mant)


# ---- tiny HuggingFace checkpoints ---------------------------------------------------------------------------------------
FAMILY_CONFIGS = {
    # all: 2 layers, vocab 512, 1024 positions, hidden 256
    "qwen3_d128": dict(family="qwen3", num_attention_heads=4, num_key_value_heads=2, head_dim=128),     # q_size 512 != 256
    "qwen3_d64_tied": dict(family="qwen3", num_attention_heads=4, num_key_value_heads=2, head_dim=64, tie_word_embeddings=True),
    "qwen2": dict(family="qwen2", num_attention_heads=4, num_key_value_heads=2),
    "mistral": dict(family="mistral", num_attention_heads=4, num_key_value_heads=1, head_dim=128, sliding_window=None),
}


def hf_config(name: str, **overrides):
    import transformers
    kw = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, max_position_embeddings=1024,
              rms_norm_eps=1e-6, tie_word_embeddings=False)
    kw.update(FAMILY_CONFIGS[name], **overrides)
    cls = {"qwen3": transformers.Qwen3Config, "qwen2": transformers.Qwen2Config, "mistral": transformers.MistralConfig}[kw.pop("family")]
    cfg = cls(**kw)
    cfg._attn_implementation = "eager"
    return cfg


def make_hf_checkpoint(path: str, name: str, dtype: torch.dtype, seed: int, **overrides):
    """Write the directory; return the fp32 eager HF model holding the same (dtype-rounded) parameter values.
    Matrices N(0, 0.02^2), norm weights 1 + N(0, 0.2^2), biases N(0, 0.5^2)."""
    import transformers
    cfg = hf_config(name, **overrides)
    model = transformers.AutoModelForCausalLM.from_config(cfg, dtype=torch.float32)
    model.eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for pname, p in sorted(model.named_parameters()):
            if pname.endswith("bias"):
                t = torch.randn(p.shape, generator=g) * 0.5
            elif "norm" in pname:
                t = 1.0 + torch.randn(p.shape, generator=g) * 0.2
            else:
                t = torch.randn(p.shape, generator=g) * 0.02
            p.copy_(t.to(dtype).float())
    copy.deepcopy(model).to(dtype).save_pretrained(path)
    synth.write_tokenizer(path, cfg.vocab_size)
    assert os.path.exists(os.path.join(path, "model.safetensors"))
    return model


@torch.no_grad()
def hf_logits(model, token_rows, dtype: torch.dtype = torch.float32):
    """Eager logits [len, vocab] (as fp32) of each token row, from the model cast to `dtype`."""
    m = model if dtype == torch.float32 else copy.deepcopy(model).to(dtype)
    return [m(torch.tensor([row])).logits[0].float() for row in token_rows]
