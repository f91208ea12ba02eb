"""References for the mixture-of-experts models (Qwen3-MoE, Mixtral).

`route_ref`, `up_gate_silu_ref`, `down_ref`, `combine_ref`: the contract of csrc/moe.hip restated in plain torch, fp64, each
from ITS OWN inputs, each returning next to its value the sum of the absolute products behind every element (the bounds of
tests/test_gpu_moe_kernels.py are relative to them).

`make_moe_checkpoint`: a seeded tiny HuggingFace model of one kind whose parameters are rounded to the tested 16-bit dtype
first, written by HF's own save_pretrained (per-expert tensor names, as the published checkpoints carry them), with the
tokenizer of oracle.synth; returns the fp32 eager model.

`forced_logits`: HF's eager forward with every router module hooked — the routing-forced reference. With `forced[layer]` =
expert ids [positions, k] the router returns those ids and the weights recomputed from ITS OWN logits over that set
(softmax over all experts in fp32, gathered, renormalised as the model's router does, cast as it casts); everything else is
what HF computes, in fp32 or in the tested 16-bit dtype. Without `forced` the hook only records. Either way it returns the
router logits and the free top-k choice of every layer. tests/test_moe_host.py ties it to unhooked HF."""
import copy
import os

import torch
import torch.nn.functional as F

from oracle import synth

D = torch.float64


# ---- the kernels, fp64 ---------------------------------------------------------------------------------------------------
def route_ref(logits: torch.Tensor, k: int, norm: bool):
    """logits [T, E] -> (ids int64 [T, k], w fp64 [T, k]): the k largest logits, ties to the lowest id, descending; softmax
    over all E, divided by the slots' sum when `norm`. A row that is not all finite: ids 0..k-1, weights 0."""
    x = logits.to(D)
    T, E = x.shape
    ids = torch.empty((T, k), dtype=torch.int64)
    w = torch.zeros((T, k), dtype=D)
    for t in range(T):
        row = x[t]
        if not bool(torch.isfinite(row).all()):
            ids[t] = torch.arange(k)
            continue
        order = sorted(range(E), key=lambda e: (-float(row[e]), e))[:k]
        p = torch.softmax(row, 0)
        ids[t] = torch.tensor(order)
        w[t] = p[order] / (p[order].sum() if norm else 1.0)
    return ids, w


def kth_gap(logits: torch.Tensor, k: int) -> torch.Tensor:
    """[T]: the k-th largest logit minus the (k + 1)-th (inf when k == E)."""
    s = logits.to(D).sort(dim=-1, descending=True).values
    if k >= s.shape[-1]:
        return torch.full(s.shape[:-1], float("inf"), dtype=D)
    return s[..., k - 1] - s[..., k]


def up_gate_silu_ref(x, expert_up_gate, ids):
    """x [T, H], expert_up_gate [E, 2 I, H] ([up ; gate]), ids [T, k] -> dict(up, gate, up_mag, gate_mag) fp64 [T k, I]:
    the two projections of every pair before any rounding, and the sums of their absolute products."""
    T, k = ids.shape
    inter = expert_up_gate.shape[1] // 2
    xd = x.to(D)
    out = {n: torch.empty((T * k, inter), dtype=D) for n in ("up", "gate", "up_mag", "gate_mag")}
    for t in range(T):
        for j in range(k):
            w = expert_up_gate[int(ids[t, j])].to("cpu", D)     # (one expert at a time: the stack may be large, on any device)
            full, mag = w @ xd[t], w.abs() @ xd[t].abs()
            p = t * k + j
            out["up"][p], out["gate"][p] = full[:inter], full[inter:]
            out["up_mag"][p], out["gate_mag"][p] = mag[:inter], mag[inter:]
    return out


def silu(g):
    return g / (1.0 + torch.exp(-g))


def down_ref(act, expert_down, ids):
    """act [T k, I] (the stored activations), expert_down [E, H, I] -> (y, y_mag) fp64 [T k, H]."""
    T, k = ids.shape
    ad = act.to(D)
    flat = ids.reshape(-1)
    y, mag = [], []
    for p in range(T * k):
        w = expert_down[int(flat[p])].to("cpu", D)
        y.append(w @ ad[p])
        mag.append(w.abs() @ ad[p].abs())
    return torch.stack(y), torch.stack(mag)


def combine_ref(y, w):
    """y [T k, H], w [T, k] -> (out, out_mag) fp64 [T, H]."""
    T, k = w.shape
    yd = y.to(D).view(T, k, -1)
    wd = w.to(D)[:, :, None]
    return (wd * yd).sum(1), (wd * yd).abs().sum(1)


def ulp_of(y: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of `dtype` at |y| (fp64), floored at the dtype's smallest normal exponent."""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(y.abs().clamp(min=2.0 ** (emin - mant)))).clamp(min=emin)
    return torch.exp2(e - mant)


# ---- tiny HuggingFace checkpoints ----------------------------------------------------------------------------------------
MOE_CONFIGS = {
    # both: 2 layers, vocab 512, 1024 positions, hidden 256, top-2
    "qwen3_moe": dict(num_attention_heads=4, num_key_value_heads=2, head_dim=128, num_experts=8, num_experts_per_tok=2,
                      moe_intermediate_size=128, intermediate_size=512, norm_topk_prob=True, mlp_only_layers=[],
                      decoder_sparse_step=1),
    "mixtral": dict(num_attention_heads=4, num_key_value_heads=2, head_dim=64, num_local_experts=4, num_experts_per_tok=2,
                    intermediate_size=256, sliding_window=None),
}


def hf_config(kind: str, **overrides):
    import transformers
    kw = dict(vocab_size=512, hidden_size=256, num_hidden_layers=2, max_position_embeddings=1024, rms_norm_eps=1e-6,
              tie_word_embeddings=False)
    kw.update(MOE_CONFIGS[kind], **overrides)
    cls = {"qwen3_moe": transformers.Qwen3MoeConfig, "mixtral": transformers.MixtralConfig}[kind]
    cfg = cls(**kw)
    cfg._attn_implementation = "eager"
    return cfg


def make_moe_checkpoint(path: str, kind: str, dtype: torch.dtype, seed: int, **overrides):
    """Write the directory; return the fp32 eager HF model holding the same (dtype-rounded) parameter values. Matrices
    (expert stacks and routers included) N(0, 0.02^2), norm weights 1 + N(0, 0.2^2) — as _families_ref.make_hf_checkpoint."""
    import transformers
    cfg = hf_config(kind, **overrides)
    model = transformers.AutoModelForCausalLM.from_config(cfg, dtype=torch.float32)
    model.eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for pname, p in sorted(model.named_parameters()):
            if "norm" in pname:
                t = 1.0 + torch.randn(p.shape, generator=g) * 0.2
            else:
                t = torch.randn(p.shape, generator=g) * 0.02
            p.copy_(t.to(dtype).float())
    copy.deepcopy(model).to(dtype).save_pretrained(path)
    synth.write_tokenizer(path, cfg.vocab_size)
    assert os.path.exists(os.path.join(path, "model.safetensors"))
    return model


def routers(model):
    """The router module of every layer, in layer order."""
    out = []
    for layer in model.model.layers:
        found = [m for m in layer.modules() if type(m).__name__.endswith("TopKRouter")]
        assert len(found) == 1, [type(m).__name__ for m in layer.modules()]
        out.append(found[0])
    return out


def experts_of(model):
    """(fused gate_up_proj [E, 2 I, H] as [gate ; up], down_proj [E, H, I]) of every layer."""
    out = []
    for layer in model.model.layers:
        found = [m for m in layer.modules() if type(m).__name__.endswith("Experts")]
        assert len(found) == 1
        out.append((found[0].gate_up_proj.detach(), found[0].down_proj.detach()))
    return out


class _Hooked:
    """Replaces a router's forward for the length of one model call."""

    def __init__(self, router, forced, qwen):
        self.router, self.forced, self.qwen = router, forced, qwen
        self.logits = self.free = None

    def __call__(self, hidden_states):
        r = self.router
        hidden_states = hidden_states.reshape(-1, r.hidden_dim)
        logits = F.linear(hidden_states, r.weight)
        probs = torch.softmax(logits, dim=-1, dtype=torch.float)
        free_val, free_idx = torch.topk(probs, r.top_k, dim=-1)
        self.logits, self.free = logits.detach().float(), free_idx.detach()
        if self.forced is None:
            val, idx = free_val, free_idx
        else:
            idx = self.forced.to(torch.int64)
            assert tuple(idx.shape) == tuple(free_idx.shape), (idx.shape, free_idx.shape)
            val = probs.gather(-1, idx)
        if not self.qwen or r.norm_topk_prob:
            val = val / val.sum(dim=-1, keepdim=True)
        if self.qwen:
            val = val.to(logits.dtype)
        return logits, val, idx


@torch.no_grad()
def forced_logits(model, token_rows, dtype: torch.dtype = torch.float32, forced=None):
    """Per token row: (logits [len, vocab] fp32, router logits [layers, len, E] fp32, free top-k ids [layers, len, k]) of
    the model cast to `dtype`, with `forced[row][layer]` = ids [len, k] imposed on the routers (None: free routing)."""
    m = model if dtype == torch.float32 else copy.deepcopy(model).to(dtype)
    qwen = m.config.model_type == "qwen3_moe"
    mods = routers(m)
    out = []
    for r, row in enumerate(token_rows):
        hooks = [_Hooked(mod, None if forced is None else torch.as_tensor(forced[r][layer]), qwen)
                 for layer, mod in enumerate(mods)]
        for mod, h in zip(mods, hooks):
            mod.forward = h
        try:
            lg = m(torch.tensor([row])).logits[0].float()
        finally:
            for mod in mods:
                del mod.forward
        out.append((lg, torch.stack([h.logits for h in hooks]), torch.stack([h.free for h in hooks])))
    return out
