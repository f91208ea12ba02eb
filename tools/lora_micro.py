"""Timing of multi-LoRA serving (csrc/lora.hip, the LoRA layer path) on the GPU.

    python tools/lora_micro.py [--iters 200] [--no-step] [--out FILE]

1. swl_lora_shrink and swl_lora_expand per call at the four projection groups of Llama-3-8B (fused qkv, o, [up ; gate],
   down), rank 16, bf16, for T = 1 / 8 / 32 / 256 / 4096 rows with 1 and with 4 distinct adapters (rows interleaved) —
   device events around `--iters` back-to-back launches.
2. A Llama-3-8B-dims decode step (random-init bf16, 1024-token prompts) at batch 8 and 32: host wall time per forward() of the
   base step (graph replay), the base step launched eagerly, and the LoRA step (eager, every row on one of 4 adapters).
3. A 4 x 1024 prefill without and with adapters (every row on one of 4 adapters).
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HQ, HKV, INTER, RANK, SLOTS = 4096, 4096, 1024, 14336, 16, 4
GROUPS = {"qkv": ((HQ, HKV, HKV), H), "o": ((H,), HQ), "up_gate": ((INTER, INTER), H), "down": ((H,), INTER)}


def _timed(fn, iters):
    for _ in range(10):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / iters


def kernel_us(iters):
    from swiftllm_amd.worker.kernels import lora as K
    out = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, (widths, k) in GROUPS.items():
        grp = K.LoraGroup([name] * len(widths), widths, k, SLOTS, RANK, torch.bfloat16, "cuda")
        grp.a_stack.normal_(0.0, 0.02, generator=g)
        grp.b_stack.normal_(0.0, 0.02, generator=g)
        grp.scale.fill_(2.0)
        for t in (1, 8, 32, 256, 4096):
            x = torch.randn(t, k, device="cuda", generator=g).to(torch.bfloat16)
            y = torch.randn(t, grp.n, device="cuda", generator=g).to(torch.bfloat16)
            for adapters in (1, 4):
                batch = K.LoraBatch([i % adapters for i in range(t)], SLOTS, "cuda")
                tt = K.lora_shrink(x, grp, batch)
                it = iters if t < 4096 else max(20, iters // 10)
                out[f"{name}_T{t}_a{adapters}_shrink_us"] = round(_timed(lambda: K.lora_shrink(x, grp, batch), it), 2)
                out[f"{name}_T{t}_a{adapters}_expand_us"] = round(_timed(lambda: K.lora_expand(y, tt, grp, batch), it), 2)
    return out


def _adapter(cfg, seed):
    """A rank-16 adapter on all seven projections of every layer, PEFT names (small values: the timing does not care)."""
    g = torch.Generator().manual_seed(seed)
    h, inter = cfg["hidden_size"], cfg["intermediate_size"]
    kv = cfg["num_key_value_heads"] * (h // cfg["num_attention_heads"])
    shapes = dict(q_proj=(h, h), k_proj=(kv, h), v_proj=(kv, h), o_proj=(h, h), up_proj=(inter, h), gate_proj=(inter, h),
                  down_proj=(h, inter))
    sd = {}
    for layer in range(cfg["num_hidden_layers"]):
        for m, (n, k) in shapes.items():
            block = "self_attn" if m in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp"
            pre = f"base_model.model.model.layers.{layer}.{block}.{m}."
            sd[pre + "lora_A.weight"] = (torch.randn(RANK, k, generator=g) * 0.01).to(torch.bfloat16)
            sd[pre + "lora_B.weight"] = (torch.randn(n, RANK, generator=g) * 0.01).to(torch.bfloat16)
    return sd


def _model(batch, max_len, max_tokens=0):
    import bench
    from swiftllm_amd.worker.lora import LoraStore
    saved, sys.argv = sys.argv, [sys.argv[0]]
    try:
        args = bench.parse_args()
    finally:
        sys.argv = saved
    cfg = bench.model_config_dict("llama3-8b")
    args.kv_blocks = batch * (max_len // 16 + 2) + 64        # (a pool of the run's size: the adapters are attached after it)
    model = bench.build_model(args, cfg, args.kv_blocks, batch, max_len, True, max_tokens=max_tokens)
    model.lora_store = LoraStore(model.model_config, SLOTS, RANK, model.dtype, model.device)
    config = dict(peft_type="LORA", r=RANK, lora_alpha=2 * RANK, target_modules=[], bias="none")
    for i in range(SLOTS):
        model.load_lora(f"a{i}", state_dict=_adapter(cfg, 100 + i), config=config)
    return model, cfg


def decode_step_ms(model, cfg, batch, steps=24):
    S = 1024
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg["vocab_size"], (S,), generator=g).tolist() for _ in range(batch)]
    seqs = list(range(batch))
    names = [f"a{i % SLOTS}" for i in range(batch)]
    toks = model.forward(prompts, seqs, [])
    lens = [S] * batch
    res = {}
    for name in ("base_graph", "base_eager", "lora"):
        # (the switch is read at every forward; a LoRA step is eager whatever it says: it runs with the switch off here)
        model.engine_config.use_hip_graph = name == "base_graph"
        kw = {"lora": names} if name == "lora" else {}
        for i in range(steps + 4):
            lens = [n + 1 for n in lens]
            t = time.perf_counter()
            toks = model.forward([[x] for x in toks], seqs, lens, **kw)
            if i >= 4:      # (the first steps after a switch capture / warm the other path)
                res.setdefault(name, []).append(time.perf_counter() - t)
    model.free_seqs_resources(seqs)
    out = {f"b{batch}_step_{k}_ms": round(1000.0 * sum(v) / len(v), 3) for k, v in res.items()}
    model.engine_config.use_hip_graph = True
    return out


def prefill_ms(model, cfg, rounds=3):
    B, S = 4, 1024
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, cfg["vocab_size"], (S,), generator=g).tolist() for _ in range(B)]
    seqs = list(range(B))
    names = [f"a{i % SLOTS}" for i in range(B)]
    res = {"base": [], "lora": []}
    for r in range(rounds + 1):
        for name in ("base", "lora"):
            kw = {"lora": names} if name == "lora" else {}
            torch.cuda.synchronize()
            t = time.perf_counter()
            model.forward(prompts, seqs, [], **kw)
            if r:           # (the first round warms both paths)
                res[name].append(time.perf_counter() - t)
            model.free_seqs_resources(seqs)
    return {f"prefill_4x1024_{k}_ms": round(1000.0 * sum(v) / len(v), 3) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    res = kernel_us(a.iters)
    if not a.no_step:
        steps = 24
        model, cfg = _model(32, 1024 + 4 * (steps + 4) + 64, 0)
        res["adapter_mib_4_slots"] = round(model.lora_store.nbytes() / 2 ** 20, 1)
        for batch in (8, 32):
            res.update(decode_step_ms(model, cfg, batch, steps))
        res.update(prefill_ms(model, cfg))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
