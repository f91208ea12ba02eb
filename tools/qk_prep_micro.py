"""Timing of swl_qk_prep_rotary (csrc/qk_prep.hip) next to swl_rotary on the GPU. Nothing here is asserted anywhere.

    python tools/qk_prep_micro.py [--iters 200] [--repeats 5] [--no-step] [--no-kernels] [--out FILE]

1. The kernel in its QK-norm form (Qwen3) and its bias form (Qwen2: q, k AND v rows) and swl_rotary on the same q/k rows —
   column slices of one fused [tokens, (H + 2 KVH) D] bf16 buffer — at the Qwen3-8B (H 32, KVH 8, D 128) and Qwen2.5-3B
   (H 16, KVH 2, D 128) shapes, 1 / 32 / 256 / 4096 tokens. Every launch rotates in place what the last one left (the rows
   stay finite: the norm form renormalises, the others are rotations plus a small bias on rows that are re-drawn per case).
   At 4096 tokens all three are bandwidth-bound and `norm_over_rotary` is the figure DESIGN.md section 4.18 records.
2. A decode step at Qwen3-8B dimensions (dummy weights, bf16, 1024-token contexts, graph replay) at batch 8 and 32, host
   wall time per forward(), next to Llama-3-8B in the same run, with the launches per layer of each.
Each kernel figure is the median of `--repeats` runs of `--iters` back-to-back launches between two device events, with
the range [min, max]. Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"qwen3_8b": (32, 8, 128), "qwen25_3b": (16, 2, 128)}
QWEN3_8B = dict(model_type="qwen3", hidden_act="silu", num_hidden_layers=36, hidden_size=4096, num_attention_heads=32,
                num_key_value_heads=8, head_dim=128, intermediate_size=12288, vocab_size=151936, rope_theta=1000000,
                rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=False)


def _timed(fn, iters, repeats):
    for _ in range(10):
        fn()
    runs = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        runs.append(t0.elapsed_time(t1) * 1000.0 / iters)
    return runs


def _summary(runs):
    return {"median_us": round(statistics.median(runs), 2), "min_us": round(min(runs), 2), "max_us": round(max(runs), 2)}


def kernel_us(iters, repeats):
    from swiftllm_amd.worker.kernels.rotary_emb import qk_prep_rotary_inplace, rotary_embedding_inplace
    dt, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for name, (H, KVH, D) in SHAPES.items():
        inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, device=dev, dtype=torch.float32) / D))
        freqs = torch.outer(torch.arange(8192, device=dev, dtype=torch.float32), inv)
        cos, sin = torch.cos(freqs).to(dt).contiguous(), torch.sin(freqs).to(dt).contiguous()
        vec = lambda n, mean, std: (mean + std * torch.randn(n, device=dev, generator=g)).to(dt)     # noqa: E731
        qn, kn = vec(D, 1.0, 0.2), vec(D, 1.0, 0.2)
        # (a small bias: 200 x 5 launches add it again and again to rows that are only rotated in between)
        qb, kb, vb = vec(H * D, 0.0, 1e-3), vec(KVH * D, 0.0, 1e-3), vec(KVH * D, 0.0, 1e-3)
        for T in (1, 32, 256, 4096):
            pos = torch.randint(0, 8192, (T,), device=dev, generator=g, dtype=torch.int32)
            st = SimpleNamespace(position_cos=cos, position_sin=sin, position_indices=pos)

            def rows():
                buf = torch.randn(T, (H + 2 * KVH) * D, device=dev, generator=g).to(dt)
                return (buf[:, :H * D].view(T, H, D), buf[:, H * D:(H + KVH) * D].view(T, KVH, D),
                        buf[:, (H + KVH) * D:].view(T, KVH, D))
            q, k, v = rows()
            rot = _timed(lambda: rotary_embedding_inplace(q, k, st), iters, repeats)
            q, k, v = rows()
            norm = _timed(lambda: qk_prep_rotary_inplace(q, k, v, st, q_norm=qn, k_norm=kn, eps=1e-6), iters, repeats)
            q, k, v = rows()
            bias = _timed(lambda: qk_prep_rotary_inplace(q, k, v, st, q_bias=qb, k_bias=kb, v_bias=vb), iters, repeats)
            key = f"{name}_t{T}"
            out[key + "_rotary"], out[key + "_prep_norm"], out[key + "_prep_bias"] = _summary(rot), _summary(norm), _summary(bias)
            out[key + "_norm_over_rotary"] = round(statistics.median(norm) / statistics.median(rot), 3)
            out[key + "_bias_over_rotary"] = round(statistics.median(bias) / statistics.median(rot), 3)
    return out


def decode_step_ms(tag, cfg, batch, steps=32):
    """Host wall time per forward() of a pure-decode step on graph replay, and the kernel launches per layer of one eager
    step (counted at the C boundary)."""
    from swiftllm_amd import EngineConfig, LlamaModel, _hip
    S = 1024
    max_len = S + steps + 80
    path = tempfile.mkdtemp(prefix="swl_qk_prep_micro_")
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(cfg, f)
    ec = EngineConfig(model_path=path, use_dummy=True, block_size=16, gpu_mem_utilization=0.97, num_cpu_blocks=0,
                      max_seqs_in_block_table=batch + 64, max_blocks_per_seq=max_len // 16 + 8, max_batch_size=batch,
                      max_tokens_in_batch=batch * max_len, dtype="bfloat16", use_hip_graph=True)
    model = LlamaModel(ec)
    model.load_weights()
    model.init_kvcache_and_swap(batch * (max_len // 16 + 2) + 64)
    g = torch.Generator().manual_seed(1)
    seqs = list(range(batch))
    toks = model.forward([torch.randint(0, cfg["vocab_size"], (S,), generator=g).tolist() for _ in seqs], seqs, [])
    lens, times = [S] * batch, []
    for i in range(steps + 4):
        lens = [n + 1 for n in lens]
        t = time.perf_counter()
        toks = model.forward([[x] for x in toks], seqs, lens)
        if i >= 4:      # (the first steps capture and warm the graph)
            times.append(time.perf_counter() - t)
    # one eager step, its launches counted
    calls, inner = [], _hip.call
    _hip.call = lambda name, *a: (calls.append(name), inner(name, *a))[1]
    ec.use_hip_graph = False
    try:
        lens = [n + 1 for n in lens]
        model.forward([[x] for x in toks], seqs, lens)
    finally:
        _hip.call = inner
    layers = cfg["num_hidden_layers"]
    head = calls.index("swl_fused_add_rmsnorm") if "swl_fused_add_rmsnorm" in calls else 0
    per_layer = (len(calls) - head) // layers       # (hipBLASLt calls, if any, are not swl_ entries: decode takes none)
    model.free_seqs_resources(seqs)
    del model
    torch.cuda.empty_cache()
    return {f"{tag}_b{batch}_step_ms": {"median": round(1000.0 * statistics.median(times), 3),
                                        "min": round(1000.0 * min(times), 3), "max": round(1000.0 * max(times), 3),
                                        "n": len(times)},
            f"{tag}_b{batch}_swl_calls_per_layer": per_layer,
            f"{tag}_b{batch}_layer_calls": calls[head:head + per_layer]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    res = {}
    if not a.no_kernels:
        res.update(kernel_us(a.iters, a.repeats))
    if not a.no_step:
        import bench
        for batch in (8, 32):
            res.update(decode_step_ms("llama3_8b", bench.model_config_dict("llama3-8b"), batch))
            res.update(decode_step_ms("qwen3_8b", QWEN3_8B, batch))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
