"""Timing of the seeded sampler (csrc/sampling.hip) on the GPU.

    python tools/sample_micro.py [--iters 200] [--no-step]

1. swl_sample per call at batch 1 / 32 / 256 x 128256 bf16 logits — greedy rows (and swl_argmax for comparison),
   temperature only, top-k 50 + top-p 0.95 — from device events around `--iters` back-to-back launches.
2. A BASELINE configs[2]-shaped decode step (Llama-3-8B random-init bf16, batch 32, 1024-token prompts, graph replay):
   host wall time per forward() (which ends in the tokens' device-to-host copy) with every row at T = 0.8, top_p = 0.95
   against greedy, alternated twice.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_us(iters):
    from swiftllm_amd.worker.kernels.sampling import SampleArgs, argmax_rows, sample_rows
    out = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    for b in (1, 32, 256):
        x = (torch.randn(b, 128256, device="cuda", generator=g) * 2.5).to(torch.bfloat16)
        dev = x.device
        seeds = torch.stack((torch.arange(b, dtype=torch.int32), torch.zeros(b, dtype=torch.int32)), 1).to(dev)
        pos = torch.full((b,), 1100, dtype=torch.int32, device=dev)

        def args(t, k, p):
            return SampleArgs(torch.full((b,), t, device=dev), torch.full((b,), k, dtype=torch.int32, device=dev),
                              torch.full((b,), p, device=dev), seeds, pos)
        cases = {"argmax": lambda: argmax_rows(x)}
        for name, a in (("greedy", args(0.0, 0, 1.0)), ("temperature", args(0.8, 0, 1.0)),
                        ("top_k_top_p", args(0.8, 50, 0.95)), ("top_p", args(0.8, 0, 0.95))):
            cases[name] = (lambda a=a: sample_rows(x, a, None))
        for name, fn in cases.items():
            for _ in range(10):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            out[f"b{b}_{name}_us"] = round(t0.elapsed_time(t1) * 1000.0 / iters, 2)
    return out


def decode_step_ms(steps=32, rounds=2):
    import bench
    from swiftllm_amd import SamplingParams
    saved, sys.argv = sys.argv, [sys.argv[0]]
    try:
        args = bench.parse_args()
    finally:
        sys.argv = saved
    B, S = 32, 1024
    cfg = bench.model_config_dict("llama3-8b")
    max_len = S + 2 * rounds * steps + 64
    model = bench.build_model(args, cfg, B * (max_len // 16 + 2) + 64, B, max_len, True)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg["vocab_size"], (S,), generator=g).tolist() for _ in range(B)]
    seqs = list(range(B))
    toks = model.forward(prompts, seqs, [])
    lens = [S] * B
    sampled = [SamplingParams(0.8, top_p=0.95, seed=1000 + i) for i in range(B)]
    res = {"greedy": [], "sampled": []}
    for _ in range(rounds):
        for name, sp in (("greedy", None), ("sampled", sampled)):
            for i in range(steps + 4):
                lens = [n + 1 for n in lens]
                t = time.perf_counter()
                toks = model.forward([[x] for x in toks], seqs, lens, sampling_params=sp)
                if i >= 4:      # (the first steps after a switch capture / warm the other graph)
                    res[name].append(time.perf_counter() - t)
    model.free_seqs_resources(seqs)
    return {f"step_{k}_ms": round(1000.0 * sum(v) / len(v), 3) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    res = kernel_us(a.iters)
    if not a.no_step:
        res.update(decode_step_ms())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
