"""Timing of the per-token logprob kernel (csrc/logprobs.hip) on the GPU.

    python tools/logprobs_micro.py [--iters 200] [--no-step] [--out FILE]

1. swl_logprobs per call on [rows, 128256] bf16 logits, rows 1 / 8 / 32 / 256, every row asking with N = 0 / 5 / 20 (the
   chosen token is the row's argmax) — device events around `--iters` back-to-back launches after 10 warm-up launches —
   and, on the same rows, swl_sample with temperature 1 and top-k 50: a kernel of the same structure (one 1024-thread
   workgroup per row, the row held in registers, a 16-round bisection).
2. A Llama-3-8B-dims decode step (random-init bf16, 1024-token prompts, graph replay) at batch 8 and batch 32: host wall
   time per forward() — which ends in the tokens' device synchronise — with no row asking against every row asking for
   N = 5, alternated twice; the first steps after a switch (capture, warm-up) are left out.
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

N = 128256


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
    from swiftllm_amd import SamplingParams
    from swiftllm_amd.worker.kernels.logprobs import token_logprobs
    from swiftllm_amd.worker.kernels.sampling import device_args, pack_params, sample_rows
    import numpy as np
    out = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    for rows in (1, 8, 32, 256):
        x = (torch.randn(rows, N, device="cuda", generator=g) * 2.5).to(torch.bfloat16)
        tokens = x.float().argmax(1)
        for top in (0, 5, 20):
            args = token_logprobs(x, tokens, [top] * rows)
            out[f"r{rows}_n{top}_us"] = round(_timed(lambda: token_logprobs(x, tokens, args), iters), 2)
        host = pack_params([SamplingParams(1.0, top_k=50, seed=7 + r) for r in range(rows)], np.empty(5 * rows, np.int32))
        sargs = device_args(torch.from_numpy(host).cuda(), torch.full((rows,), 100, dtype=torch.int32, device="cuda"))
        drawn = torch.empty(rows, dtype=torch.int64, device="cuda")
        out[f"r{rows}_sample_topk50_us"] = round(_timed(lambda: sample_rows(x, sargs, None, drawn), iters), 2)
    return out


def decode_step_ms(batch, steps=32, rounds=2):
    import bench
    from swiftllm_amd import SamplingParams
    saved, sys.argv = sys.argv, [sys.argv[0]]
    try:
        args = bench.parse_args()
    finally:
        sys.argv = saved
    S = 1024
    cfg = bench.model_config_dict("llama3-8b")
    max_len = S + 2 * rounds * (steps + 4) + 64
    model = bench.build_model(args, cfg, batch * (max_len // 16 + 2) + 64, batch, max_len, True)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg["vocab_size"], (S,), generator=g).tolist() for _ in range(batch)]
    seqs = list(range(batch))
    asking = [SamplingParams(logprobs=5)] * batch
    toks = model.forward(prompts, seqs, [])
    lens = [S] * batch
    res = {"none_asking": [], "all_asking": []}
    for _ in range(rounds):
        for name, sp in (("none_asking", None), ("all_asking", asking)):
            for i in range(steps + 4):
                lens = [n + 1 for n in lens]
                t = time.perf_counter()
                toks = model.forward([[x] for x in toks], seqs, lens, sampling_params=sp)
                if i >= 4:      # (the first steps after a switch capture / warm the other graph)
                    res[name].append(time.perf_counter() - t)
                assert (model.last_logprobs is None) == (sp is None)
    model.free_seqs_resources(seqs)
    out = {f"b{batch}_step_{k}_ms": round(1000.0 * sum(v) / len(v), 3) for k, v in res.items()}
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    res = kernel_us(a.iters)
    if not a.no_step:
        for batch in (8, 32):
            res.update(decode_step_ms(batch))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
