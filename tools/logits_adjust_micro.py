"""Timing of the logits adjustment (csrc/logits_adjust.hip) on the GPU.

    python tools/logits_adjust_micro.py [--iters 200] [--no-step] [--out FILE]

1. swl_logits_adjust per call on [rows, 128256] bf16 logits, rows 1 / 32 / 256, 0 / 64 / 4096 entries per row, min-p off
   and on — device events around `--iters` back-to-back launches. The logits are restored by a device copy before every
   launch of a min-p case (the phase works on what it left otherwise); that copy is timed alone and subtracted.
2. A Llama-3-8B-dims decode step (random-init bf16, 1024-token prompts, graph replay) at batch 1 and batch 32: host wall
   time per forward() with every row plain against every row processed (repetition 1.2, presence 0.2, frequency 0.1,
   min_p 0.05 at T = 0.8, a bias on four ids), alternated twice; the first steps after a switch are left out.
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
    from swiftllm_amd.worker.kernels.logits_process import AdjustArgs, adjust_logits
    out = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    for rows in (1, 32, 256):
        src = (torch.randn(rows, N, device="cuda", generator=g) * 2.5).to(torch.bfloat16)
        x = src.clone()
        copy_us = _timed(lambda: x.copy_(src), iters)
        out[f"r{rows}_restore_copy_us"] = round(copy_us, 2)
        for edits in (0, 64, 4096):
            ids = torch.stack([torch.randperm(N, device="cuda", generator=g)[:edits] for _ in range(rows)]).to(torch.int32)
            offsets = torch.arange(rows + 1, device="cuda", dtype=torch.int32) * edits
            meta = torch.randint(0, 4, (rows * edits,), device="cuda", generator=g, dtype=torch.int32)
            bias = torch.zeros(max(rows * edits, 1), device="cuda")
            for name, gap in (("minp_off", float("-inf")), ("minp_on", -3.0)):
                if edits == 0 and name == "minp_off":
                    params = torch.tensor([[1.0, 0.0, 0.0, gap]] * rows, device="cuda")     # inert rows: the early return
                else:
                    params = torch.tensor([[1.2, 0.2, 0.1, gap]] * rows, device="cuda")
                args = AdjustArgs(offsets, ids.reshape(-1) if edits else torch.zeros(1, dtype=torch.int32, device="cuda"),
                                  meta if edits else torch.zeros(1, dtype=torch.int32, device="cuda"), bias, params)
                if name == "minp_on":
                    us = _timed(lambda: adjust_logits(x.copy_(src), args), iters) - copy_us
                else:
                    us = _timed(lambda: adjust_logits(x, args), iters)
                out[f"r{rows}_e{edits}_{name}_us"] = round(us, 2)
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
    processed = [SamplingParams(0.8, seed=1000 + i, repetition_penalty=1.2, presence_penalty=0.2, frequency_penalty=0.1,
                                min_p=0.05, logit_bias={5: 1.0, 6: -1.0, 7: 2.0, 8: -2.0}) for i in range(batch)]
    # (the histories start at the prefill: the processed params go in there, the plain rounds pass none)
    toks = model.forward(prompts, seqs, [], sampling_params=processed)
    lens = [S] * batch
    res = {"plain": [], "processed": []}
    for _ in range(rounds):
        for name, sp in (("plain", None), ("processed", processed)):
            for i in range(steps + 4):
                lens = [n + 1 for n in lens]
                t = time.perf_counter()
                toks = model.forward([[x] for x in toks], seqs, lens, sampling_params=sp)
                if i >= 4:      # (the first steps after a switch capture / warm the other graph)
                    res[name].append(time.perf_counter() - t)
    entries = sum(h.size for h in model._histories.values())
    model.free_seqs_resources(seqs)
    out = {f"b{batch}_step_{k}_ms": round(1000.0 * sum(v) / len(v), 3) for k, v in res.items()}
    out[f"b{batch}_entries_per_step"] = entries
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
        for batch in (1, 32):
            res.update(decode_step_ms(batch))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
