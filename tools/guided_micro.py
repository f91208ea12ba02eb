"""Timing of the guided-decoding kernels (csrc/guided.hip) on the GPU. Nothing here is asserted anywhere.

    python tools/guided_micro.py [--iters 200] [--repeats 5] [--no-step] [--unguided-only] [--out FILE]

1. swl_logits_mask per call on [rows, 128256] bf16 logits, rows 1 / 32 / 256, every row guided by a mask row that allows
   about 1 token in 64 (the logits are restored between launches by a device copy that is timed on its own and taken off),
   next to swl_logits_adjust with min-p 0.05 on the same rows.
2. swl_guide_build_masks for S = 16 / 256 / 2048 states (a counter DFA over [a-z0-9 ]) on a synthetic 128256-token
   vocabulary: 256 single bytes, then tokens of 2..16 bytes over the same alphabet and some punctuation.
3. A Llama-3-8B-dims decode step (random-init bf16, 1024-token prompts, graph replay) at batch 8 and 32: host wall time per
   forward() — which ends in the tokens' device synchronise — with every row guided (the cursors are advanced by the
   loop, as the engine does) against no row guided, alternated twice; the first steps after a switch are left out.
   `--unguided-only` runs just the unguided half with nothing of the guided code imported, so the same file measures the
   parent commit's step.
Each kernel figure is the median of `--repeats` runs of `--iters` back-to-back launches between two device events, with
the range [min, max]. Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 128256


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


def _summary(runs, minus=0.0):
    runs = [r - minus for r in runs]
    return {"median_us": round(statistics.median(runs), 2), "min_us": round(min(runs), 2), "max_us": round(max(runs), 2)}


def synthetic_vocab(size=N, seed=0):
    from swiftllm_amd.guided import TokenVocab
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789 ,.-:\"{}", dtype=np.uint8)
    tokens = [bytes([b]) for b in range(256)]
    lens = rng.integers(2, 17, size - 256)
    for n in lens:
        tokens.append(alphabet[rng.integers(0, len(alphabet), n)].tobytes())
    tokens[-1] = tokens[-2] = None      # two specials
    return TokenVocab(tokens)


def mask_kernel_us(iters, repeats):
    from swiftllm_amd.worker.kernels.guided import GuideArgs, mask_logits
    from swiftllm_amd.worker.kernels.logits_process import RowEdits, adjust_logits
    import math
    out = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    words = (N + 31) // 32
    for rows in (1, 32, 256):
        src = (torch.randn(rows, N, device="cuda", generator=g) * 2.5).to(torch.bfloat16)
        x = src.clone()
        bits = torch.rand(8, words * 32, device="cuda", generator=g) < 1.0 / 64
        weights = (1 << torch.arange(32, device="cuda", dtype=torch.int64))
        masks = (bits.view(8, words, 32).to(torch.int64) * weights).sum(-1)
        masks = torch.where(masks >= 2 ** 31, masks - 2 ** 32, masks).to(torch.int32).contiguous()
        args = GuideArgs(masks, (torch.arange(rows, device="cuda") % 8).to(torch.int32))
        restore = _timed(lambda: x.copy_(src), iters, repeats)
        base = statistics.median(restore)

        def masked():
            x.copy_(src)
            mask_logits(x, args)
        out[f"r{rows}_mask"] = _summary(_timed(masked, iters, repeats), base)
        # (a second launch on already-masked rows: nothing changes, nothing is written back)
        out[f"r{rows}_mask_nothing_to_do"] = _summary(_timed(lambda: mask_logits(x, args), iters, repeats))
        empty_i, empty_f = np.zeros(0, np.int32), np.zeros(0, np.float32)
        from swiftllm_amd.worker.kernels import logits_process as lp
        host = np.empty(lp.buffer_len(rows, 1), dtype=np.int32)
        lp.pack_edits([RowEdits(empty_i, empty_i, empty_f, min_p_gap=math.log(0.05))] * rows, host, rows)
        aargs = lp.device_args(torch.from_numpy(host).cuda(), rows)

        def adjusted():
            x.copy_(src)
            adjust_logits(x, aargs)
        out[f"r{rows}_adjust_min_p"] = _summary(_timed(adjusted, iters, repeats), base)
        out[f"r{rows}_restore_copy"] = _summary(restore)
    return out


def build_kernel_us(iters, repeats):
    from swiftllm_amd.guided import compile_regex
    from swiftllm_amd.worker.kernels.guided import build_guide_masks, upload_vocab
    vocab = synthetic_vocab()
    dv = upload_vocab(vocab, N, torch.device("cuda"))
    ends = torch.tensor([N - 1, N - 2], dtype=torch.int32, device="cuda")
    out = {}
    for s, pattern in ((16, "[a-z0-9 ]{15}"), (256, "[a-z0-9 ]{255}"), (2048, "([a-z0-9 ]{89}){23}")):
        t = time.perf_counter()
        dfa = compile_regex(pattern)
        out[f"s{s}_compile_host_ms"] = round(1000 * (time.perf_counter() - t), 1)
        assert dfa.num_states == s, (s, dfa.num_states)
        pool = torch.zeros((s, (N + 31) // 32), dtype=torch.int32, device="cuda")
        trans = torch.from_numpy(dfa.trans).cuda()
        acc = torch.from_numpy(dfa.accepting.view(np.uint8)).cuda()
        out[f"s{s}_build"] = _summary(_timed(lambda: build_guide_masks(pool, 0, trans, acc, dv, ends),
                                             iters, repeats))
    return out


def build_model(cfg, batch, max_len, guided):
    """A random-init bf16 model of `cfg`'s dimensions with a KV pool for `batch` sequences of `max_len` tokens, graph
    replay on; `guided`: with a 64-row mask pool over the synthetic vocabulary (the parent commit has no such option, so
    the field is named only then)."""
    import tempfile
    from swiftllm_amd import EngineConfig, LlamaModel
    path = tempfile.mkdtemp(prefix="swl_guided_micro_")
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(cfg, f)
    extra = {"guided_max_states": 64} if guided else {}
    ec = EngineConfig(model_path=path, use_dummy=True, block_size=16, gpu_mem_utilization=0.97, num_cpu_blocks=0,
                      max_seqs_in_block_table=max(64, batch) + 64, max_blocks_per_seq=max_len // 16 + 8, max_batch_size=batch,
                      max_tokens_in_batch=batch * max_len, dtype="bfloat16", use_hip_graph=True, **extra)
    model = LlamaModel(ec)
    if guided:
        model.set_guide_vocab(synthetic_vocab(cfg["vocab_size"]))
    model.load_weights()
    # random-init weights as bench.py draws them: N(0, 0.02^2) matrices, norm weights 1 + N(0, 0.02^2)
    g = torch.Generator(device="cuda").manual_seed(1234)
    w = model.weight
    tensors = [w.wte, w.lm_head, w.final_norm]
    for layer in w.layers:
        tensors += [t for t in vars(layer).values() if isinstance(t, torch.Tensor)]
    with torch.inference_mode():
        for t in tensors:
            if t.dim() == 1:
                t.normal_(0.0, 0.02, generator=g).add_(1.0)
            else:
                t.normal_(0.0, 0.02, generator=g)
    model.repack_decode_weights()
    model.init_kvcache_and_swap(batch * (max_len // 16 + 2) + 64)
    return model


def decode_step_ms(batch, guided=True, steps=32, rounds=2):
    import bench
    S = 1024
    cfg = bench.model_config_dict("llama3-8b")
    max_len = S + 2 * rounds * (steps + 4) + 64
    model = build_model(cfg, batch, max_len, guided)
    if guided:
        from swiftllm_amd.guided import GuideCursor, guide_key
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg["vocab_size"], (S,), generator=g).tolist() for _ in range(batch)]
    seqs = list(range(batch))
    toks = model.forward(prompts, seqs, [])
    lens = [S] * batch
    res = {"unguided": []}
    modes = [("unguided", False)]
    cursors = None
    if guided:
        res["all_guided"] = []
        modes.append(("all_guided", True))
        guide = model.guide_store.acquire(guide_key("regex", "([a-z0-9 ]+[,.]?)+"))
        cursors = [GuideCursor(guide) for _ in range(batch)]
    for _ in range(rounds):
        for name, on in modes:
            for i in range(steps + 4):
                lens = [n + 1 for n in lens]
                t = time.perf_counter()
                if on:
                    toks = model.forward([[x] for x in toks], seqs, lens, guides=cursors)
                    for c, x in zip(cursors, toks):
                        c.advance(x)
                else:
                    toks = model.forward([[x] for x in toks], seqs, lens)
                if i >= 4:      # (the first steps after a switch capture / warm the other graph)
                    res[name].append(time.perf_counter() - t)
    model.free_seqs_resources(seqs)
    out = {}
    for k, v in res.items():
        out[f"b{batch}_step_{k}_ms"] = {"median": round(1000.0 * statistics.median(v), 3), "min": round(1000.0 * min(v), 3),
                                        "max": round(1000.0 * max(v), 3), "n": len(v)}
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--unguided-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    res = {}
    if not a.unguided_only and not a.no_kernels:
        res.update(mask_kernel_us(a.iters, a.repeats))
        res.update(build_kernel_us(a.iters, a.repeats))
    if not a.no_step:
        for batch in (8, 32):
            res.update(decode_step_ms(batch, guided=not a.unguided_only))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
