"""Timing of prompt-lookup speculative decoding on the GPU: the verify attention kernel, the verify forward, the proposer.

    python tools/spec_decode_micro.py [--iters 20] [--rounds 5] [--dtype bfloat16] [--skip-model] [--out FILE]

Llama-3-8B heads and dims (32 q / 8 kv x 128; dummy weights), contexts 1 x 1.1k, 1 x 16k and 8 x 1.1k tokens. Variants
alternate inside one process after a warm-up; every figure is the median over `--rounds` of the mean of `--iters` calls.
1. kernel (us, device events): swl_paged_attn_verify at n = 1, 2, 4 new tokens per sequence against
   swl_paged_attn_decode on the same contexts (its n = 1 floor) and swl_prefill_attn_paged on the same rows;
2. model (ms, wall clock around calls that return their tokens): LlamaModel.forward_verify with k = 1 and 3 drafts at
   batch 1, 4 and 8 against the plain decode step (hipGraph replay) at the same contexts; the break-even acceptance
   is verify_ms / decode_ms - 1 accepted drafts per step;
3. proposer (us per append + propose on the host) at a 16k-token history.
Every part's result is printed (and --out rewritten) as soon as it exists; the last line on stdout is the whole JSON.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS = types.SimpleNamespace
H, KVH, D, L, LAYER = 32, 8, 128, 2, 1
CONTEXTS = {"1x1.1k": [1100], "1x16k": [16000], "8x1.1k": [1100 + 7 * i for i in range(8)]}
LLAMA3_8B = dict(model_type="llama", hidden_act="silu", rms_norm_eps=1e-5, rope_scaling=None, tie_word_embeddings=False,
                 num_hidden_layers=32, hidden_size=4096, num_attention_heads=32, num_key_value_heads=8,
                 intermediate_size=14336, vocab_size=128256, max_position_embeddings=32768, rope_theta=500000.0)   # (rotary rows for 16k)


def _events_us(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3


def _wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def _alternate(variants, timer, iters, rounds):
    """{name: fn} -> {name: median over rounds}; one warm-up pass, then the variants take turns in every round."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    got = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            got[name].append(timer(fn, iters))
    return {name: round(statistics.median(v), 3) for name, v in got.items()}


def kernel_part(a, dtype, emit):
    from swiftllm_amd.worker.batch_plan import select_seq_block_size
    from swiftllm_amd.worker.kernels.paged_attn import paged_attention, paged_attention_verify
    from swiftllm_amd.worker.kernels.prefill_attn import prefill_attention_paged
    dev = "cuda"
    mc, ec = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator().manual_seed(0)
    res = {}
    for label, ctxs in CONTEXTS.items():
        b = len(ctxs)
        blocks = [-(-(c + 4) // 16) for c in ctxs]
        nb = sum(blocks) + 1
        perm = torch.randperm(nb, generator=g)
        bt = torch.zeros((b, max(blocks)), dtype=torch.int32)
        off = 0
        for i, n in enumerate(blocks):
            bt[i, :n] = perm[off:off + n].to(torch.int32)
            off += n
        bt = bt.to(dev)
        kc = (torch.randn(nb, L, KVH, 16, D, device=dev) * 0.5).to(dtype)
        vc = torch.randn(nb, L, KVH, 16, D, device=dev).to(dtype)
        seq_ids = torch.arange(b, dtype=torch.int32, device=dev)
        variants = {}
        # the decode kernel on the same contexts: one new token per sequence, c + 1 keys
        lens = [c + 1 for c in ctxs]
        sbs = select_seq_block_size(lens, KVH, num_cus)
        qd = (torch.randn(b, H, D, device=dev) * 0.5).to(dtype)
        od = torch.empty_like(qd)
        std = NS(num_decoding_seqs=b, num_prefill_seqs=0, seq_block_size=sbs, num_seq_blocks=-(-max(lens) // sbs),
                 softmax_scale=D ** -0.5, decoding_seq_lens=torch.tensor(lens, dtype=torch.int32, device=dev),
                 seq_ids=seq_ids)
        variants["decode"] = lambda qd=qd, od=od, std=std: paged_attention(qd, kc, vc, bt, mc, ec, std, LAYER, od)
        for n in (1, 2, 4):
            total = [c + n for c in ctxs]
            sbs = select_seq_block_size(total, KVH, num_cus)
            cu = torch.arange(0, (b + 1) * n, n, dtype=torch.int32, device=dev)
            rows = torch.cat([c + 1 + torch.arange(n) for c in ctxs]).to(torch.int32).to(dev)
            q = (torch.randn(b * n, H, D, device=dev) * 0.5).to(dtype)
            o = torch.empty_like(q)
            st = NS(num_prefill_seqs=b, max_prefill_len=n, softmax_scale=D ** -0.5, prefill_seq_start_locs_with_end=cu,
                    num_prefill_tokens=b * n, prefill_ctx_lens=torch.tensor(ctxs, dtype=torch.int32, device=dev),
                    max_prefill_total_len=max(total), seq_ids=seq_ids, seq_block_size=sbs,
                    num_seq_blocks=-(-max(total) // sbs), verify_row_lens=rows, kv_scales=None)
            variants[f"verify_n{n}"] = lambda q=q, o=o, st=st: paged_attention_verify(q, kc, vc, bt, o, mc, ec, st, LAYER)
            variants[f"prefill_paged_n{n}"] = lambda q=q, o=o, st=st: prefill_attention_paged(q, kc, vc, bt, o, mc, ec, st,
                                                                                             LAYER)
        res[label] = _alternate(variants, _events_us, a.iters, a.rounds)
        emit("kernel_us", res)
        del kc, vc
    return res


def model_part(a, emit):
    from swiftllm_amd import EngineConfig, LlamaModel
    path = tempfile.mkdtemp(prefix="swl_spec_micro_")
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(LLAMA3_8B, f)
    ec = EngineConfig(model_path=path, use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=0,
                      max_seqs_in_block_table=16, max_blocks_per_seq=2048, max_batch_size=8, max_tokens_in_batch=16384,
                      dtype=a.dtype, use_hip_graph=True)
    model = LlamaModel(ec)
    model.load_weights()
    model.init_kvcache_and_swap(2048)
    g = torch.Generator().manual_seed(1)
    res = {"max_draft_tokens": model.max_draft_tokens}
    for label, ctxs in (("1x1.1k", CONTEXTS["1x1.1k"]), ("4x1.1k", CONTEXTS["8x1.1k"][:4]), ("8x1.1k", CONTEXTS["8x1.1k"]),
                        ("1x16k", CONTEXTS["1x16k"])):
        b = len(ctxs)
        ids = list(range(b))
        for sid, c in zip(ids, ctxs):       # the resident contexts, one prompt per forward
            model.forward([torch.randint(0, 1000, (c,), generator=g).tolist()], [sid], [])
        lens = [c + 1 for c in ctxs]
        variants = {"decode": lambda: model.forward([[5]] * b, ids, lens)}
        for k in (1, 3):
            if k <= model.max_draft_tokens:
                variants[f"verify_k{k}"] = lambda k=k: model.forward_verify([[5] * (k + 1)] * b, ids, list(ctxs))
        got = _alternate(variants, _wall_ms, a.iters, a.rounds)
        for k in (1, 3):
            if f"verify_k{k}" in got:
                got[f"break_even_k{k}"] = round(got[f"verify_k{k}"] / got["decode"] - 1.0, 3)
        res[label] = got
        emit("model_ms", res)
        model.free_seqs_resources(ids)
    return res


def proposer_part():
    from swiftllm_amd.server.speculative import NgramProposer
    import random
    rng = random.Random(0)
    hist = [rng.randrange(32000) for _ in range(16000)]
    for i in range(0, 16000 - 40, 400):     # copied spans, as prompt lookup meets them
        hist[i + 200:i + 240] = hist[i:i + 40]
    t0 = time.perf_counter()
    prop = NgramProposer(hist)
    build_us = (time.perf_counter() - t0) * 1e6
    calls, hits = 20000, 0
    t0 = time.perf_counter()
    for i in range(calls):
        prop.append(hist[(i * 7) % 16000])
        hits += bool(prop.propose(3))
    per_call = (time.perf_counter() - t0) * 1e6 / calls
    return {"history": 16000, "index_build_us_per_token": round(build_us / 16000, 3),
            "append_plus_propose_us": round(per_call, 3), "calls_with_a_draft": hits / calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="bfloat16", choices=["float16", "bfloat16"])
    ap.add_argument("--skip-model", action="store_true", help="kernel and proposer only (no 8B dummy model)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dtype = torch.float16 if a.dtype == "float16" else torch.bfloat16
    res = {"dtype": a.dtype, "iters": a.iters, "rounds": a.rounds}

    def emit(key, value):
        res[key] = value
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w", encoding="utf-8") as f:
                f.write(line + "\n")
    emit("proposer", proposer_part())
    kernel_part(a, dtype, emit)
    if not a.skip_model:
        model_part(a, emit)


if __name__ == "__main__":
    main()
