"""Timing of the paged prefill attention (csrc/prefill_attn_paged.hip) against the fresh-K/V kernel on the GPU.

    python tools/prefill_paged_micro.py [--iters 20] [--dtype bfloat16] [--kv-dtype auto|fp8_e4m3]

Llama-3-8B heads (32 q / 8 kv x 128), one layer of a 2-layer pool, block ids shuffled:
1. context 0, the same work on both kernels in one process: 32 x 1024 and 4 x 16 384 tokens — TF/s of
   swl_prefill_attn_varlen, of swl_prefill_attn_paged, and their ratio;
2. one 2 048-token chunk behind contexts 0, 2 048 .. 14 336: TF/s of the paged kernel, and the sum of the eight chunk
   times against one whole 16 384-token prefill on the fresh-K/V kernel.
Flop = 4 * D * H * (visible (row, key) pairs). Device events around `--iters` back-to-back launches. One JSON line.
--kv-dtype fp8_e4m3: the pools hold the same random values quantised to e4m3 at unit scales, so the paged figures are
those of the FP8 instantiation of the kernel (the fresh-K/V kernel has no FP8 form: its figures stay 16-bit).
"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS = types.SimpleNamespace
H, KVH, D, L, LAYER = 32, 8, 128, 2, 1


def _time_ms(fn, iters):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def _pairs(c, n):
    return n * c + n * (n + 1) // 2


def _setup(ctxs, lens, dtype, g, fp8=False):
    """q for the new tokens, pools holding ctx + len keys per sequence behind a shuffled block table."""
    dev = "cuda"
    blocks = [-(-(c + n) // 16) for c, n in zip(ctxs, lens)]
    nb = sum(blocks) + 1
    perm = torch.randperm(nb, generator=g)
    mbps = max(blocks)
    bt = torch.zeros((len(lens), mbps), dtype=torch.int32)
    off = 0
    for i, b in enumerate(blocks):
        bt[i, :b] = perm[off:off + b].to(torch.int32)
        off += b
    kc = torch.randn(nb, L, KVH, 16, D, device=dev) * 0.5
    vc = torch.randn(nb, L, KVH, 16, D, device=dev)
    if fp8:     # the storage contract of csrc/fp8_kv.h at scale 1
        kc, vc = (x.clamp(-448, 448).to(torch.float8_e4m3fn) for x in (kc, vc))
    else:
        kc, vc = kc.to(dtype), vc.to(dtype)
    q = (torch.randn(sum(lens), H, D, device=dev) * 0.5).to(dtype)
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0)
    st = NS(num_prefill_seqs=len(lens), max_prefill_len=max(lens), softmax_scale=D ** -0.5,
            prefill_seq_start_locs_with_end=cu.to(dev), num_prefill_tokens=sum(lens),
            prefill_ctx_lens=torch.tensor(ctxs, dtype=torch.int32, device=dev),
            max_prefill_total_len=max(c + n for c, n in zip(ctxs, lens)),
            seq_ids=torch.arange(len(lens), dtype=torch.int32, device=dev),
            kv_scales=torch.ones(2, L, KVH, dtype=torch.float32, device=dev) if fp8 else None)
    return q, kc, vc, bt.to(dev), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", default="bfloat16", choices=["float16", "bfloat16"])
    ap.add_argument("--kv-dtype", default="auto", choices=["auto", "fp8_e4m3"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from swiftllm_amd.worker.kernels.prefill_attn import prefill_attention, prefill_attention_paged
    dtype = torch.float16 if a.dtype == "float16" else torch.bfloat16
    g = torch.Generator().manual_seed(0)
    mc, ec = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16)
    fp8 = a.kv_dtype == "fp8_e4m3"
    res = {"dtype": a.dtype, "kv_dtype": a.kv_dtype}
    whole_ms = None
    for b, s in ((32, 1024), (4, 16384)):
        lens = [s] * b
        q, kc, vc, bt, st = _setup([0] * b, lens, dtype, g, fp8)
        o = torch.empty_like(q)
        k = (torch.randn(b * s, KVH, D, device="cuda") * 0.5).to(dtype)
        v = torch.randn(b * s, KVH, D, device="cuda").to(dtype)
        flop = 4.0 * D * H * b * _pairs(0, s)
        fresh = _time_ms(lambda: prefill_attention(q, k, v, o, mc, ec, st), a.iters)
        paged = _time_ms(lambda: prefill_attention_paged(q, kc, vc, bt, o, mc, ec, st, LAYER), a.iters)
        res[f"{b}x{s}_fresh_tflops"] = round(flop / fresh / 1e9, 1)
        res[f"{b}x{s}_paged_tflops"] = round(flop / paged / 1e9, 1)
        res[f"{b}x{s}_paged_over_fresh"] = round(fresh / paged, 3)
        res[f"{b}x{s}_fresh_ms"], res[f"{b}x{s}_paged_ms"] = round(fresh, 4), round(paged, 4)
        if (b, s) == (4, 16384):
            whole_ms = fresh / b
        del q, kc, vc, k, v, o
    total = 0.0
    for c in range(0, 16384, 2048):
        q, kc, vc, bt, st = _setup([c], [2048], dtype, g, fp8)
        o = torch.empty_like(q)
        ms = _time_ms(lambda: prefill_attention_paged(q, kc, vc, bt, o, mc, ec, st, LAYER), a.iters)
        total += ms
        res[f"chunk2048_ctx{c}_tflops"] = round(4.0 * D * H * _pairs(c, 2048) / ms / 1e9, 1)
        del q, kc, vc, o
    res["attn_16384_in_chunks_of_2048_ms"] = round(total, 3)
    res["attn_16384_whole_fresh_ms"] = round(whole_ms, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
