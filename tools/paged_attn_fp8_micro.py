"""Decode attention over 16-bit and FP8 (e4m3fn) KV pools, back to back in one process on the same shuffled block tables.

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d OUT -- python tools/paged_attn_fp8_micro.py [--model]

The kernels are timed by the profiler (kernel-trace statistics of paged_attn_phase1_kernel / paged_attn_fp8_phase1_kernel
/ paged_attn_phase2_kernel), not by this script: it only launches them, `--iters` times per shape after `--warmup`, and
prints one JSON line per shape with the launch geometry and the algorithmic bytes
(sum len * 2 * KVH * D * e + q/o + partials, e = 2 or 1) so that TB/s = bytes / kernel time. The pools are sized past the
256 MiB of MALL so every launch streams from HBM. `--model`: also time `model.forward` decode steps (host wall clock over
hipGraph replays, 1024-token contexts) at batch 32 / 128 / 256 with a dummy Llama-3-8B-shaped model in both modes.
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftllm_amd.worker.batch_plan import select_seq_block_size  # noqa: E402
from swiftllm_amd.worker.kernels.paged_attn import paged_attention  # noqa: E402

NS = types.SimpleNamespace
SHAPES = [  # name, batch, context, H, KVH
    ("b32x1.1k_gqa", 32, 1100, 32, 8), ("b128x1.1k_gqa", 128, 1100, 32, 8), ("b256x1.1k_gqa", 256, 1100, 32, 8),
    ("b4x16k_mha", 4, 16384, 32, 32), ("b1x131k_gqa", 1, 131072, 32, 8),
]


def run_shape(name, batch, ctx, H, KVH, dtype, iters, warmup, D=128, L=1):
    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    per_seq = -(-ctx // 16)
    need = batch * per_seq
    nblk = max(need, (512 << 20) // (KVH * 16 * D * 2) + 1)          # >= 512 MiB per 16-bit pool: past the MALL
    perm = torch.randperm(nblk, generator=g)[:need].to(torch.int32).reshape(batch, per_seq)
    bt = perm.to(dev).contiguous()
    k16 = (torch.randn(nblk, L, KVH, 16, D, device=dev) * 0.5).to(dtype)
    v16 = torch.randn(nblk, L, KVH, 16, D, device=dev).to(dtype)
    k8 = k16.float().clamp(-448, 448).to(torch.float8_e4m3fn)
    v8 = v16.float().clamp(-448, 448).to(torch.float8_e4m3fn)
    q = (torch.randn(batch, H, D, device=dev) * 0.5).to(dtype)
    o = torch.empty_like(q)
    lens = [ctx] * batch
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    sbs = select_seq_block_size(lens, KVH, num_cus)
    nsb = -(-ctx // sbs)
    st = NS(num_decoding_seqs=batch, num_prefill_seqs=0, seq_block_size=sbs, num_seq_blocks=nsb, softmax_scale=D ** -0.5,
            decoding_seq_lens=torch.tensor(lens, dtype=torch.int32, device=dev),
            seq_ids=torch.arange(batch, dtype=torch.int32, device=dev),
            kv_scales=torch.ones(2, L, KVH, dtype=torch.float32, device=dev))
    mc, ec = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16)
    for it in range(warmup + iters):
        paged_attention(q, k16, v16, bt, mc, ec, st, 0, o)
        paged_attention(q, k8, v8, bt, mc, ec, st, 0, o)
    torch.cuda.synchronize()
    qo = 2 * batch * H * D * 2
    parts = 0 if nsb == 1 else 2 * batch * H * nsb * (D + 1) * 4
    kv = batch * ctx * 2 * KVH * D
    print(json.dumps(dict(shape=name, batch=batch, ctx=ctx, H=H, KVH=KVH, D=D, seq_block_size=sbs, num_seq_blocks=nsb,
                          launches_each=warmup + iters, bytes_16bit=kv * 2 + qo + parts, bytes_fp8=kv + qo + parts)),
          flush=True)


def run_model(dtype_name, iters, warmup):
    import tempfile
    import swiftllm_amd as swiftllm
    cfg = dict(model_type="llama", hidden_act="silu", num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8,
               hidden_size=4096, vocab_size=128256, max_position_embeddings=8192, intermediate_size=14336,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    with tempfile.TemporaryDirectory() as d:
        json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
        for kvd in ("auto", "fp8_e4m3"):
            ec = swiftllm.EngineConfig(model_path=d, use_dummy=True, block_size=16, gpu_mem_utilization=0.9,
                                       num_cpu_blocks=0, max_seqs_in_block_table=512, max_blocks_per_seq=128,
                                       max_batch_size=256, max_tokens_in_batch=8192, dtype=dtype_name, kv_cache_dtype=kvd)
            model = swiftllm.LlamaModel(ec)
            model.load_weights()
            model.init_kvcache_and_swap(256 * 72)
            for batch in (32, 128, 256):
                ids = list(range(batch))
                lens = [1024] * batch
                model.gpu_block_manager.allocate_blocks_for_seqs(ids, lens)
                times = []
                for it in range(warmup + iters):
                    lens = [n + 1 for n in lens]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model.forward([[1]] * batch, ids, lens)
                    times.append(time.perf_counter() - t0)
                model.free_seqs_resources(ids)
                t = sorted(times[warmup:])
                print(json.dumps(dict(model_step=True, kv_cache_dtype=kvd, batch=batch, ctx=1024, dtype=dtype_name,
                                      median_ms=1e3 * t[len(t) // 2], min_ms=1e3 * t[0], max_ms=1e3 * t[-1])), flush=True)
            del model
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtype", default="bfloat16", choices=["float16", "bfloat16"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    a = ap.parse_args()
    dtype = torch.float16 if a.dtype == "float16" else torch.bfloat16
    want = set(filter(None, a.shapes.split(",")))
    for name, batch, ctx, H, KVH in SHAPES:
        if not want or name in want:
            run_shape(name, batch, ctx, H, KVH, dtype, a.iters, a.warmup)
            torch.cuda.empty_cache()
    if a.model:
        run_model(a.dtype, a.iters, a.warmup)


if __name__ == "__main__":
    main()
