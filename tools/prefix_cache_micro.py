#!/usr/bin/env python3
"""prefix_cache_micro.py — what prefix caching by KV block copy costs and saves on the MI355X.

(a) --part copy: swl_kv_copy_blocks (ONE launch, device-resident ids) against the same pairs done the way
    csrc/swap_blocks.hip moves blocks — consecutive pairs run-length coalesced, one hipMemcpyAsync device-to-device per run
    and pool — for 64 contiguous and 64 scattered blocks of 1 MiB in two pools of --pool-blocks blocks each. Every timed
    iteration takes another set of pairs (24 sets, 6 GiB touched: nothing is served from a cache), the two methods
    alternate window by window, and each figure is the median (min .. max) over --repeats windows of --iters copies:
    GB/s of read + write by device events, and host microseconds spent ISSUING one copy (no synchronise inside).
(b) --part step: Llama-3-8B dims, dummy weights, one model, two engines (cache on / off): the step that admits 4 prompts
    of 1024 tokens sharing their first 1008 (on: one copy of 4 x 63 blocks + a forward of 4 x 16 tokens behind a context
    of 1008; off: a forward of 4 x 1024 tokens), and the decode step that follows — whose forward() call is compared
    argument for argument between the two engines.
One JSON line per result.
"""
import argparse
import asyncio
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIB = 1 << 20
SETS = 24


def spread(xs, nd=1):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


# ---- (a) the copy ----------------------------------------------------------------------------------------------------
def runs_of(src, dst):
    """[(src id, dst id, blocks)] — swap_blocks.hip's run-length coalescing."""
    out, i = [], 0
    while i < len(src):
        j = i + 1
        while j < len(src) and src[j] == src[j - 1] + 1 and dst[j] == dst[j - 1] + 1:
            j += 1
        out.append((src[i], dst[i], j - i))
        i = j
    return out


def part_copy(a):
    from swiftllm_amd import _hip
    from swiftllm_amd.worker.kernels.kv_copy import kv_copy_blocks
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    D2D = 3
    nb, n = a.pool_blocks, 64
    assert nb * MIB * 2 >= 8 << 30 and nb >= 2 * n * SETS
    g = torch.Generator(device="cuda").manual_seed(1)
    pools = [torch.empty((nb, MIB), dtype=torch.uint8, device="cuda") for _ in range(2)]
    for p in pools:
        for b0 in range(0, nb, 1024):
            p[b0:b0 + 1024] = torch.randint(0, 256, (min(1024, nb - b0), MIB), dtype=torch.uint8, device="cuda", generator=g)
    k, v = pools
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(2)).tolist()
    sets = {"contiguous": [(list(range(2 * n * s, 2 * n * s + n)), list(range(2 * n * s + n, 2 * n * s + 2 * n)))
                           for s in range(SETS)],
            "scattered": [(perm[2 * n * s:2 * n * s + n], perm[2 * n * s + n:2 * n * s + 2 * n]) for s in range(SETS)]}
    stream = _hip.stream()
    kp, vp = k.data_ptr(), v.data_ptr()
    nbytes = 2 * 2 * n * MIB        # read + write, two pools

    for shape, pairs in sets.items():
        dev = [(torch.tensor(s, dtype=torch.int32, device="cuda"), torch.tensor(d, dtype=torch.int32, device="cuda"))
               for s, d in pairs]
        runs = [runs_of(s, d) for s, d in pairs]

        def by_kernel(i):
            kv_copy_blocks(k, v, *dev[i % SETS])

        def by_memcpy(i):
            for s, d, m in runs[i % SETS]:
                for base in (kp, vp):
                    rc = hip.hipMemcpyAsync(base + d * MIB, base + s * MIB, m * MIB, D2D, stream)
                    assert rc == 0, rc

        # the two methods do the same thing
        s0, d0 = pairs[0]
        want = k[s0].clone()
        by_kernel(0)
        torch.cuda.synchronize()
        assert torch.equal(k[d0], want)
        k[d0] = 0
        by_memcpy(0)
        torch.cuda.synchronize()
        assert torch.equal(k[d0], want)

        methods = {"kernel": by_kernel, "memcpy_runs": by_memcpy}
        gbps = {m: [] for m in methods}
        issue_us = {m: [] for m in methods}
        for m, fn in methods.items():       # warm-up
            for i in range(SETS):
                fn(i)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for m, fn in methods.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                for i in range(a.iters):
                    fn(i)
                t1 = time.perf_counter()
                e1.record()
                torch.cuda.synchronize()
                gbps[m].append(nbytes * a.iters / (e0.elapsed_time(e1) * 1e-3) / 1e9)
                issue_us[m].append((t1 - t0) / a.iters * 1e6)
        for m in methods:
            print(json.dumps({"part": "copy", "blocks": n, "block_MiB": 1, "pool_GiB": round(2 * nb * MIB / 2**30, 1),
                              "pairs": shape, "method": m, "runtime_calls_per_copy": 1 if m == "kernel" else 2 * len(runs[0]),
                              "MiB_read_plus_written": nbytes // MIB, "GBps": spread(gbps[m]),
                              "us_per_copy_device": spread([nbytes / (x * 1e9) * 1e6 for x in gbps[m]]),
                              "host_issue_us_per_copy": spread(issue_us[m]), "windows": a.repeats, "iters": a.iters}),
                  flush=True)


# ---- (b) the step ----------------------------------------------------------------------------------------------------
def part_step(a):
    import bench
    from swiftllm_amd import Engine, EngineConfig, LlamaModel
    from swiftllm_amd.server import RawRequest, Request
    cfg = bench.model_config_dict("llama3-8b")
    path = tempfile.mkdtemp(prefix="swl_prefix_")
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(cfg, f)
    kw = dict(model_path=path, use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=0,
              max_seqs_in_block_table=64, max_blocks_per_seq=128, max_batch_size=8, max_tokens_in_batch=8192,
              dtype="bfloat16", max_prefill_chunk=8192)
    model = LlamaModel(EngineConfig(**kw))
    model.load_weights()
    g = torch.Generator(device="cuda").manual_seed(1234)
    tensors = [model.weight.wte, model.weight.lm_head, model.weight.final_norm]
    for layer in model.weight.layers:
        tensors += [t for t in vars(layer).values() if isinstance(t, torch.Tensor)]
    with torch.inference_mode():            # bench.py's random init: realistic value ranges
        for t in tensors:
            t.normal_(0.0, 0.02, generator=g)
            if t.dim() == 1:
                t.add_(1.0)
    model.repack_decode_weights()
    model.init_kvcache_and_swap(1024)
    vocab = cfg["vocab_size"]
    rng = torch.Generator().manual_seed(7)

    def ids(n):
        return torch.randint(0, vocab, (n,), generator=rng).tolist()
    shared = ids(1008)
    calls = []
    inner = model.forward

    def spy(input_ids, seq_ids, dec_lens, **kwargs):
        calls.append(([len(x) for x in input_ids], list(dec_lens), sorted(kwargs)))
        return inner(input_ids, seq_ids, dec_lens, **kwargs)
    model.forward = spy

    async def serve(eng, prompts, out_len, timed):
        reqs = [Request(RawRequest("", out_len, list(p))) for p in prompts]
        eng.scheduler.on_requests_arrival(reqs)
        times = []
        while not all(r.is_finished() for r in reqs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert await eng.step()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return times if timed else None

    async def run():
        engines = {}
        for mode in ("off", "on"):
            eng = Engine(EngineConfig(enable_prefix_caching=(mode == "on"), prefix_cache_max_seqs=32, **kw), model=model,
                         piggyback=True)
            await eng.initialize()
            engines[mode] = eng
        admit = {m: [] for m in engines}
        decode = {m: [] for m in engines}
        decode_calls = {}
        for rep in range(a.repeats + 1):        # (the first repetition warms up: graph capture, BLAS algorithms)
            tails = [ids(16) for _ in range(4)]
            for mode, eng in engines.items():   # the two modes alternate on the same prompts
                if mode == "on":
                    eng.drop_prefix_cache()
                    await serve(eng, [shared + ids(16)], 2, False)      # the donor: 1024 + 1 tokens, 64 whole blocks
                hits = eng.num_prefix_hit_tokens
                calls.clear()
                times = await serve(eng, [shared + t for t in tails], 3, True)
                assert eng.num_prefix_hit_tokens - hits == (4 * 1008 if mode == "on" else 0)
                assert calls[0][0] == ([16] * 4 if mode == "on" else [1024] * 4) and calls[1][0] == [1] * 4
                decode_calls[mode] = calls[1]
                if rep:
                    admit[mode].append(times[0])
                    decode[mode].append(times[1])
                eng.drop_prefix_cache()         # (the two engines hand out the same block-table rows of one model)
            assert decode_calls["on"] == decode_calls["off"], decode_calls
        engines["on"].drop_prefix_cache()
        for mode in engines:
            print(json.dumps({"part": "step", "model": "llama3-8b dims, dummy weights, bfloat16", "prefix_caching": mode,
                              "prompts": 4, "prompt_tokens": 1024, "shared_tokens": 1008,
                              "admit_step_ms": spread(admit[mode], 3), "next_decode_step_ms": spread(decode[mode], 3),
                              "decode_forward_call_identical": True, "repetitions": a.repeats}), flush=True)
    asyncio.run(run())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["copy", "step", "both"], default="both")
    ap.add_argument("--pool-blocks", type=int, default=6144, help="1 MiB blocks per pool (two pools)")
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prefix_cache_micro.py measures on the GPU; there is no CPU figure"
    if a.part in ("copy", "both"):
        part_copy(a)
    if a.part in ("step", "both"):
        part_step(a)


if __name__ == "__main__":
    main()
