"""Timing of the mixture-of-experts FFN (csrc/moe.hip) on the GPU, next to the per-expert loop HuggingFace's eager model runs.
Nothing here is asserted anywhere.

    python tools/moe_micro.py [--iters 200] [--repeats 5] [--sections ffn:qwen3_30b_a3b,ffn:mixtral_8x7b,step] [--out FILE]

Run without --child it starts one fresh child process per section, each under its own `timeout -k 10`, and stops at the
first that fails (nothing more is started on the GPU after a fault or a time limit); the children's JSON is merged into one
line (and written to --out).

ffn:<geometry>  One layer's FFN with dummy weights U(-1e-3, 1e-3) — the router's included, so routing is near-uniform over
    the experts — in bfloat16, Qwen3-30B-A3B (H 2048, I 768, E 128, k 8) or Mixtral-8x7B (H 4096, I 14336, E 8, k 2), at
    T = 1, 8, 32, 128 decode tokens and, not gated, 1024 and 4096. Per T: us of the whole FFN (router GEMM, route, align,
    up_gate_silu, down, combine — `moe_ffn`), us per stage where the step fits one call, the number of DISTINCT active
    experts read off the routed ids, and TB/s over THEIR bytes (3 I H 2 bytes each) for the two GEMM stages and for the
    whole FFN. Yardstick in the same run: the loop HF's eager experts module runs, with torch on the GPU — router
    F.linear, softmax, top-k, the host synchronisation that finds the experts hit, then per active expert index_select ->
    F.linear x 3 (up, gate, down) -> index_add. `ours_over_loop` < 1 means ours is faster.
step  A whole decode step at Qwen3-30B-A3B dimensions (48 layers, dummy weights, bfloat16, 1024-token contexts) at batch
    1 / 8 / 32: host wall time per forward() on graph replay.
Each kernel figure is the median of `--repeats` runs of `--iters` back-to-back launches between two device events (a tenth
of the iterations from 1024 tokens on), with the range [min, max].
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRIES = {"qwen3_30b_a3b": (2048, 768, 128, 8), "mixtral_8x7b": (4096, 14336, 8, 2)}
QWEN3_30B_A3B = dict(model_type="qwen3_moe", hidden_act="silu", hidden_size=2048, intermediate_size=6144,
                     moe_intermediate_size=768, num_hidden_layers=48, num_attention_heads=32, num_key_value_heads=4,
                     head_dim=128, num_experts=128, num_experts_per_tok=8, norm_topk_prob=True, decoder_sparse_step=1,
                     mlp_only_layers=[], vocab_size=151936, max_position_embeddings=40960, rms_norm_eps=1e-6,
                     rope_theta=1000000.0, tie_word_embeddings=False)
SECTION_TIMEOUT_S = {"ffn": 300, "step": 420}


def _timed(fn, iters, repeats):
    for _ in range(5):
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


def hf_loop(x, router, up_gate, down, k, inter):
    """What HF's eager sparse block computes, on our [up ; gate] stack: one host synchronisation, 3 F.linear per expert hit."""
    logits = F.linear(x, router)
    probs = torch.softmax(logits, dim=-1, dtype=torch.float)
    w, idx = torch.topk(probs, k, dim=-1)
    w = (w / w.sum(dim=-1, keepdim=True)).to(x.dtype)
    out = torch.zeros_like(x)
    mask = F.one_hot(idx, num_classes=router.shape[0]).permute(2, 1, 0)
    for e in torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero():        # (the host synchronisation)
        e = int(e[0])
        pos, tok = torch.where(mask[e])
        cur = x.index_select(0, tok)
        h = F.silu(F.linear(cur, up_gate[e, inter:])) * F.linear(cur, up_gate[e, :inter])
        out.index_add_(0, tok, F.linear(h, down[e]) * w[tok, pos, None])
    return out


def ffn_section(name, iters, repeats):
    from swiftllm_amd.worker.kernels import moe as M
    from swiftllm_amd.worker.kernels.linear import linear
    H, I, E, k = GEOMETRIES[name]
    dt, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    u = lambda *shape: torch.empty(shape, dtype=dt, device=dev).uniform_(-1e-3, 1e-3, generator=g)     # noqa: E731
    router, up_gate, down = u(E, H), u(E, 2 * I, H), u(E, H, I)
    expert_bytes = 3 * I * H * 2
    out = {}
    for T in (1, 8, 32, 128, 1024, 4096):
        n = iters if T < 1024 else max(2, iters // 10)
        x = torch.randn((T, H), device=dev, generator=g).to(dt)
        res = {}
        ours = _timed(lambda: M.moe_ffn(x, router, up_gate, down, k, True), n, repeats)
        loop = _timed(lambda: hf_loop(x, router, up_gate, down, k, I), max(2, n // 4), repeats)
        tap = []                                # (the routed ids of the whole step, whatever its token blocks)
        M.moe_ffn(x, router, up_gate, down, k, True, tap=tap)
        active = int(torch.unique(tap[0][1]).numel())
        res.update(ffn=_summary(ours), hf_loop=_summary(loop), active_experts=active,
                   ours_over_loop=round(statistics.median(ours) / statistics.median(loop), 3),
                   ffn_tb_s=round(active * expert_bytes / statistics.median(ours) / 1e6, 3))
        if T * k <= M.max_pairs():
            logits = linear(x, router, False)
            ids, w = M.moe_route(logits, k, True)
            rows, experts = M.moe_align(ids, E)
            act = M.moe_up_gate_silu(x, up_gate, rows, experts, k)
            y = M.moe_down(act, down, rows, experts, k)
            o = torch.empty_like(x)
            stages = dict(router=lambda: linear(x, router, False), route=lambda: M.moe_route(logits, k, True),
                          align=lambda: M.moe_align(ids, E),
                          up_gate_silu=lambda: M.moe_up_gate_silu(x, up_gate, rows, experts, k, act),
                          down=lambda: M.moe_down(act, down, rows, experts, k, y), combine=lambda: M.moe_combine(y, w, o))
            med = {}
            for stage, fn in stages.items():
                runs = _timed(fn, n, repeats)
                res[stage] = _summary(runs)
                med[stage] = statistics.median(runs)
            res["up_gate_silu_tb_s"] = round(active * 2 * I * H * 2 / med["up_gate_silu"] / 1e6, 3)
            res["down_tb_s"] = round(active * I * H * 2 / med["down"] / 1e6, 3)
        out[f"{name}_t{T}"] = res
    return out


def step_section():
    from swiftllm_amd import EngineConfig, LlamaModel
    S, steps, out = 1024, 32, {}
    path = tempfile.mkdtemp(prefix="swl_moe_micro_")
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(QWEN3_30B_A3B, f)
    max_len = S + steps + 80
    batch_max = 32
    ec = EngineConfig(model_path=path, use_dummy=True, block_size=16, gpu_mem_utilization=0.97, num_cpu_blocks=0,
                      max_seqs_in_block_table=batch_max + 64, max_blocks_per_seq=max_len // 16 + 8, max_batch_size=batch_max,
                      max_tokens_in_batch=4096, dtype="bfloat16", use_hip_graph=True)
    model = LlamaModel(ec)
    model.load_weights()
    model.init_kvcache_and_swap(batch_max * (max_len // 16 + 2) + 64)
    g = torch.Generator().manual_seed(1)
    for batch in (1, 8, 32):
        seqs = list(range(batch))
        toks = []
        for s0 in range(0, batch, 4):        # prompts in steps of 4 x 1024 tokens
            part = seqs[s0:s0 + 4]
            toks += model.forward([torch.randint(0, 151936, (S,), generator=g).tolist() for _ in part], part, [])
        lens, times = [S] * batch, []
        for i in range(steps + 4):
            lens = [n + 1 for n in lens]
            t = time.perf_counter()
            toks = model.forward([[x] for x in toks], seqs, lens)
            if i >= 4:      # (the first steps capture and warm the graph)
                times.append(time.perf_counter() - t)
        model.free_seqs_resources(seqs)
        out[f"qwen3_30b_a3b_b{batch}_step_ms"] = {"median": round(1000.0 * statistics.median(times), 3),
                                                  "min": round(1000.0 * min(times), 3),
                                                  "max": round(1000.0 * max(times), 3), "n": len(times)}
    out["graph_captures"] = model.replay.captures
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sections", default="ffn:qwen3_30b_a3b,ffn:mixtral_8x7b,step")
    ap.add_argument("--child", default="", help="(internal) run one section in this process")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        assert torch.cuda.is_available(), "needs a HIP device"
        kind, _, name = a.child.partition(":")
        res = ffn_section(name, a.iters, a.repeats) if kind == "ffn" else step_section()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    merged = {"iters": a.iters, "repeats": a.repeats}
    for section in [s for s in a.sections.split(",") if s]:
        limit = SECTION_TIMEOUT_S[section.partition(":")[0]]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", section,
               "--iters", str(a.iters), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"[moe_micro] section {section} ended with status {r.returncode}; nothing more is started\n"
                  f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr, flush=True)
            merged["failed"] = {"section": section, "status": r.returncode}
            break
        merged.update(json.loads(lines[-1][len("RESULT "):]))
        print(f"[moe_micro] {section} done", file=sys.stderr, flush=True)
    line = json.dumps(merged)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    return 1 if "failed" in merged else 0


if __name__ == "__main__":
    sys.exit(main())
