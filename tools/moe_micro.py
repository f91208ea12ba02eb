"""Timing of the mixture-of-experts FFN (csrc/moe.hip) on the GPU, next to the per-expert loop HuggingFace's eager model runs.
Nothing here is asserted anywhere.

    python tools/moe_micro.py [--iters 200] [--repeats 5] [--sections ffn:qwen3_30b_a3b,ffn:mixtral_8x7b,step] [--out FILE]
    python tools/moe_micro.py --sections wide:qwen3_30b_a3b,wide:mixtral_8x7b --out profiles/moe_wide_micro.json

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
wide:<geometry>  The two forms of the expert GEMMs side by side (same weights and inputs as ffn:) at T = 64, 128, 256, 512,
    1024, 2048 (one call where T k <= 4096) and 4096 (token blocks): us of up_gate_silu, down (one-call steps) and the whole
    FFN with the form forced to the 16-row kernels (`rt0`) and to each row_tiles the wide kernels take (`rt2`, `rt4`), what
    the chooser picks (`chosen`), and the torch loop in the same run. The forms' outputs are compared bit for bit first.
step  A whole decode step at Qwen3-30B-A3B dimensions (48 layers, dummy weights, bfloat16, 1024-token contexts) at batch
    1 / 8 / 32: host wall time per forward() on graph replay.
fp8:<geometry>  The 16-bit and the FP8 (e4m3, csrc/moe_fp8.hip) FFN of one layer in ONE run, alternating, on the same inputs
    (the FP8 stacks are the 16-bit ones quantised per row as the loader does) at T = 1, 8, 32, 128 and 1024 (the wide form
    where the chooser takes it): us of the whole FFN per dtype, the distinct active experts, TB/s over THEIR bytes (3 I H x
    2 or x 1 bytes, the scales' 4 (2 I + H) on top), `fp8_over_16` (medians) and `ranges_ok`: the FP8 range does not lie
    above the 16-bit range of the same run. The ideal is half the expert bytes; everything else in the FFN is unchanged.
fp8_block:<geometry>  `fp8` with a third form in the same alternation: the block-scaled FP8 FFN (csrc/moe_fp8_block.hip; the
    16-bit stacks quantised per 128 x 128 block with torch, as the published checkpoints are). Per T: us of bf16, per-row FP8
    (`fp8`) and block FP8 (`fp8_block`: the form the chooser takes; from 128 tokens on also `fp8_block_rt0` / `fp8_block_rt2`,
    the 16-row and the 2-tile form forced), `block_over_row` (medians) and `within_row_range`: the block median does not lie
    above the per-row maximum of the same run by more than the per-row range.
step_fp8  `step` for both expert dtypes in one process, the 16-bit model first.
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
SECTION_TIMEOUT_S = {"ffn": 300, "wide": 420, "step": 420, "fp8": 300, "fp8_block": 420, "step_fp8": 840}


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


def wide_section(name, iters, repeats):
    from swiftllm_amd.worker.kernels import moe as M
    from swiftllm_amd.worker.kernels.linear import linear
    H, I, E, k = GEOMETRIES[name]
    dt, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    u = lambda *shape: torch.empty(shape, dtype=dt, device=dev).uniform_(-1e-3, 1e-3, generator=g)     # noqa: E731
    router, up_gate, down = u(E, H), u(E, 2 * I, H), u(E, H, I)
    out = {}
    for T in (64, 128, 256, 512, 1024, 2048, 4096):
        n = max(2, iters // (1 if T < 256 else 10 if T < 2048 else 40))
        x = torch.randn((T, H), device=dev, generator=g).to(dt)
        res = {"chosen": [M.wide_row_tiles(min(T - t0, M.max_pairs() // k), k, E, H, I)
                          for t0 in range(0, T, M.max_pairs() // k)]}
        base = M.moe_ffn(x, router, up_gate, down, k, True, wide_tiles=0)
        one_call = T * k <= M.max_pairs()
        if one_call:
            ids, _ = M.moe_route(linear(x, router, False), k, True)
            rows, experts = M.moe_align(ids, E)
        for rt in (0,) + M.WIDE_ROW_TILES:
            assert torch.equal(M.moe_ffn(x, router, up_gate, down, k, True, wide_tiles=rt).view(torch.int16),
                               base.view(torch.int16)), (T, rt)
            form = {"ffn": _summary(_timed(lambda: M.moe_ffn(x, router, up_gate, down, k, True, wide_tiles=rt), n, repeats))}
            if one_call:
                act = M.moe_up_gate_silu(x, up_gate, rows, experts, k, row_tiles=rt)
                y = M.moe_down(act, down, rows, experts, k, row_tiles=rt)
                form["up_gate_silu"] = _summary(_timed(
                    lambda: M.moe_up_gate_silu(x, up_gate, rows, experts, k, act, rt), n, repeats))
                form["down"] = _summary(_timed(lambda: M.moe_down(act, down, rows, experts, k, y, rt), n, repeats))
            res[f"rt{rt}"] = form
        res["hf_loop"] = _summary(_timed(lambda: hf_loop(x, router, up_gate, down, k, I), max(2, n // 4), repeats))
        out[f"wide_{name}_t{T}"] = res
    return out


def _block_quantise(w, halves):
    """[E, halves * rows, k] 16-bit -> (codes, block scales [E, halves * ceil(rows / 128), ceil(k / 128)]), in plain torch."""
    E, rows, k = w.shape[0], w.shape[1] // halves, w.shape[2]
    rb, kb = -(-rows // 128), -(-k // 128)
    p = torch.zeros((E, halves, rb * 128, kb * 128), dtype=torch.float32, device=w.device)
    p[:, :, :rows, :k] = w.view(E, halves, rows, k).float()
    scale = p.view(E, halves, rb, 128, kb, 128).abs().amax(dim=(3, 5)).clamp(min=1e-12) / 448.0
    codes = (p.view(E, halves, rb, 128, kb, 128) / scale[:, :, :, None, :, None]).view(E, halves, rb * 128, kb * 128)
    return codes[:, :, :rows, :k].to(torch.float8_e4m3fn).reshape(w.shape).contiguous(), scale.view(E, halves * rb, kb).contiguous()


def fp8_section(name, iters, repeats, block=False):
    from swiftllm_amd.worker.kernels import moe as M
    H, I, E, k = GEOMETRIES[name]
    dt, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    u = lambda *shape: torch.empty(shape, dtype=dt, device=dev).uniform_(-1e-3, 1e-3, generator=g)     # noqa: E731
    router, stacks16 = u(E, H), (u(E, 2 * I, H), u(E, H, I))
    stacks8, scales = [], []
    for w in stacks16:
        scale, inv = M.row_scales(w.view(-1, w.shape[-1]))
        stacks8.append(M.quantise_rows(w.view(-1, w.shape[-1]), inv, torch.empty(w.shape, dtype=M.FP8, device=dev).view(
            -1, w.shape[-1])).view(w.shape))
        scales.append(scale.view(w.shape[:2]))
    forms = {"bf16": (lambda x: M.moe_ffn(x, router, *stacks16, k, True), 3 * I * H * 2),
             "fp8": (lambda x: M.moe_ffn(x, router, *stacks8, k, True, up_gate_scale=scales[0], down_scale=scales[1]),
                     3 * I * H + 4 * (2 * I + H))}
    if block:
        (ug8, ug_s), (dn8, dn_s) = _block_quantise(stacks16[0], 2), _block_quantise(stacks16[1], 1)
        ffn_b = lambda x, wt=-1: M.moe_ffn(x, router, ug8, dn8, k, True, wide_tiles=wt, up_gate_bscale=ug_s,     # noqa: E731
                                           down_bscale=dn_s)
        forms["fp8_block"] = (ffn_b, 3 * I * H + 4 * (ug_s[0].numel() + dn_s[0].numel()))
    out = {}
    for T in (1, 8, 32, 128, 1024):
        n = iters if T < 1024 else max(2, iters // 10)
        x = torch.randn((T, H), device=dev, generator=g).to(dt)
        tap = []
        M.moe_ffn(x, router, *stacks16, k, True, tap=tap)
        active = int(torch.unique(tap[0][1]).numel())
        if block and T >= 128:                              # both forms of the block kernels, forced
            forms["fp8_block_rt0"] = (lambda x: ffn_b(x, 0), forms["fp8_block"][1])
            forms["fp8_block_rt2"] = (lambda x: ffn_b(x, 2), forms["fp8_block"][1])
        runs = {f: [] for f in forms}
        for _ in range(repeats):                            # alternating: both dtypes see the same neighbours on the machine
            for f, (fn, _) in forms.items():
                runs[f] += _timed(lambda: fn(x), n, 1)
        res = {"active_experts": active, "wide_row_tiles": M.wide_row_tiles(T, k, E, H, I)}
        for f, (_, expert_bytes) in forms.items():
            res[f] = dict(_summary(runs[f]), tb_s=round(active * expert_bytes / statistics.median(runs[f]) / 1e6, 3))
        res["fp8_over_16"] = round(res["fp8"]["median_us"] / res["bf16"]["median_us"], 3)
        res["ranges_ok"] = res["fp8"]["min_us"] <= res["bf16"]["max_us"]
        if block:
            res["block_over_row"] = round(res["fp8_block"]["median_us"] / res["fp8"]["median_us"], 3)
            res["within_row_range"] = (res["fp8_block"]["median_us"] - res["fp8"]["median_us"]
                                       <= res["fp8"]["max_us"] - res["fp8"]["min_us"])
        out[f"fp8{'_block' if block else ''}_{name}_t{T}"] = res
    return out


def step_section(moe_weight_dtypes=("auto",)):
    out = {}
    for mwd in moe_weight_dtypes:
        res = _steps(mwd)
        out.update(res if mwd == "auto" else {f"{mwd}_{key}": v for key, v in res.items()})
    return out


def _steps(moe_weight_dtype):
    from swiftllm_amd import EngineConfig, LlamaModel
    S, steps, out = 1024, 32, {}
    path = tempfile.mkdtemp(prefix="swl_moe_micro_")
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(QWEN3_30B_A3B, f)
    max_len = S + steps + 80
    batch_max = 32
    ec = EngineConfig(model_path=path, use_dummy=True, block_size=16, gpu_mem_utilization=0.97, num_cpu_blocks=0,
                      max_seqs_in_block_table=batch_max + 64, max_blocks_per_seq=max_len // 16 + 8, max_batch_size=batch_max,
                      max_tokens_in_batch=4096, dtype="bfloat16", use_hip_graph=True, moe_weight_dtype=moe_weight_dtype)
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
        res = (ffn_section(name, a.iters, a.repeats) if kind == "ffn" else
               wide_section(name, a.iters, a.repeats) if kind == "wide" else
               fp8_section(name, a.iters, a.repeats) if kind == "fp8" else
               fp8_section(name, a.iters, a.repeats, block=True) if kind == "fp8_block" else
               step_section(("auto", "fp8_e4m3")) if kind == "step_fp8" else step_section())
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
