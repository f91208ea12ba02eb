"""Timing of the dense block-scaled FP8 projections (csrc/gemm_fp8_block.hip) on the GPU, next to the 16-bit decode GEMM route on
the same shapes. Nothing here is asserted anywhere.

    python tools/dense_fp8_micro.py [--iters 200] [--repeats 5] [--sections gemm,step] [--out profiles/dense_fp8_micro.json]
                                    [--ms 65,128,192,256] [--batches 128,256]

Run without --child it starts one fresh child process per section, each under its own `timeout -k 10`, and stops at the first
that fails (nothing more is started on the GPU after a fault or a time limit).

gemm  Llama-3-8B's four projections — qkv (6144, 4096), o (4096, 4096), up/gate + SiLU (2 x 14336, 4096), down (4096, 14336) —
      with dummy weights in bfloat16 at M = 1, 8, 32, 64: us of the FP8 GEMM (`fp8`) and of the existing 16-bit route on a
      packed weight (`bf16`: linear(skinny=True) / linear_silu_gate), alternating in one process; TB/s of codes for `fp8`;
      `fp8_over_16` (medians; the ideal is 0.5). At M = 64 and 128 also the dequantise + library GEMM route (`dequant`).
      Above 64 rows (--ms 65,128,192,256) also the wide FP8 kernel (`wide`, csrc/gemm_fp8_block_wide.hip: what
      EngineConfig.dense_fp8_wide runs in place of `dequant`), with `wide_over_dequant`, `wide_over_16` and whether the
      wide kernel's range of repeats lies wholly below the dequantising route's (`wide_wins`).
step  A whole decode step at Llama-3-8B dimensions (32 layers, dummy weights, bfloat16, 1024-token contexts) on graph replay
      at batch 1, 8, 32 and 128 (--batches): host wall time per forward() — which ends in the copy of the sampled tokens to the host, so
      the clock stops behind the step's last kernel — the bf16 model first, then the FP8 one, then the FP8 one with
      dense_fp8_wide (`fp8_block_wide`), in one process.
row_gemm  The same four shapes at M = 1, 8, 32, 64, three forms alternating in one run: the packed bf16 GEMM (`bf16`), the
      block-scaled FP8 GEMM (`fp8_block`) and the per-row FP8 GEMM on packed codes (`fp8_row`, csrc/gemm_fp8_row.hip), with
      `row_over_16` and `row_over_block` (medians).
row_step  The decode step of `step` at batch 1, 8, 32: the bf16 model, then the model with dense_weight_dtype "fp8_e4m3".
mx_gemm   The same four shapes at M = 1, 8, 32, 64, three forms alternating in one run: the packed bf16 GEMM (`bf16`), the
      per-row FP8 GEMM (`fp8_row`) and the MXFP4 GEMM (`mxfp4`, csrc/gemm_mxfp4.hip), with `mx_over_16` and `mx_over_row`
      (medians). Repeated launches on one weight read partly from the last-level cache, all three forms alike.
mx_step   The decode step at batch 1, 8, 32: the bf16 model, the "fp8_e4m3" model, then the "mxfp4" model, in one process.
Each kernel figure is the median of `--repeats` runs of `--iters` back-to-back launches between two device events, with the
range [min, max]; the forms alternate inside every repeat.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"qkv": ((4096, 1024, 1024), 4096), "o": ((4096,), 4096), "up_gate_silu": ((14336, 14336), 4096), "down": ((4096,), 14336)}
LLAMA3_8B = dict(model_type="llama", hidden_act="silu", hidden_size=4096, intermediate_size=14336, num_hidden_layers=32,
                 num_attention_heads=32, num_key_value_heads=8, vocab_size=128256, max_position_embeddings=8192,
                 rms_norm_eps=1e-5, rope_theta=500000.0, tie_word_embeddings=False)
QUANT = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}
SECTION_TIMEOUT_S = {"gemm": 400, "step": 500, "row_gemm": 400, "row_step": 500, "mx_gemm": 400, "mx_step": 700}


def _timed(fn, iters):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / iters


def _summary(runs):
    return {"median_us": round(statistics.median(runs), 2), "min_us": round(min(runs), 2), "max_us": round(max(runs), 2)}


def gemm_section(iters, repeats, ms=(1, 8, 32, 64, 128)):
    from swiftllm_amd.worker.kernels import linear_fp8 as L
    from swiftllm_amd.worker.kernels.linear import linear, linear_silu_gate, pack_weight
    dt, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for name, (segments, k) in SHAPES.items():
        n = sum(segments)
        w16 = torch.empty((n, k), dtype=dt, device=dev).uniform_(-1e-3, 1e-3, generator=g)
        pack_weight(w16)
        codes = torch.empty((n, k), dtype=dt, device=dev).uniform_(-1.0, 1.0, generator=g).to(L.FP8)
        bscale = torch.full((L.scale_rows(segments), L.blocks(k)), 1e-3, dtype=torch.float32, device=dev)
        silu = name == "up_gate_silu"
        for m in ms:
            x = torch.randn((m, k), device=dev, generator=g).to(dt)
            forms = {}

            def bf16():
                y = linear_silu_gate(x, w16) if silu else linear(x, w16, True)
                if y is None:                               # (a shape the one-launch SiLU-gate form does not take)
                    L.silu_and_mul_inplace(linear(x, w16, True))
            if m <= L.MAX_M:
                forms["fp8"] = ((lambda: L.linear_silu_gate_fp8_block(x, codes, bscale, segments[0])) if silu else
                                (lambda: L.linear_fp8_block(x, codes, bscale, segments)))
                forms["bf16"] = bf16
            if m >= L.MAX_M:                                # the dequantising route, forced below its cutoff at M = 64
                def dequant():
                    y = linear(x, L.dequantised(codes, bscale, segments, dt))
                    if silu:
                        L.silu_and_mul_inplace(y)
                forms["dequant"] = dequant
                forms.setdefault("bf16", bf16)
            if L.MAX_M < m <= L.WIDE_MAX_M:
                forms["wide"] = ((lambda: L.linear_silu_gate_fp8_block(x, codes, bscale, segments[0], wide=True)) if silu else
                                 (lambda: L.linear_fp8_block(x, codes, bscale, segments, wide=True)))
            runs = {f: [] for f in forms}
            for _ in range(repeats):
                for f, fn in forms.items():
                    runs[f].append(_timed(fn, iters))
            res = {f: _summary(r) for f, r in runs.items()}
            if "fp8" in res:
                res["fp8"]["codes_tb_s"] = round(n * k / res["fp8"]["median_us"] / 1e6, 3)
                res["fp8_over_16"] = round(res["fp8"]["median_us"] / res["bf16"]["median_us"], 3)
                res["k_splits"] = L.choose_splits(segments[0] if silu else n, k)
            if "wide" in res:
                res["wide"]["codes_tb_s"] = round(n * k / res["wide"]["median_us"] / 1e6, 3)
                res["wide_over_dequant"] = round(res["wide"]["median_us"] / res["dequant"]["median_us"], 3)
                res["wide_over_16"] = round(res["wide"]["median_us"] / res["bf16"]["median_us"], 3)
                res["wide_wins"] = res["wide"]["max_us"] < res["dequant"]["min_us"]
                res["wide_k_splits"] = L.choose_splits_wide(n, k)
            out[f"{name}_m{m}"] = res
    return out


def row_gemm_section(iters, repeats, ms=(1, 8, 32, 64)):
    from swiftllm_amd.worker.kernels import linear_fp8 as L
    from swiftllm_amd.worker.kernels import linear_fp8_row as LR
    from swiftllm_amd.worker.kernels.linear import linear, linear_silu_gate, pack_weight
    dt, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for name, (segments, k) in SHAPES.items():
        n = sum(segments)
        w16 = torch.empty((n, k), dtype=dt, device=dev).uniform_(-1e-3, 1e-3, generator=g)
        pack_weight(w16)
        codes = torch.empty((n, k), dtype=dt, device=dev).uniform_(-1.0, 1.0, generator=g).to(L.FP8)
        bscale = torch.full((L.scale_rows(segments), L.blocks(k)), 1e-3, dtype=torch.float32, device=dev)
        rcodes = torch.empty((n, k), dtype=L.FP8, device=dev)
        rscale = LR.quantise_pack_rows(w16, rcodes)
        silu = name == "up_gate_silu"
        for m in [m for m in ms if m <= LR.MAX_M]:
            x = torch.randn((m, k), device=dev, generator=g).to(dt)

            def bf16():
                y = linear_silu_gate(x, w16) if silu else linear(x, w16, True)
                if y is None:
                    L.silu_and_mul_inplace(linear(x, w16, True))
            forms = {"bf16": bf16,
                     "fp8_block": ((lambda: L.linear_silu_gate_fp8_block(x, codes, bscale, segments[0])) if silu else
                                   (lambda: L.linear_fp8_block(x, codes, bscale, segments))),
                     "fp8_row": ((lambda: LR.linear_silu_gate_fp8_row(x, rcodes, rscale)) if silu else
                                 (lambda: LR.linear_fp8_row(x, rcodes, rscale)))}
            runs = {f: [] for f in forms}
            for _ in range(repeats):
                for f, fn in forms.items():
                    runs[f].append(_timed(fn, iters))
            res = {f: _summary(r) for f, r in runs.items()}
            res["fp8_row"]["codes_tb_s"] = round(n * k / res["fp8_row"]["median_us"] / 1e6, 3)
            res["row_over_16"] = round(res["fp8_row"]["median_us"] / res["bf16"]["median_us"], 3)
            res["row_over_block"] = round(res["fp8_row"]["median_us"] / res["fp8_block"]["median_us"], 3)
            res["k_splits"] = LR.choose_splits(segments[0] if silu else n, k)
            out[f"row_{name}_m{m}"] = res
    return out


def mx_gemm_section(iters, repeats, ms=(1, 8, 32, 64)):
    from swiftllm_amd.worker.kernels import linear_fp8 as L
    from swiftllm_amd.worker.kernels import linear_fp8_row as LR
    from swiftllm_amd.worker.kernels import linear_mxfp4 as LM
    from swiftllm_amd.worker.kernels.linear import linear, linear_silu_gate, pack_weight
    dt, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for name, (segments, k) in SHAPES.items():
        n = sum(segments)
        w16 = torch.empty((n, k), dtype=dt, device=dev).uniform_(-1e-3, 1e-3, generator=g)
        pack_weight(w16)
        rcodes = torch.empty((n, k), dtype=L.FP8, device=dev)
        rscale = LR.quantise_pack_rows(w16, rcodes)
        mcodes = torch.empty((n, k // 2), dtype=torch.uint8, device=dev)
        mscales = torch.empty((LM.scale_bytes(n, k),), dtype=torch.uint8, device=dev)
        LM.quantise_pack_rows(w16, mcodes, mscales)
        silu = name == "up_gate_silu"
        for m in [m for m in ms if m <= LM.MAX_M]:
            x = torch.randn((m, k), device=dev, generator=g).to(dt)

            def bf16():
                y = linear_silu_gate(x, w16) if silu else linear(x, w16, True)
                if y is None:
                    L.silu_and_mul_inplace(linear(x, w16, True))
            forms = {"bf16": bf16,
                     "fp8_row": ((lambda: LR.linear_silu_gate_fp8_row(x, rcodes, rscale)) if silu else
                                 (lambda: LR.linear_fp8_row(x, rcodes, rscale))),
                     "mxfp4": ((lambda: LM.linear_silu_gate_mxfp4(x, mcodes, mscales)) if silu else
                               (lambda: LM.linear_mxfp4(x, mcodes, mscales)))}
            runs = {f: [] for f in forms}
            for _ in range(repeats):
                for f, fn in forms.items():
                    runs[f].append(_timed(fn, iters))
            res = {f: _summary(r) for f, r in runs.items()}
            res["mxfp4"]["codes_tb_s"] = round((mcodes.numel() + mscales.numel()) / res["mxfp4"]["median_us"] / 1e6, 3)
            res["mx_over_16"] = round(res["mxfp4"]["median_us"] / res["bf16"]["median_us"], 3)
            res["mx_over_row"] = round(res["mxfp4"]["median_us"] / res["fp8_row"]["median_us"], 3)
            res["k_splits"] = LM.choose_splits(segments[0] if silu else n, k)
            out[f"mx_{name}_m{m}"] = res
    return out


def step_section(batches=(1, 8, 32, 128), modes=("bf16", "fp8_block", "fp8_block_wide")):
    from swiftllm_amd import EngineConfig, LlamaModel
    S, steps, batch_max, out = 1024, 32, max(batches), {}
    for mode in modes:
        path = tempfile.mkdtemp(prefix="swl_dense_fp8_micro_")
        with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
            json.dump(dict(LLAMA3_8B, **({"quantization_config": QUANT} if mode.startswith("fp8_block") else {})), f)
        max_len = S + steps + 80
        ec = EngineConfig(model_path=path, use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=0,
                          max_seqs_in_block_table=batch_max + 64, max_blocks_per_seq=max_len // 16 + 8, max_batch_size=batch_max,
                          max_tokens_in_batch=4096, dtype="bfloat16", use_hip_graph=True,
                          dense_weight_dtype={"bf16": "auto", "fp8_row": "fp8_e4m3", "mxfp4": "mxfp4"}.get(mode, "fp8_block"),
                          dense_fp8_wide=mode == "fp8_block_wide")
        model = LlamaModel(ec)
        model.load_weights()
        model.init_kvcache_and_swap(batch_max * (max_len // 16 + 2) + 64)
        g = torch.Generator().manual_seed(1)
        for batch in batches:
            seqs, toks = list(range(batch)), []
            for s0 in range(0, batch, 4):                   # prompts in steps of 4 x 1024 tokens
                part = seqs[s0:s0 + 4]
                toks += model.forward([torch.randint(0, 128256, (S,), generator=g).tolist() for _ in part], part, [])
            lens, times = [S] * batch, []
            for i in range(steps + 4):
                lens = [n + 1 for n in lens]
                t = time.perf_counter()
                toks = model.forward([[x] for x in toks], seqs, lens)
                if i >= 4:                                  # (the first steps capture and warm the graph)
                    times.append(time.perf_counter() - t)
            model.free_seqs_resources(seqs)
            out[f"{mode}_b{batch}_step_ms"] = {"median": round(1000.0 * statistics.median(times), 3),
                                               "min": round(1000.0 * min(times), 3), "max": round(1000.0 * max(times), 3)}
        out[f"{mode}_graph_captures"] = model.replay.captures
        del model
        torch.cuda.empty_cache()
        shutil.rmtree(path, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sections", default="gemm,step")
    ap.add_argument("--ms", default="1,8,32,64,128", help="token counts of the gemm section")
    ap.add_argument("--batches", default="1,8,32,128", help="batch sizes of the step section")
    ap.add_argument("--child", default="", help="(internal) run one section in this process")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        assert torch.cuda.is_available(), "needs a HIP device"
        ms, batches = [int(v) for v in a.ms.split(",")], [int(v) for v in a.batches.split(",")]
        run = {"gemm": lambda: gemm_section(a.iters, a.repeats, ms), "step": lambda: step_section(batches),
               "row_gemm": lambda: row_gemm_section(a.iters, a.repeats, ms),
               "row_step": lambda: step_section([b for b in batches if b <= 32], ("bf16", "fp8_row")),
               "mx_gemm": lambda: mx_gemm_section(a.iters, a.repeats, ms),
               "mx_step": lambda: step_section([b for b in batches if b <= 32], ("bf16", "fp8_row", "mxfp4"))}[a.child]
        print("RESULT " + json.dumps(run()), flush=True)
        return 0
    merged = {"iters": a.iters, "repeats": a.repeats}
    for section in [s for s in a.sections.split(",") if s]:
        cmd = ["timeout", "-k", "10", str(SECTION_TIMEOUT_S[section]), sys.executable, os.path.abspath(__file__), "--child",
               section, "--iters", str(a.iters), "--repeats", str(a.repeats), "--ms", a.ms, "--batches", a.batches]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"[dense_fp8_micro] section {section} ended with status {r.returncode}; nothing more is started\n"
                  f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr, flush=True)
            merged["failed"] = {"section": section, "status": r.returncode}
            break
        merged.update(json.loads(lines[-1][len("RESULT "):]))
        print(f"[dense_fp8_micro] {section} done", file=sys.stderr, flush=True)
    line = json.dumps(merged)
    print(line)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    return 1 if "failed" in merged else 0


if __name__ == "__main__":
    sys.exit(main())
