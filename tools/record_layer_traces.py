#!/usr/bin/env python3
"""record_layer_traces.py — which kernels a forward launches, with which integer arguments, per engine configuration. (GPU box)

    python tools/record_layer_traces.py --out tests/golden/layer_launch_traces.json      # write the fixture
    python tools/record_layer_traces.py --bits DIR [--configs bf16,f16]                  # tapped logits + tokens of every cell

The launch route of a transformer layer (worker/layers/transformer_layer.py: decide_route) is a function of the engine
configuration and a handful of step facts. This tool runs a fixed set of cells — one model per configuration, a list of
scenarios against each — through the public model API with `_hip.call` and `kernels.linear._blas_linear` replaced by
recorders, and keeps, for every launch of every forward, the entry name and its integer arguments (pointer, size_t and
float positions are dropped by the entry's row of _hip.SIGNATURES / _hip._SPECIAL; a library GEMM is "blas", M, N, K).
tests/test_gpu_layer_routes.py replays the cells and holds every trace to the committed fixture, element for element: a
change of the layer's control flow that is meant to launch what the layer launched before is checked against what it
launched before. The fixture is written by running this tool at the commit whose launches are the yardstick.

Fixture layout: {"calls": [[name, int, ...], ...] (every distinct launch once), "cells": {config: {scenario: [[index into
calls, ...] per forward]}}}.
"""
import argparse
import ctypes
import importlib
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch    # noqa: E402

from oracle import synth    # noqa: E402

# hidden 4096, 32/8 heads of 128, FFN 14336: the smallest geometry at which the rows, NX, tiny and split-K rules all fire
WIDE = dict(num_hidden_layers=2, hidden_size=4096, num_attention_heads=32, num_key_value_heads=8,
            intermediate_size=14336, vocab_size=4096, max_position_embeddings=2048, rope_theta=500000.0)
SMALL64 = dict(synth.SMALL64)
SWITCHES = ("fuse_rope_kvstore", "fuse_splitk_consumers", "fuse_rope_into_attention", "defer_rmsnorm",
            "tiny_decode_batches", "rows_decode")

# config name -> (geometry, engine options)
CONFIGS = {"bf16": (WIDE, dict(dtype="bfloat16")), "f16": (WIDE, dict(dtype="float16"))}
for _s in SWITCHES:
    CONFIGS["no_" + _s] = (WIDE, dict(dtype="bfloat16", tuning={_s: False}))
CONFIGS.update({
    "no_tiny_no_rows": (WIDE, dict(dtype="bfloat16", tuning=dict(tiny_decode_batches=False, rows_decode=False))),
    "no_skinny_gemm": (WIDE, dict(dtype="bfloat16", use_skinny_gemm=False)),
    "no_pack_decode_weights": (WIDE, dict(dtype="bfloat16", pack_decode_weights=False)),
    "no_fuse_qkv": (WIDE, dict(dtype="bfloat16", fuse_qkv=False)),
    "head64": (SMALL64, dict(dtype="bfloat16")),
    "fp8_kv": (SMALL64, dict(dtype="bfloat16", kv_cache_dtype="fp8_e4m3")),
    "lora": (SMALL64, dict(dtype="bfloat16", max_loras=2)),
})
GRAPH_CONFIG = "bf16_graph"     # --bits only: the default configuration replaying hipGraphs, pure-decode cells

DECODE_BATCHES = (1, 2, 3, 16, 17, 32, 33, 64, 100)
NUM_BLOCKS = 512

# what the fixture must reach at least once over all cells (the last two: either form counts)
REQUIRED = ("swl_gemm_rows_add", "swl_gemm_rows_add_ssq", "swl_gemm_skinny_packed_partial_nf",
            "swl_gemm_skinny_packed_partial_nx", "swl_gemm_skinny_packed_silu_gate_nf",
            "swl_gemm_skinny_packed_silu_gate_nx", "swl_gemm_skinny_packed_silu_gate_rs", "swl_splitk_add_scale",
            "swl_splitk_fused_add_rmsnorm", "swl_gemm_tiny_partial_from_splitk", "swl_gemm_tiny_silu_gate_from_splitk",
            "swl_gemm_tiny_partial_from_attn", "swl_paged_attn_decode_qkv_rs", "swl_paged_attn_decode_qkv",
            "swl_splitk_rotary_store_kv_decode", "swl_rotary_store_kv_decode", "swl_paged_attn_verify",
            "swl_paged_attn_decode_fp8", "swl_gemm_packed_mid_partial", "swl_gemm_packed_wide_partial", "swl_lora_shrink",
            "blas")
REQUIRED_ANY = (("swl_rotary_store_kv_prefill", "swl_rotary_store_kv_prefill_at"),)


def missing_names(names) -> list:
    names = set(names)
    return [n for n in REQUIRED if n not in names] + ["|".join(g) for g in REQUIRED_ANY if not names & set(g)]


class Recorder:
    """Replaces _hip.call and kernels.linear._blas_linear; `steps` grows by one list of launches per `begin()`."""

    def __init__(self):
        from swiftllm_amd import _hip
        # (the package re-exports the function `linear` under the module's name)
        self._hip, self._linear = _hip, importlib.import_module("swiftllm_amd.worker.kernels.linear")
        ints = (ctypes.c_int32, ctypes.c_int64)
        self._keep = {name: [i for i, t in enumerate(types) if t in ints] for name, types in _hip.SIGNATURES.items()}
        self._keep.update({name: [i for i, t in enumerate(types) if t in ints] for name, (types, _) in _hip._SPECIAL.items()})
        self.steps = []

    def __enter__(self):
        self._call, self._blas = self._hip.call, self._linear._blas_linear

        def call(name, *args):
            self.steps[-1].append([name] + [int(args[i]) for i in self._keep[name]])
            return self._call(name, *args)

        def blas(a, w, *rest, **kw):
            self.steps[-1].append(["blas", int(a.shape[0]), int(w.shape[0]), int(w.shape[1])])
            return self._blas(a, w, *rest, **kw)
        self._hip.call, self._linear._blas_linear = call, blas
        return self

    def __exit__(self, *exc):
        self._hip.call, self._linear._blas_linear = self._call, self._blas

    def begin(self):
        self.steps.append([])


def _prompts(lens, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lens]


def _random_adapter(cfg, rank, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    h, inter = cfg["hidden_size"], cfg["intermediate_size"]
    kv = cfg["num_key_value_heads"] * (h // cfg["num_attention_heads"])
    shapes = dict(q_proj=(h, h), k_proj=(kv, h), v_proj=(kv, h), o_proj=(h, h), up_proj=(inter, h), gate_proj=(inter, h),
                  down_proj=(h, inter))
    sd = {}
    for layer in range(cfg["num_hidden_layers"]):
        for m, (n, k) in shapes.items():
            key = f"base_model.model.model.layers.{layer}.{'mlp' if m in ('up_proj', 'gate_proj', 'down_proj') else 'self_attn'}.{m}"
            sd[key + ".lora_A.weight"] = (torch.randn(rank, k, generator=g) * 0.05).to(dtype)
            sd[key + ".lora_B.weight"] = (torch.randn(n, rank, generator=g) * 0.05).to(dtype)
    config = dict(peft_type="LORA", r=rank, lora_alpha=rank, target_modules=list(shapes), bias="none", use_dora=False,
                  use_rslora=False, modules_to_save=None)
    return sd, config


class Cells:
    """One model of one configuration and the scenarios run against it. `run(name)` returns (launches per forward, tokens
    per forward, tapped logits per forward); every scenario frees its sequences."""

    def __init__(self, config: str, model_dirs: dict):
        from swiftllm_amd import EngineConfig, LlamaModel
        graph = config == GRAPH_CONFIG
        # (the routing of 65..256-token projections: the measured table, never a timing of this run; read at every lookup)
        self._route_tune = os.environ.get("SWIFTLLM_ROUTE_TUNE")
        os.environ["SWIFTLLM_ROUTE_TUNE"] = "table"
        geometry, opts = CONFIGS["bf16" if graph else config]
        self.config, self.cfg, self.graph = config, synth.make_config(**geometry), graph
        self.dtype = getattr(torch, opts["dtype"])
        key = (geometry is WIDE, opts["dtype"])
        if key not in model_dirs:       # one checkpoint per (geometry, dtype), shared by the configurations
            make = synth.make_state_dict_on_gpu if geometry is WIDE else synth.make_state_dict
            model_dirs[key] = synth.write_model_dir(tempfile.mkdtemp(prefix="swl_traces_"), self.cfg,
                                                    make(self.cfg, seed=23, dtype=self.dtype))
        self.model = LlamaModel(EngineConfig(
            model_path=model_dirs[key], use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
            max_seqs_in_block_table=128, max_blocks_per_seq=32, max_batch_size=128, max_tokens_in_batch=4096,
            **dict(opts, use_hip_graph=graph)))
        self.model.load_weights()
        self.model.init_kvcache_and_swap(NUM_BLOCKS)
        self.model.post_layer.logits_tap = []
        if config == "lora":
            for name, seed in (("a", 1), ("b", 2)):
                sd, acfg = _random_adapter(self.cfg, 8, seed, self.dtype)
                self.model.load_lora(name, state_dict=sd, config=acfg)
        self.split_seen = {}            # scenario -> some decode step of it ran flash decoding split (num_seq_blocks > 1)

    def scenarios(self) -> list:
        names = [f"decode_b{b}" for b in DECODE_BATCHES] + ["decode_b1_long"]
        if self.graph:
            return names
        names += ["prefill", "piggyback", "chunked", "ignore_kvcache"]
        if self.model.max_draft_tokens > 0:
            names.append("verify")
        if self.config == "lora":
            names.append("lora_mixed")
        return names

    def run(self, scenario: str):
        model, vocab = self.model, self.cfg["vocab_size"]
        tap = model.post_layer.logits_tap
        del tap[:]
        tokens, used = [], []
        make_state = model._make_infer_state

        def watched(*a, **kw):          # (only to report that the long-prompt cell really splits its flash decoding)
            st = make_state(*a, **kw)
            if st.num_prefill_seqs == 0 and st.num_seq_blocks > 1:
                self.split_seen[scenario] = True
            return st
        model._make_infer_state = watched

        def forward(ids, seqs, dec, **kw):
            rec.begin()
            used.extend(s for s in seqs if s not in used)
            tokens.append(model.forward(ids, seqs, dec, **kw))
            return tokens[-1]

        def decode(prompt_lens, steps=2, **kw):
            seqs, lens = list(range(len(prompt_lens))), list(prompt_lens)
            last = forward(_prompts(lens, vocab, 7), seqs, [], **kw)
            for _ in range(steps):
                lens = [n + 1 for n in lens]
                last = forward([[t] for t in last], seqs, list(lens), **kw)

        with Recorder() as rec:
            try:
                if scenario == "decode_b1_long":
                    decode([300])
                elif scenario.startswith("decode_b"):
                    decode([3 + (7 * i) % 29 for i in range(int(scenario[len("decode_b"):]))])
                elif scenario == "prefill":
                    forward(_prompts([5, 19, 33], vocab, 8), [0, 1, 2], [])
                elif scenario == "piggyback":
                    first = forward(_prompts([9, 16, 40], vocab, 9), [0, 1, 2], [])
                    forward(_prompts([21, 4], vocab, 10) + [[t] for t in first], [3, 4, 0, 1, 2], [10, 17, 41])
                elif scenario == "chunked":
                    prompt = _prompts([80], vocab, 11)[0]
                    forward([prompt[:48]], [0], [], prefill_ctx_lens=[0])
                    forward([prompt[48:]], [0], [], prefill_ctx_lens=[48])
                elif scenario == "ignore_kvcache":
                    forward(_prompts([12, 31], vocab, 12), [0, 1], [], ignore_kvcache=True)
                    del used[:]
                elif scenario == "verify":
                    last = forward(_prompts([20, 9], vocab, 13), [0, 1], [])
                    drafts = min(3, model.max_draft_tokens)
                    rec.begin()
                    out = model.forward_verify([[last[0]] + list(range(1, 1 + drafts)), [last[1], 5]], [0, 1], [20, 9])
                    tokens.append([t for row in out for t in row])
                elif scenario == "lora_mixed":
                    decode([11, 18], lora=["a", None])
                else:
                    raise KeyError(scenario)
            finally:
                model._make_infer_state = make_state
                if used:
                    model.free_seqs_resources(used)
        torch.cuda.synchronize()
        return rec.steps, tokens, [t.clone() for t in tap]

    def close(self):
        if self._route_tune is None:
            os.environ.pop("SWIFTLLM_ROUTE_TUNE", None)
        else:
            os.environ["SWIFTLLM_ROUTE_TUNE"] = self._route_tune
        del self.model
        torch.cuda.empty_cache()


def encode(cells: dict) -> dict:
    """{config: {scenario: launches per forward}} -> the fixture (every distinct launch stored once)."""
    index, calls, out = {}, [], {}
    for config, scenarios in cells.items():
        out[config] = {}
        for scenario, steps in scenarios.items():
            enc = []
            for step in steps:
                row = []
                for call in step:
                    key = tuple(call)
                    if key not in index:
                        index[key] = len(calls)
                        calls.append(list(call))
                    row.append(index[key])
                enc.append(row)
            out[config][scenario] = enc
    return dict(calls=calls, cells=out)


def decode_fixture(fixture: dict) -> dict:
    calls = fixture["calls"]
    return {config: {scenario: [[calls[i] for i in step] for step in steps] for scenario, steps in scenarios.items()}
            for config, scenarios in fixture["cells"].items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the fixture here")
    ap.add_argument("--bits", help="directory for one <config>.pt per configuration: tokens + tapped logits of every cell")
    ap.add_argument("--configs", default=None, help="comma-separated subset (default: all; --bits adds the hipGraph one)")
    a = ap.parse_args()
    configs = a.configs.split(",") if a.configs else list(CONFIGS) + ([GRAPH_CONFIG] if a.bits else [])
    model_dirs, traces = {}, {}
    for config in configs:
        cells = Cells(config, model_dirs)
        traces[config], bits = {}, {}
        for scenario in cells.scenarios():
            steps, tokens, logits = cells.run(scenario)
            traces[config][scenario] = steps
            bits[scenario] = dict(tokens=tokens, logits=[t.cpu() for t in logits])
        if config in ("bf16", "no_rows_decode") and not cells.split_seen.get("decode_b1_long"):
            raise SystemExit(f"{config}: the 300-token cell did not split its flash decoding")
        if a.bits:
            os.makedirs(a.bits, exist_ok=True)
            torch.save(bits, os.path.join(a.bits, config + ".pt"))
        print(f"[traces] {config}: {len(traces[config])} cells, {sum(len(s) for c in traces[config].values() for s in c)} launches",
              flush=True)
        cells.close()
    for path in model_dirs.values():
        shutil.rmtree(path, ignore_errors=True)
    traces.pop(GRAPH_CONFIG, None)
    seen = {call[0] for scenarios in traces.values() for steps in scenarios.values() for step in steps for call in step}
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(encode(traces), f, separators=(",", ":"))
        print(f"[traces] wrote {a.out}: {os.path.getsize(a.out)} bytes")
        missing = missing_names(seen)
        if missing:
            raise SystemExit(f"no cell launches {missing}: add the cell that reaches it")


if __name__ == "__main__":
    main()
