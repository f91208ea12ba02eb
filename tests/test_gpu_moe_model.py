"""Qwen3-MoE and Mixtral checkpoints through LlamaModel / Engine against the routing-forced reference of tests/_moe_ref.py.

Checkpoints: tests/_moe_ref.make_moe_checkpoint — seeded, every parameter rounded to the tested 16-bit dtype first, written by
HF's save_pretrained (per-expert tensor names), loaded with use_dummy=False. Run: the prompts of
tests/test_gpu_model_families.py (5, 16, 17 and 48 tokens in one prefill, then 12 decode steps) with post_layer.logits_tap
and model.moe_tap on (a tapped step runs eager).

A free 16-bit forward flips experts on near-ties, and a flip is a discontinuity that contaminates every later position
through the KV. So the reference is HF's eager forward FORCED to our tapped expert ids (its weights recomputed from its own
router logits over that set), and the routing decision is checked on its own:

  Logits.  d_ours = max |ours - forced-ref fp32| <= 1.5 d_ref16, d_ref16 = max |forced-ref in the 16-bit dtype - forced-ref
           fp32| at the same positions: the reference at our precision is the yardstick, never our own code.
  Routing. At every (layer, position) — prompt positions included — where the forced fp32 reference's own k-th gap in
           router logits exceeds 3 router_err, our tapped expert set equals its free top-k; router_err = max |router logits
           of forced-ref 16-bit - forced-ref fp32|. The share this leaves out is asserted from the reference alone: at most
           10 % in float16, 35 % in bfloat16.
  Tokens.  Our greedy id is the forced fp32 reference's argmax wherever its top-2 gap exceeds 3 d_ref16; left-out caps 15 % /
           50 % as in the families test.

Variants on the qwen3_moe checkpoint: hipGraph replay against eager launches (equal bits); chunked prefill, prompt-lookup
speculation and prefix caching through the Engine (token streams equal to plain greedy decoding); an FP8 KV pool — held to
"serves without error, and two runs give equal streams" (a forced reference fed the same quantised K/V is not built here);
one seeded sampling request with logprobs=2. Refusals at load: decode_engine, max_loras > 0, qwen2_moe."""
import json
import os

import pytest
import torch

import _moe_ref as R
from test_gpu_model_families import (LEFT_OUT_CAP, STEPS, TORCH_DTYPE, _engine_config, _generate, _prompts, _serve)

pytestmark = pytest.mark.gpu

KINDS = ("qwen3_moe", "mixtral")
SEED = {"qwen3_moe": 6, "mixtral": 1}       # (the reference stays within the caps at these: checked on the CPU over seeds 1, 2, 4, 6)
ROUTE_LEFT_OUT_CAP = {"float16": 0.10, "bfloat16": 0.35}


def _load(path, dtype, num_blocks=48, **kw):
    from swiftllm_amd import LlamaModel
    model = LlamaModel(_engine_config(path, dtype=dtype, **kw))
    model.load_weights()
    model.init_kvcache_and_swap(num_blocks)
    model.post_layer.logits_tap = []
    return model


def _tapped_ids(tap, prompts, num_layers, k):
    """moe_tap entries of one prefill + STEPS decode steps -> per prompt, per layer, the expert ids [len + STEPS, k] and
    weights at the positions of prompt + stream[:-1]."""
    assert len(tap) == (STEPS + 1) * num_layers, len(tap)
    assert [e[0] for e in tap] == list(range(num_layers)) * (STEPS + 1)
    total = sum(len(p) for p in prompts)
    starts = [sum(len(p) for p in prompts[:i]) for i in range(len(prompts))]
    ids = [[None] * num_layers for _ in prompts]
    ws = [[None] * num_layers for _ in prompts]
    for layer in range(num_layers):
        pre_ids, pre_w = tap[layer][1], tap[layer][2]
        assert tuple(pre_ids.shape) == (total, k) and pre_ids.dtype == torch.int32 and pre_w.dtype == torch.float32
        steps = [tap[s * num_layers + layer] for s in range(1, STEPS + 1)]
        assert all(tuple(e[1].shape) == (len(prompts), k) for e in steps)
        for i, p in enumerate(prompts):
            ids[i][layer] = torch.cat([pre_ids[starts[i]:starts[i] + len(p)]] + [e[1][i:i + 1] for e in steps]).long()
            ws[i][layer] = torch.cat([pre_w[starts[i]:starts[i] + len(p)]] + [e[2][i:i + 1] for e in steps])
    return ids, ws


_CACHE = {}


@pytest.fixture
def moe(tmp_path_factory):
    """(path, HF fp32 model, prompts, streams, logits, tapped ids, tapped weights) of a kind and dtype: once per module."""
    def get(kind, dtype):
        key = (kind, dtype)
        if key not in _CACHE:
            path = str(tmp_path_factory.mktemp(f"{kind}_{dtype}"))
            hf = R.make_moe_checkpoint(path, kind, TORCH_DTYPE[dtype], SEED[kind])
            prompts = _prompts(SEED[kind], hf.config.vocab_size)
            model = _load(path, dtype)
            assert model.model_config.is_moe and all(layer.moe for layer in model.transformer_layers)
            assert model.moe_tap is None
            model.moe_tap = []
            streams, logits = _generate(model, prompts)
            assert model.replay.captures == 0                 # a tapped step is never captured
            cfg = model.model_config
            ids, ws = _tapped_ids(model.moe_tap, prompts, cfg.num_layers, cfg.num_experts_per_tok)
            model.moe_tap = None
            assert all(layer.moe_tap is None for layer in model.transformer_layers)
            model.free_seqs_resources(list(range(len(prompts))))
            del model
            _CACHE[key] = (path, hf, prompts, streams, logits, ids, ws)
        return _CACHE[key]
    return get


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("kind", KINDS)
def test_moe_model_matches_the_forced_reference(moe, kind, dtype):
    path, hf, prompts, streams, logits, ids, ws = moe(kind, dtype)
    k, E = hf.config.num_experts_per_tok, R.routers(hf)[0].num_experts
    assert logits.shape == (STEPS + 1, 4, 512)
    rows = [p + s[:-1] for p, s in zip(prompts, streams)]
    for per_layer, w_layer in zip(ids, ws):
        for t, w in zip(per_layer, w_layer):
            assert bool(((t >= 0) & (t < E)).all()) and bool((t[:, 0] != t[:, 1]).all())
            assert bool((w[:, 0] >= w[:, 1]).all()) and float((w.sum(1) - 1).abs().max()) < 1e-6     # both renormalise
    ref32 = R.forced_logits(hf, rows, torch.float32, ids)
    ref16 = R.forced_logits(hf, rows, TORCH_DTYPE[dtype], ids)
    at = lambda ref: torch.stack([r[0][len(p) - 1:] for r, p in zip(ref, prompts)], dim=1)     # noqa: E731
    lg32, lg16 = at(ref32), at(ref16)
    assert lg32.shape == logits.shape

    # routing: what the reference alone decides, then our ids
    router_err = max(float((a[1] - b[1]).abs().max()) for a, b in zip(ref16, ref32))
    decided = [R.kth_gap(r[1], k) > 3 * router_err for r in ref32]            # per row: [layers, positions]
    n_all = sum(d.numel() for d in decided)
    left_out = 1.0 - sum(int(d.sum()) for d in decided) / n_all
    assert left_out <= ROUTE_LEFT_OUT_CAP[dtype], f"{kind}: the reference leaves {left_out:.0%} of the routings undecided; pick another seed"
    wrong = 0
    for r, d, per_layer in zip(ref32, decided, ids):
        ours = torch.stack(per_layer).sort(dim=-1).values
        free = r[2].sort(dim=-1).values
        wrong += int(((ours != free).any(-1) & d).sum())
    flips = sum(int((torch.stack(per_layer).sort(-1).values != r[2].sort(-1).values).any(-1).sum())
                for r, per_layer in zip(ref32, ids))

    # logits and tokens
    d_ref16 = (lg16 - lg32).abs().max().item()
    top2 = lg32.topk(2, dim=-1).values
    tok_decided = (top2[..., 0] - top2[..., 1]) > 3 * d_ref16
    tok_left_out = 1.0 - tok_decided.float().mean().item()
    assert tok_left_out <= LEFT_OUT_CAP[dtype], f"{kind}: the reference leaves {tok_left_out:.0%} of the positions undecided"
    d_ours = (logits - lg32).abs().max().item()
    print(f"\n[{kind} {dtype}] d_ours {d_ours:.3e}  d_ref16 {d_ref16:.3e}  ratio {d_ours / d_ref16:.2f}  router_err "
          f"{router_err:.3e}  routings {n_all}  left out {left_out:.1%}  ours != fp32's free choice at {flips} (decided: {wrong})  "
          f"tokens left out {tok_left_out:.0%}")
    assert wrong == 0, f"{kind}: {wrong} decided routings differ from the reference's free top-k"
    assert d_ours <= 1.5 * d_ref16, (kind, d_ours, d_ref16)
    got = torch.tensor(streams).t()
    assert torch.equal(got[tok_decided], lg32.argmax(-1)[tok_decided]), f"{kind}: a decided token differs from the reference's argmax"


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_graph_replay_gives_the_bits_of_eager_launches(moe, dtype):
    path, _, prompts, base_streams, base_logits, _, _ = moe("qwen3_moe", dtype)
    replay = _load(path, dtype)                               # use_hip_graph is on by default; no tap: decode steps replay
    streams, logits = _generate(replay, prompts)
    assert replay.replay.captures >= 1
    assert streams == base_streams and torch.equal(logits, base_logits)     # ... the tapped (eager) base run included
    del replay
    eager = _load(path, dtype, use_hip_graph=False)
    streams, logits = _generate(eager, prompts)
    assert eager.replay.captures == 0
    assert streams == base_streams and torch.equal(logits, base_logits)


@pytest.mark.parametrize("option", [dict(max_prefill_chunk=16), dict(speculative_ngram=3),
                                    dict(max_prefill_chunk=32, enable_prefix_caching=True, prefix_cache_max_seqs=4)],
                         ids=["chunked_prefill", "speculation", "prefix_cache"])
def test_engine_options_deliver_the_plain_greedy_streams(moe, option):
    dtype = "float16"
    path, _, prompts, base_streams, _, _, _ = moe("qwen3_moe", dtype)
    model = _load(path, dtype, **option)
    eng, (got, again) = _serve(model, [prompts, prompts[3:]], STEPS + 1)
    for i, (err, toks) in enumerate(got):
        assert err is None and toks == base_streams[i], (option, i)
    assert again == [(None, base_streams[3])]
    if option.get("enable_prefix_caching"):
        assert eng.num_prefix_hits >= 1 and eng.num_prefix_hit_tokens >= 32
    if "speculative_ngram" in option:
        ids = [8, 9, 10, 11]
        first = model.forward(prompts, ids, [])
        assert first == [s[0] for s in base_streams]
        out = model.forward_verify([s[:4] for s in base_streams], ids, [len(p) for p in prompts])
        assert [o[:4] for o in out] == [s[1:5] for s in base_streams]


def test_an_fp8_kv_pool_serves_and_repeats_itself(moe):
    """Held to: serves without error, two runs give equal streams and equal logits (module docstring)."""
    dtype = "bfloat16"
    path, _, prompts, base_streams, _, _, _ = moe("qwen3_moe", dtype)
    runs = []
    for _ in range(2):
        model = _load(path, dtype, kv_cache_dtype="fp8_e4m3")
        assert model.k_cache.dtype == torch.float8_e4m3fn
        runs.append(_generate(model, prompts))
        del model
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert all(len(s) == STEPS + 1 for s in runs[0][0]) and bool(torch.isfinite(runs[0][1]).all())
    assert [s[0] for s in runs[0][0]] == [s[0] for s in base_streams]       # the prefill attends to fresh K/V: no FP8 yet


def test_a_seeded_sampling_request_with_logprobs_completes(moe):
    from swiftllm_amd import Engine, RawRequest, SamplingParams
    import asyncio
    path, _, prompts, _, _, _, _ = moe("qwen3_moe", "bfloat16")
    model = _load(path, "bfloat16")

    async def serve():
        eng = Engine(model.engine_config, model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        sp = SamplingParams(0.8, top_k=20, top_p=0.9, seed=77, logprobs=2)
        out = []
        for _ in range(2):
            req, toks = await asyncio.wait_for(eng.add_request_and_wait(RawRequest("", 8, prompts[1], sampling_params=sp)), 120)
            out.append((req.error, toks))
        loops.cancel()
        return out
    (err, toks), (err2, toks2) = asyncio.run(serve())
    assert err is None and err2 is None and len(toks) == 8 and toks == toks2          # seeded: the same draw twice


def test_refusals_at_load(moe, tmp_path):
    from swiftllm_amd import LlamaModel
    path = moe("qwen3_moe", "bfloat16")[0]
    with pytest.raises(ValueError, match="decode_engine"):
        LlamaModel(_engine_config(path, dtype="bfloat16", tuning=dict(decode_engine=True)))
    with pytest.raises(ValueError, match="max_loras"):
        LlamaModel(_engine_config(path, dtype="bfloat16", max_loras=2, max_lora_rank=8))
    cfg = json.load(open(os.path.join(path, "config.json")))
    cfg["model_type"] = "qwen2_moe"
    with open(os.path.join(str(tmp_path), "config.json"), "w") as f:
        json.dump(cfg, f)
    with pytest.raises(ValueError, match="shared expert"):
        LlamaModel(_engine_config(str(tmp_path), dtype="bfloat16"))
