"""Qwen3, Qwen2 / Qwen2.5 and Mistral checkpoints through LlamaModel / Engine against HuggingFace's fp32 eager forward,
teacher-forced with our own tokens.

Checkpoints: tests/_families_ref.make_hf_checkpoint — seeded, every parameter rounded to the tested 16-bit dtype first,
written by HF's save_pretrained, loaded with use_dummy=False. Run: four prompts of 5, 16, 17 and 48 tokens in one prefill,
then 12 decode steps; our logits come from post_layer.logits_tap; HF runs once over prompt + our output and is read at the
same 52 positions.

Gate: d_ours = max |ours - HF32| <= 1.5 d_hf16, d_hf16 = max |HF in the same 16-bit dtype - HF32| at the same positions,
computed here on the CPU — the reference implementation at our precision, not our code. Tokens: our greedy id is HF32's
argmax wherever HF32's top-2 gap exceeds 3 d_hf16 (twice the allowed distance); the share of positions that leaves out is
asserted from HF's numbers alone, before ours are looked at: at most 15 % in float16 and 50 % in bfloat16.

Variants on the first qwen3 config (head_dim 128, q_size 512 != hidden 256). Logits are compared where the variant is a
property of the model step (fused against unfused qkv: the gate, both; hipGraph replay against eager launches: equal bits).
The engine's options — chunked prefill, prompt-lookup speculation, prefix caching — are compared on what they deliver: the
token streams, equal to those of plain greedy decoding."""
import asyncio
import copy
import os

import pytest
import torch

import _lora as L
from _families_ref import FAMILY_CONFIGS, hf_logits, make_hf_checkpoint

pytestmark = pytest.mark.gpu

PROMPT_LENS = (5, 16, 17, 48)
STEPS = 12
TORCH_DTYPE = {"float16": torch.float16, "bfloat16": torch.bfloat16}
LEFT_OUT_CAP = {"float16": 0.15, "bfloat16": 0.50}
SEED = {"qwen3_d128": 1, "qwen3_d64_tied": 2, "qwen2": 5, "mistral": 4,     # (HF stays within the caps: module docstring)
        "qwen3_4b_layer": 2, "qwen3_wide_vocab": 35}   # (151936 near-equal logits: most seeds leave > 50 % open in bfloat16)
# Two further cases, by overrides of the first qwen3 config: one layer at Qwen3-4B's real width — the only end-to-end run
# where q_size (4096) != hidden at real width and hidden % 1024 != 0 (no deferred norm, uneven down-projection splits) —
# and a Qwen vocabulary, 151936 columns: wider than the rows the sampling and logprob kernels keep in registers.
CASES = {"qwen3_4b_layer": ("qwen3_d128", dict(hidden_size=2560, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
                                               intermediate_size=9728, num_hidden_layers=1)),
         "qwen3_wide_vocab": ("qwen3_d128", dict(vocab_size=151936))}


def _engine_config(path, **kw):
    from swiftllm_amd import EngineConfig
    base = dict(model_path=path, use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                max_seqs_in_block_table=16, max_blocks_per_seq=16, max_batch_size=8, max_tokens_in_batch=256)
    base.update(kw)
    return EngineConfig(**base)


def _load(path, dtype, num_blocks=48, **kw):
    from swiftllm_amd import LlamaModel
    model = LlamaModel(_engine_config(path, dtype=dtype, **kw))
    model.load_weights()
    model.init_kvcache_and_swap(num_blocks)
    model.post_layer.logits_tap = []
    return model


def _prompts(seed=0, vocab=512):
    g = torch.Generator().manual_seed(100 + seed)
    return [torch.randint(3, vocab, (n,), generator=g).tolist() for n in PROMPT_LENS]


def _generate(model, prompts, steps=STEPS, seq_ids=None, **kw):
    """One prefill of all prompts, then `steps` decode steps. Returns the streams (steps + 1 tokens per prompt) and the
    tapped logits [steps + 1, prompts, vocab] (fp32, CPU)."""
    ids = seq_ids or list(range(len(prompts)))
    taps = model.post_layer.logits_tap
    start = len(taps)
    out = [model.forward(prompts, ids, [], **kw)]
    lens = [len(p) for p in prompts]
    for _ in range(steps):
        lens = [n + 1 for n in lens]
        out.append(model.forward([[t] for t in out[-1]], ids, list(lens), **kw))
    logits = torch.stack([t.float().cpu() for t in taps[start:]])
    assert logits.shape[:2] == (steps + 1, len(prompts))
    return [[step[i] for step in out] for i in range(len(prompts))], logits


def _hf_at_our_positions(hf, prompts, streams, dtype):
    """HF logits [steps + 1, prompts, vocab] at the positions our logits were taken, teacher-forced with our streams."""
    rows = [p + s[:-1] for p, s in zip(prompts, streams)]
    per_seq = hf_logits(hf, rows, dtype)
    return torch.stack([lg[len(p) - 1:] for lg, p in zip(per_seq, prompts)], dim=1)


def _hold_to_hf(tag, dtype, hf, prompts, streams, logits, rows=None):
    """The gate and the token rule of the module docstring on the rows `rows` (default: all). Returns (d_ours, d_hf16)."""
    rows = list(range(len(prompts))) if rows is None else rows
    sub = lambda seq: [seq[i] for i in rows]       # noqa: E731
    hf32 = _hf_at_our_positions(hf, sub(prompts), sub(streams), torch.float32)
    hf16 = _hf_at_our_positions(hf, sub(prompts), sub(streams), TORCH_DTYPE[dtype])
    d_hf16 = (hf16 - hf32).abs().max().item()
    top2 = hf32.topk(2, dim=-1).values
    decided = (top2[..., 0] - top2[..., 1]) > 3 * d_hf16
    left_out = 1.0 - decided.float().mean().item()
    # from HF alone, before our numbers are looked at
    assert left_out <= LEFT_OUT_CAP[dtype], f"{tag}: HF leaves {left_out:.0%} of the positions undecided; pick another seed"
    ours = logits[:, rows]
    d_ours = (ours - hf32).abs().max().item()
    print(f"\n[{tag} {dtype}] d_ours {d_ours:.3e}  d_hf16 {d_hf16:.3e}  ratio {d_ours / d_hf16:.2f}  "
          f"positions {decided.numel()}  left out {left_out:.0%}")
    assert d_ours <= 1.5 * d_hf16, (tag, d_ours, d_hf16)
    got = torch.tensor(sub(streams)).t()
    assert torch.equal(got[decided], hf32.argmax(-1)[decided]), f"{tag}: a decided token differs from HF32's argmax"
    return d_ours, d_hf16


_CACHE = {}


@pytest.fixture
def family(tmp_path_factory):
    """(path, HF fp32 model, prompts, base streams, base logits) of a family and dtype: built and run once per module."""
    def get(name, dtype):
        key = (name, dtype)
        if key not in _CACHE:
            path = str(tmp_path_factory.mktemp(f"{name}_{dtype}"))
            base, overrides = CASES.get(name, (name, {}))
            hf = make_hf_checkpoint(path, base, TORCH_DTYPE[dtype], SEED[name], **overrides)
            prompts = _prompts(SEED[name], hf.config.vocab_size)      # (drawn from the whole vocabulary)
            model = _load(path, dtype)
            streams, logits = _generate(model, prompts)
            plain = model.plain_qkv
            model.free_seqs_resources(list(range(len(prompts))))
            del model
            _CACHE[key] = (path, hf, prompts, streams, logits, plain)
        return _CACHE[key]
    return get


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(FAMILY_CONFIGS) + list(CASES))
def test_family_matches_hf(family, name, dtype):
    path, hf, prompts, streams, logits, plain = family(name, dtype)
    assert plain is True        # every config here has a bias, a QK-norm or q_size != hidden
    assert logits.shape == (STEPS + 1, 4, 151936 if name == "qwen3_wide_vocab" else 512)
    _hold_to_hf(name, dtype, hf, prompts, streams, logits)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_wide_vocabulary_rows_are_sampled_and_scored_as_the_references_say(family, dtype):
    """Eight seeded sampling steps with logprobs on the 151936-column model: every token is the numpy reference's draw from
    the tapped logits of its step wherever that draw is decided (margin > 1e-3, nucleus equal at p +- 1e-4: the rule of
    tests/test_gpu_sampling.py), and the logprobs meet the bound of tests/test_gpu_logprobs.py (checked by its `_run`)."""
    from swiftllm_amd import SamplingParams
    from test_gpu_logprobs import _run
    from test_gpu_sampling import _rows
    path, _, prompts, _, _, _ = family("qwen3_wide_vocab", dtype)
    prompts = prompts[:2]
    model = _load(path, dtype)
    sps = [SamplingParams(0.9, top_k=40, top_p=0.9, seed=900 + r, logprobs=5) for r in range(len(prompts))]
    toks, logits, scores = _run(model, prompts, lambda k: sps, steps=7)
    assert len(toks) == 8 and all(s is not None and len(s[0].top) == 5 for s in scores)
    decided = 0
    for k in range(8):
        assert logits[k].shape == (len(prompts), 151936)
        ref = _rows(logits[k].cpu(), sps, [len(p) + k for p in prompts], 0.9)
        for r, (tok, ok) in enumerate(ref):
            if ok:
                decided += 1
                assert toks[k][r] == tok, (k, r, toks[k][r], tok)
    print(f"\n[qwen3_wide_vocab {dtype}] sampled rows decided by the reference: {decided} of {8 * len(prompts)}; "
          f"tokens past column 131072: {sum(t >= 131072 for step in toks for t in step)}")
    assert decided >= 8, decided


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_unfused_qkv_is_held_to_the_same_gate(family, dtype):
    path, hf, prompts, _, _, _ = family("qwen3_d128", dtype)
    model = _load(path, dtype, fuse_qkv=False)
    assert model.weight.layers[0].qkv_proj is None
    streams, logits = _generate(model, prompts)
    _hold_to_hf("qwen3_d128 unfused qkv", dtype, hf, prompts, streams, logits)
    # ... and so is the biased family, whose three biases are then three tensors
    path, hf, prompts, _, _, _ = family("qwen2", dtype)
    model = _load(path, dtype, fuse_qkv=False)
    assert model.weight.layers[0].qkv_bias is None and model.weight.layers[0].q_bias is not None
    streams, logits = _generate(model, prompts)
    _hold_to_hf("qwen2 unfused qkv", dtype, hf, prompts, streams, logits)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_eager_launches_give_the_bits_of_graph_replay(family, dtype):
    path, _, prompts, base_streams, base_logits, _ = family("qwen3_d128", dtype)
    model = _load(path, dtype, use_hip_graph=False)
    streams, logits = _generate(model, prompts)
    assert streams == base_streams
    assert torch.equal(logits, base_logits)
    assert model.replay.captures == 0


def _serve(model, waves, output_len):
    """Serve the waves of prompts one after another through one Engine; returns it and (error, tokens) per request."""
    from swiftllm_amd import Engine, RawRequest

    async def serve():
        eng = Engine(model.engine_config, model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        out = []
        for prompts in waves:
            jobs = [asyncio.ensure_future(eng.add_request_and_wait(RawRequest("", output_len, p))) for p in prompts]
            done = await asyncio.wait_for(asyncio.gather(*jobs), timeout=120)
            out.append([(r.error, toks) for r, toks in done])
        loops.cancel()
        return eng, out
    return asyncio.run(serve())


def test_engine_streams_equal_direct_forward_calls(family):
    path, _, prompts, base_streams, _, _ = family("qwen3_d128", "bfloat16")
    model = _load(path, "bfloat16")
    eng, (got,) = _serve(model, [prompts[:3]], STEPS + 1)
    for i, (err, toks) in enumerate(got):
        assert err is None and toks == base_streams[i], i
    assert model.gpu_block_manager.num_free_blocks == 48


@pytest.mark.parametrize("option", [dict(max_prefill_chunk=16), dict(speculative_ngram=3),
                                    dict(max_prefill_chunk=32, enable_prefix_caching=True, prefix_cache_max_seqs=4)],
                         ids=["chunked_prefill", "speculation", "prefix_cache"])
def test_engine_options_deliver_the_plain_greedy_streams(family, option):
    dtype = "float16"
    path, _, prompts, base_streams, _, _ = family("qwen3_d128", dtype)
    model = _load(path, dtype, **option)
    # (prefix caching: the 48-token prompt comes again — its whole blocks below the last token are a hit, copied)
    eng, (got, again) = _serve(model, [prompts, prompts[3:]], STEPS + 1)
    for i, (err, toks) in enumerate(got):
        assert err is None and toks == base_streams[i], (option, i)
    assert again == [(None, base_streams[3])]
    if option.get("enable_prefix_caching"):
        assert eng.num_prefix_hits >= 1 and eng.num_prefix_hit_tokens >= 32
    if "speculative_ngram" in option:
        assert eng.speculative_k == 3
        # the verify step itself, whatever the prompt lookup proposed above: three right drafts per sequence are accepted
        ids = [8, 9, 10, 11]
        first = model.forward(prompts, ids, [])
        assert first == [s[0] for s in base_streams]
        out = model.forward_verify([s[:4] for s in base_streams], ids, [len(p) for p in prompts])
        assert [o[:4] for o in out] == [s[1:5] for s in base_streams]


def test_fp8_pools_hold_the_codes_of_the_16_bit_rows(family):
    """Layer 0 sees identical inputs in both runs: after the prefill its K and V codes are the quantised 16-bit rows."""
    dtype = "float16"
    path, _, prompts, _, _, _ = family("qwen3_d128", dtype)
    pools = {}
    for kv in ("auto", "fp8_e4m3"):
        model = _load(path, dtype, kv_cache_dtype=kv)
        model.forward(prompts, [0, 1, 2, 3], [])
        torch.cuda.synchronize()
        table = model.gpu_block_manager.block_table.cpu()
        rows = {}
        for s, p in enumerate(prompts):
            blocks = table[s, :(len(p) + 15) // 16].long()
            for name, pool in (("k", model.k_cache), ("v", model.v_cache)):
                x = pool[blocks.to(pool.device), 0]                             # [blocks, KVH, 16, D] of layer 0
                rows[name, s] = x.permute(1, 0, 2, 3).reshape(x.shape[1], -1, x.shape[3])[:, :len(p)].cpu()
        pools[kv] = rows
        scale = None if model.kv_scales is None else model.kv_scales.cpu()
        # the FP8 run decodes on: the quantising decode store and the FP8 attention serve the family too
        if kv == "fp8_e4m3":
            assert model.k_cache.dtype == torch.float8_e4m3fn
            toks = model.forward(prompts, [4, 5, 6, 7], [])
            model.forward([[t] for t in toks], [4, 5, 6, 7], [len(p) + 1 for p in prompts])
    assert scale is not None and bool((scale == 1).all())
    for key, x16 in pools["auto"].items():
        want = x16.float().mul(1.0).clamp(-448, 448).to(torch.float8_e4m3fn)
        assert torch.equal(pools["fp8_e4m3"][key].view(torch.uint8), want.view(torch.uint8)), key


def test_lora_rows_match_hf_with_the_adapter_merged(family):
    """One rank-8 adapter on q_proj and v_proj: the rows that name it are held to HF32 with W + scale B A merged in fp32
    under the same gate; the rows without an adapter are bit-equal to the base run."""
    dtype = "float16"
    path, hf, prompts, base_streams, base_logits, _ = family("qwen3_d128", dtype)
    raw = hf.config
    D, H, KVH, hidden = raw.head_dim, raw.num_attention_heads, raw.num_key_value_heads, raw.hidden_size
    shapes = dict(q_proj=(H * D, hidden), v_proj=(KVH * D, hidden))
    rank, alpha = 8, 16
    g = torch.Generator().manual_seed(9)
    adapter = {}
    for layer in range(raw.num_hidden_layers):
        for m, (n, k) in shapes.items():
            adapter[L.peft_key(layer, m, "A")] = (torch.randn(rank, k, generator=g) * 0.05).to(torch.float16)
            adapter[L.peft_key(layer, m, "B")] = (torch.randn(n, rank, generator=g) * 0.05).to(torch.float16)
    config = L.adapter_config(rank, alpha, modules=("q_proj", "v_proj"))
    merged = copy.deepcopy(hf)
    sd = merged.state_dict()
    with torch.no_grad():
        for layer in range(raw.num_hidden_layers):
            for m in shapes:
                a, b = adapter[L.peft_key(layer, m, "A")].float(), adapter[L.peft_key(layer, m, "B")].float()
                sd[L.weight_key(layer, m)].add_((alpha / rank) * (b @ a))
    model = _load(path, dtype, max_loras=2, max_lora_rank=8)
    model.load_lora("ad", state_dict=adapter, config=config)
    names = ["ad", None, "ad", None]
    streams, logits = _generate(model, prompts, lora=names)
    for i in (1, 3):
        assert streams[i] == base_streams[i]
        assert torch.equal(logits[:, i], base_logits[:, i]), f"row {i} names no adapter and moved"
    assert streams[0] != base_streams[0] or not torch.equal(logits[:, 0], base_logits[:, 0])    # the adapter acts
    _hold_to_hf("qwen3_d128 lora rows", dtype, merged, prompts, streams, logits, rows=[0, 2])


def test_a_sliding_window_caps_the_context(tmp_path):
    from swiftllm_amd import Engine, RawRequest
    path = str(tmp_path)
    make_hf_checkpoint(path, "mistral", torch.float16, 4, sliding_window=64)
    model = _load(path, "float16")
    assert model.model_config.max_position_embeddings == 64 == model.model_config.sliding_window
    assert model._cos_cached.shape[0] == 64
    prompt = _prompts(4)[3]     # 48 tokens

    async def serve():
        eng = Engine(model.engine_config, model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        jobs = [asyncio.ensure_future(eng.add_request_and_wait(RawRequest("", n, prompt))) for n in (16, 17)]
        done = await asyncio.wait_for(asyncio.gather(*jobs), timeout=120)
        loops.cancel()
        return [(r.error, toks) for r, toks in done]
    (ok_err, ok_toks), (bad_err, _) = asyncio.run(serve())
    assert ok_err is None and len(ok_toks) == 16                # 64 tokens: inside the window
    assert bad_err is not None and "64 rotary positions" in str(bad_err)        # 65: the engine's existing refusal


def test_the_decode_engine_is_refused_at_construction(family):
    from swiftllm_amd import LlamaModel
    path = family("qwen3_d128", "bfloat16")[0]
    with pytest.raises(ValueError, match="decode_engine"):
        LlamaModel(_engine_config(path, dtype="bfloat16", tuning=dict(decode_engine=True)))
    assert os.path.exists(os.path.join(path, "config.json"))
