"""Prefix caching by KV block copy on the GPU: LlamaModel.copy_kv_prefix (bit-exactness, what it may touch, its host
refusals) and the Engine with the option on, on the decisive checkpoint (oracle/synth.py: the greedy stream is a closed
form of the prompt — the token after position p is perm[token(p - OFFSET)], so an output depends on the K/V of a token
OFFSET + 1 positions back: the prompts here end less than OFFSET + 1 tokens behind the copied blocks, so that their first
outputs read copied K/V)."""
import asyncio
import random

import pytest
import torch

import _churn
from oracle import synth

pytestmark = pytest.mark.gpu
OFFSET, STEPS, BLOCK = _churn.OFFSET, 26, 16
CASES = [("float16", "auto"), ("bfloat16", "auto"), ("bfloat16", "fp8_e4m3")]


def _model(tmp_path, dtype, num_blocks=40, **kw):
    """(model, perm) on the decisive checkpoint at the geometry of tests/test_gpu_chunked_prefill.py."""
    from swiftllm_amd import EngineConfig, LlamaModel
    cfg, sd, perm = _churn.decisive(dtype)
    synth.write_model_dir(str(tmp_path), cfg, sd)
    base = dict(model_path=str(tmp_path), use_dummy=False, block_size=BLOCK, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                max_seqs_in_block_table=8, max_blocks_per_seq=16, max_batch_size=4, max_tokens_in_batch=1024, dtype=dtype)
    base.update(kw)
    model = LlamaModel(EngineConfig(**base))
    model.load_weights()
    model.init_kvcache_and_swap(num_blocks)
    return model, perm


def _prompt(n, seed, vocab):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, vocab, (n,), generator=g).tolist()


def _bytes(t):
    return t.view(torch.uint8).reshape(t.shape[0], -1)


@pytest.mark.parametrize("dtype,kv", CASES)
def test_copy_kv_prefix_is_bit_exact_and_touches_nothing_else(tmp_path, dtype, kv):
    """Row 0 prefills p[:64] and then p[64:] behind it; row 1 gets the 64 tokens by copy and runs the same second forward:
    the same kernels on the same shapes and inputs, only the block ids differ — the logits must be bit-equal. Row 1's four
    blocks equal row 0's byte for byte (a block holds every layer of both pools' slices), no other block of either pool
    changes across the copy, and row 1 decodes on after row 0 was freed and its blocks were overwritten."""
    model, perm = _model(tmp_path, dtype, kv_cache_dtype=kv)
    model.post_layer.logits_tap = tap = []
    mgr = model.gpu_block_manager
    p = _prompt(81, 1, len(perm))
    want = [t[0] for t in synth.decisive_expected_tokens([p], perm, OFFSET, STEPS)]
    model.forward([p[:64]], [0], [])
    tok0 = model.forward([p[64:]], [0], [], prefill_ctx_lens=[64])
    logits0 = tap[-1].clone()
    free = mgr.num_free_blocks
    k_before, v_before = _bytes(model.k_cache).clone(), _bytes(model.v_cache).clone()

    model.copy_kv_prefix([0], [1], [64])
    torch.cuda.synchronize()
    b0, b1 = mgr.get_block_ids_host(0), mgr.get_block_ids_host(1)
    assert len(b0) == 6 and len(b1) == 4 and not set(b0) & set(b1) and mgr.num_free_blocks == free - 4
    rest = [b for b in range(model.num_blocks) if b not in b1]
    for now, before in ((_bytes(model.k_cache), k_before), (_bytes(model.v_cache), v_before)):
        assert torch.equal(now[b1], before[b0[:4]])
        assert before[b0[:4]].any()                              # (the prefix really holds something)
        assert torch.equal(now[rest], before[rest])
    tok1 = model.forward([p[64:]], [1], [], prefill_ctx_lens=[64])
    logits1 = tap[-1].clone()
    assert logits0.dtype == logits1.dtype and logits0.shape == logits1.shape
    assert torch.equal(logits0.view(torch.int16), logits1.view(torch.int16))
    assert tok0 == tok1
    model.post_layer.logits_tap = None

    # free the donor and scribble over its old blocks: another sequence is stored there
    model.free_seqs_resources([0])
    other = _prompt(90, 2, len(perm))
    model.forward([other], [2], [])
    assert set(b0) <= set(mgr.get_block_ids_host(2))
    got, n = [tok1[0]], len(p)
    for _ in range(STEPS):
        n += 1
        got.append(model.forward([[got[-1]]], [1], [n])[0])
    print(f"\n[copy_kv_prefix {dtype} {kv}] stream of the copied row: {sum(a == b for a, b in zip(got, want))} / {len(want)} "
          f"tokens on the closed form")
    assert got == want


def test_copy_kv_prefix_copies_several_pairs_in_one_call(tmp_path):
    """Two donors, three destinations of different lengths (one donor twice), one call; each destination continues behind
    its copied context and walks its own closed form."""
    model, perm = _model(tmp_path, "bfloat16", max_batch_size=8)
    vocab = len(perm)
    a, b = _prompt(70, 3, vocab), _prompt(50, 4, vocab)
    model.forward([a, b], [0, 1], [])
    tails = [_prompt(9, 5, vocab), _prompt(14, 6, vocab), _prompt(5, 7, vocab)]
    prompts = [a[:64] + tails[0], b[:32] + tails[1], a[:16] + tails[2]]
    want = synth.decisive_expected_tokens(prompts, perm, OFFSET, 6)
    model.copy_kv_prefix([0, 1, 0], [4, 3, 2], [64, 32, 16])
    model.free_seqs_resources([0, 1])
    rows = [4, 3, 2]
    got = [model.forward(tails, rows, [], prefill_ctx_lens=[64, 32, 16])]
    lens = [len(x) for x in prompts]
    for _ in range(6):
        lens = [n + 1 for n in lens]
        got.append(model.forward([[t] for t in got[-1]], rows, list(lens)))
    assert got == want


def test_copy_kv_prefix_host_refusals_allocate_nothing(tmp_path):
    model, perm = _model(tmp_path, "float16", num_blocks=6)
    mgr = model.gpu_block_manager
    p = _prompt(64, 1, len(perm))
    model.forward([p], [0], [])                 # 4 blocks
    model.forward([p[:16]], [2], [])            # 1 block
    free = mgr.num_free_blocks
    assert free == 1
    bad = [
        (ValueError, ([0], [1, 3], [16])),              # lists of different lengths
        (ValueError, ([0], [1], [16, 16])),
        (ValueError, ([0], [1], [0])),                  # not a positive multiple of the block size
        (ValueError, ([0], [1], [-16])),
        (ValueError, ([0], [1], [20])),
        (ValueError, ([0], [1], [80])),                 # the source owns 4 blocks
        (ValueError, ([5], [1], [16])),                 # the source owns nothing
        (ValueError, ([0], [2], [16])),                 # the destination already owns blocks
        (ValueError, ([0, 0], [1, 1], [16, 16])),       # a destination twice
        (ValueError, ([0, 2], [2, 3], [16, 16])),       # a destination that is a source
        (ValueError, ([0], [0], [16])),
        (RuntimeError, ([0], [1], [32])),               # the pool has one free block
        (RuntimeError, ([0], [8], [16])),               # a row outside the block table
    ]
    for exc, args in bad:
        with pytest.raises(exc):
            model.copy_kv_prefix(*args)
        assert mgr.num_free_blocks == free and mgr.host.num_allocated(1) == 0 and mgr.host.num_allocated(3) == 0, args
    saved = model.gpu_block_manager
    model.gpu_block_manager = None
    with pytest.raises(RuntimeError, match="no KV pool"):
        model.copy_kv_prefix([0], [1], [16])
    model.gpu_block_manager = saved
    model.copy_kv_prefix([], [], [])            # nothing to do
    assert mgr.num_free_blocks == free
    model.copy_kv_prefix([0], [1], [16])        # ... and the legal call takes its one block
    assert mgr.num_free_blocks == 0 and mgr.host.num_allocated(1) == 1


# ---- the engine ------------------------------------------------------------------------------------------------------
def _shared_prompts(vocab):
    shared = _prompt(48, 11, vocab)
    return [shared + _prompt(12 + 7 * i, 20 + i, vocab) for i in range(4)]       # 60, 67, 74, 81 tokens


def _engine(model, piggyback=True):
    from swiftllm_amd import Engine
    eng = Engine(model.engine_config, model=model, piggyback=piggyback)
    seen = []           # per forward: [(row, context, prompt tokens fed)] of its prefill sequences
    inner = model.forward

    def spy(input_ids, seq_ids, dec_lens, **kw):
        n_prefill = len(input_ids) - len(dec_lens)
        ctx = kw.get("prefill_ctx_lens") or [0] * n_prefill
        seen.append([(seq_ids[i], ctx[i], len(input_ids[i])) for i in range(n_prefill)])
        assert sum(len(x) for x in input_ids[:n_prefill]) <= 32
        return inner(input_ids, seq_ids, dec_lens, **kw)
    model.forward = spy
    return eng, seen


async def _serve(eng, reqs, max_steps=400):
    from swiftllm_amd.server import RawRequest, Request
    if not eng.initialized:
        await eng.initialize()
    eng.event_loop = asyncio.get_running_loop()
    reqs = [Request(RawRequest("", n, list(p))) for p, n in reqs]
    eng.scheduler.on_requests_arrival(reqs)
    for _ in range(max_steps):
        if all(r.is_finished() for r in reqs):
            break
        assert await eng.step()
    assert all(r.is_finished() and r.error is None for r in reqs)
    return reqs


def _fed(seen, since):
    """Per block-table row: (context of its first prompt forward, prompt tokens fed in all) over seen[since:]."""
    out = {}
    for step in seen[since:]:
        for row, ctx, n in step:
            first, total = out.get(row, (ctx, 0))
            out[row] = (first, total + n)
    return out


@pytest.mark.parametrize("piggyback,dtype", [(True, "bfloat16"), (False, "float16")])
def test_engine_serves_shared_prefixes_by_copy_and_gives_the_closed_form(tmp_path, piggyback, dtype):
    """The four prompts one after another (hits of 0, 48, 48, 48 tokens), then all four again at once (each finds its own
    entry: hits of 48, 64, 64, 80 tokens = the whole blocks below its last token, copied by one call). Every stream is the
    closed form of its full prompt; a hit forwards prompt_len - hit tokens, the first of them behind a context of hit."""
    model, perm = _model(tmp_path, dtype, num_blocks=64, max_prefill_chunk=32, enable_prefix_caching=True,
                         prefix_cache_max_seqs=4)
    prompts = _shared_prompts(len(perm))
    want = synth.decisive_expected_tokens(prompts, perm, OFFSET, STEPS)
    eng, seen = _engine(model, piggyback)
    copies = []
    inner_copy = model.copy_kv_prefix
    model.copy_kv_prefix = lambda s, d, n: (copies.append((list(s), list(d), list(n))), inner_copy(s, d, n))[1]

    async def run():
        for i, p in enumerate(prompts):
            since, hit_before = len(seen), eng.num_prefix_hit_tokens
            (r,) = await _serve(eng, [(p, STEPS + 1)])
            assert r.output_token_ids == [step[i] for step in want], i
            hit = 48 if i else 0
            assert eng.num_prefix_hit_tokens - hit_before == hit
            assert list(_fed(seen, since).values()) == [(hit, len(p) - hit)], i
        since = len(seen)
        again = await _serve(eng, [(p, STEPS + 1) for p in prompts])
        for i, r in enumerate(again):
            assert r.output_token_ids == [step[i] for step in want], i
        hits = [(len(p) - 1) // BLOCK * BLOCK for p in prompts]
        assert hits == [48, 64, 64, 80]
        assert sorted(_fed(seen, since).values()) == sorted((h, len(p) - h) for h, p in zip(hits, prompts))
        return hits
    hits = asyncio.run(run())
    assert eng.num_prefix_hits == 7 and eng.num_prefix_hit_tokens == 3 * 48 + sum(hits)
    assert eng.num_prefix_evictions == 0 and (eng.num_swapped_out, eng.num_swapped_in) == (0, 0)
    assert copies[-1][2] == hits and len(copies) == 4                   # the four hits of the last step: one call
    assert len(eng.scheduler.prefix_cache) == 4
    assert model.gpu_block_manager.num_free_blocks < 64
    assert eng.drop_prefix_cache() == 4
    assert model.gpu_block_manager.num_free_blocks == 64 and model.cpu_block_manager.num_free_blocks == 8
    _churn.assert_scheduler_empty(eng)


def test_engine_evicts_cached_blocks_instead_of_swapping(tmp_path):
    """A pool of 16 blocks: a finished request holds 6 - 7 as a cache entry, so the third and the fourth request are
    admitted only because the least recently used entry goes (never the one they copy from). Nothing is swapped out."""
    model, perm = _model(tmp_path, "bfloat16", num_blocks=16, max_prefill_chunk=32, enable_prefix_caching=True,
                         prefix_cache_max_seqs=4)
    prompts = _shared_prompts(len(perm))
    want = synth.decisive_expected_tokens(prompts, perm, OFFSET, STEPS)
    eng, seen = _engine(model)

    async def run():
        for i, p in enumerate(prompts):
            (r,) = await _serve(eng, [(p, STEPS + 1)])
            assert r.output_token_ids == [step[i] for step in want], i
    asyncio.run(run())
    assert eng.num_swapped_out == 0 and eng.num_swapped_in == 0
    assert eng.num_prefix_evictions == 2 and eng.num_prefix_hits == 3 and eng.num_prefix_hit_tokens == 3 * 48
    assert eng.drop_prefix_cache() == 2
    assert model.gpu_block_manager.num_free_blocks == 16
    _churn.assert_scheduler_empty(eng)


def test_engine_with_speculation_a_verified_request_donates(tmp_path):
    """speculative_ngram = 3, 16-bit pool. The first request's prompt plants 1-gram matches (tests/_churn.py:
    _plant_pairs), so it takes verify steps with accepted and rejected drafts, which store K/V past its length; it
    finishes as a cache entry (its row stays marked as one that may own a surplus block — at the end it owns none: drafts
    are clipped to output_len, so a request that runs to output_len never reserves past its last token). Only the whole
    blocks under num_tokens - 1 are cached: the follow-up shares those 96 tokens — 21 of them generated, some stored by
    verify steps — adds 5 of its own, hits 96 and walks the closed form, whose first 14 outputs read copied K/V."""
    model, perm = _model(tmp_path, "float16", num_blocks=40, max_prefill_chunk=32, enable_prefix_caching=True,
                         prefix_cache_max_seqs=4, speculative_ngram=3)
    rng = random.Random(0)
    first = _churn._plant_pairs([rng.randrange(len(perm)) for _ in range(75)], perm)
    eng, seen = _engine(model)

    async def run():
        (r1,) = await _serve(eng, [(first, 30)])
        assert r1.output_token_ids == _churn.closed_form(first, perm, 30)
        assert eng.num_verify_steps > 0 and 0 < eng.num_accepted_tokens < eng.num_draft_tokens
        assert r1.kv_reserved_tokens > 0 and r1.request_id in model.gpu_block_manager.host.surplus_ok
        entry = eng.scheduler.prefix_cache.entries()[0]
        assert (entry.seq_id, entry.num_cached_tokens) == (r1.request_id, 96)
        follow = (first + r1.output_token_ids)[:96] + [rng.randrange(len(perm)) for _ in range(5)]
        since = len(seen)
        (r2,) = await _serve(eng, [(follow, 30)])
        assert r2.output_token_ids == _churn.closed_form(follow, perm, 30)
        assert list(_fed(seen, since).values()) == [(96, 5)]
    asyncio.run(run())
    assert eng.num_prefix_hits == 1 and eng.num_prefix_hit_tokens == 96
    eng.drop_prefix_cache()
    assert model.gpu_block_manager.num_free_blocks == 40
    _churn.assert_scheduler_empty(eng)
