"""Prefix caching by KV block copy, on the CPU: the config fields, the trie (server/prefix_cache.py), the scheduler's
invariant — a cached block never causes a swap-out, never delays a swap-in and never refuses an admission the scheduler
without the cache grants — and the real Engine against a data plane that keeps a per-row token ledger."""
import argparse
import asyncio
import random

import pytest

import _churn

BLOCK = 16


def _cfg(**kw):
    from swiftllm_amd import EngineConfig
    base = dict(model_path="", use_dummy=False, block_size=BLOCK, gpu_mem_utilization=0.9, num_cpu_blocks=64,
                max_seqs_in_block_table=16, max_blocks_per_seq=16, max_batch_size=8, max_tokens_in_batch=96)
    base.update(kw)
    return EngineConfig(**base)


# ---- EngineConfig ----------------------------------------------------------------------------------------------------
def test_config_defaults_change_nothing_else():
    from swiftllm_amd import EngineConfig
    cfg = _cfg(max_prefill_chunk=32)
    assert cfg.enable_prefix_caching is False and cfg.prefix_cache_max_seqs == 256
    on = _cfg(max_prefill_chunk=32, enable_prefix_caching=True, prefix_cache_max_seqs=8)
    a, b = dict(vars(cfg)), dict(vars(on))
    for d in (a, b):
        d.pop("enable_prefix_caching")
        d.pop("prefix_cache_max_seqs")
    assert a == b
    # the default of 256 rows is not held against a small block table while the option is off
    assert _cfg(max_seqs_in_block_table=4).prefix_cache_max_seqs == 256
    assert [f.name for f in __import__("dataclasses").fields(EngineConfig)][-2:] == ["enable_prefix_caching",
                                                                                     "prefix_cache_max_seqs"]


def test_config_refusals():
    with pytest.raises(ValueError, match="max_prefill_chunk"):
        _cfg(enable_prefix_caching=True, prefix_cache_max_seqs=8)                      # a hit IS a chunk behind a context
    with pytest.raises(ValueError, match="decode_engine"):
        _cfg(enable_prefix_caching=True, prefix_cache_max_seqs=8, max_prefill_chunk=32, tuning={"decode_engine": True})
    with pytest.raises(ValueError, match="prefix_cache_max_seqs"):
        _cfg(enable_prefix_caching=True, max_prefill_chunk=32, prefix_cache_max_seqs=0)
    with pytest.raises(ValueError, match="prefix_cache_max_seqs"):
        _cfg(prefix_cache_max_seqs=0)
    with pytest.raises(ValueError, match="prefix_cache_max_seqs"):
        _cfg(enable_prefix_caching=True, max_prefill_chunk=32, prefix_cache_max_seqs=16)     # == max_seqs_in_block_table
    with pytest.raises(ValueError, match="prefix_cache_max_seqs"):
        _cfg(enable_prefix_caching=True, max_prefill_chunk=32)                               # the default 256 >= 16 rows
    assert _cfg(enable_prefix_caching=True, max_prefill_chunk=32, prefix_cache_max_seqs=15).enable_prefix_caching


def test_cli_flags():
    from swiftllm_amd import EngineConfig
    ap = argparse.ArgumentParser()
    EngineConfig.add_cli_args(ap)
    off = ap.parse_args(["--model-path", "x"])
    assert off.enable_prefix_caching is False and off.prefix_cache_max_seqs == 256
    on = ap.parse_args(["--model-path", "x", "--enable-prefix-caching", "--prefix-cache-max-seqs", "64",
                        "--max-prefill-chunk", "512"])
    assert on.enable_prefix_caching is True and on.prefix_cache_max_seqs == 64
    fields = {f.name for f in __import__("dataclasses").fields(EngineConfig)}
    cfg = EngineConfig(**{k: v for k, v in vars(on).items() if k in fields})        # what api_server does
    assert cfg.enable_prefix_caching and cfg.prefix_cache_max_seqs == 64 and cfg.max_prefill_chunk == 512


def test_entry_point_refusals_need_no_device():
    """swl_kv_copy_blocks checks its arguments before anything is launched (the pointers here are never dereferenced)."""
    import ctypes
    from swiftllm_amd import _hip
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    f = lib.swl_kv_copy_blocks
    assert f(None, None, None, None, 0, 1 << 20, 8, None) == 0
    assert f(p, p, p, p, 0, 1 << 20, 8, None) == 0
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert f(*args, 1, 512, 8, None) == -1
    assert f(p, p, p, p, -1, 512, 8, None) == -1
    assert f(p, p, p, p, 1, 0, 8, None) == -1
    assert f(p, p, p, p, 1, 512, 0, None) == -1
    assert f(p, p, p, p, 1, 520, 8, None) == -2
    assert f(p + 8, p, p, p, 1, 512, 8, None) == -1
    assert f(p, p + 4, p, p, 1, 512, 8, None) == -1
    assert "swl_kv_copy_blocks" not in _hip.SIGNATURES and _hip._SPECIAL["swl_kv_copy_blocks"][1] is ctypes.c_int32
    assert lib.swl_abi_version() == 2


# ---- PrefixCache -----------------------------------------------------------------------------------------------------
def _toks(*blocks, tail=()):
    """Token ids made of whole blocks named by an int (block b = 16 ids b*100 .. b*100 + 15) and a tail."""
    out = []
    for b in blocks:
        out += [b * 100 + i for i in range(BLOCK)]
    return out + list(tail)


def _node_count(cache):
    n, stack = 0, [cache._root]
    while stack:
        node = stack.pop()
        n += len(node.children)
        stack += node.children.values()
    return n


def _check_trie(cache):
    """Every node holds an entry; every entry of a child is in its parent; an entry sits on exactly its own path."""
    seen = {}
    stack = [(cache._root, None, 0)]
    while stack:
        node, parent, depth = stack.pop()
        if parent is not None:
            assert node.entries
            for e in node.entries:
                seen[e.seq_id] = seen.get(e.seq_id, 0) + 1
            if depth > 1:
                assert node.entries <= parent.entries
        for child in node.children.values():
            stack.append((child, node, depth + 1))
    assert seen == {e.seq_id: e.num_cached_tokens // BLOCK for e in cache.entries()}
    assert cache.num_blocks_held == sum(e.num_blocks_held for e in cache.entries())


def test_match_is_exact_whole_blocks_and_capped():
    from swiftllm_amd.server.prefix_cache import PrefixCache
    c = PrefixCache(BLOCK, 8)
    assert c.match(_toks(1, 2, 3)) == (None, 0)
    assert c.insert(5, _toks(1, 2, tail=[7, 8, 9]), blocks_held=3)
    e = c.entries()[0]
    assert (e.seq_id, e.num_blocks_held, e.num_cached_tokens) == (5, 3, 32)
    # the cap: at least one prompt token must be forwarded — a 32-token prompt identical to the cached one matches 16
    assert c.match(_toks(1, 2)) == (e, 16)
    assert c.match(_toks(1, 2, tail=[7])) == (e, 32)
    assert c.match(_toks(1, 2, 3, 4)) == (e, 32)
    assert c.match(_toks(1, tail=[0])) == (e, 16)
    assert c.match(_toks(1)) == (None, 0) and c.match(_toks(1)[:5]) == (None, 0) and c.match([]) == (None, 0)
    # exact keys: one differing id in a block ends the chain there; the tail of the entry (no whole block) is not cached
    p = _toks(1, 2, 3)
    p[20] += 1
    assert c.match(p) == (e, 16)
    p = _toks(1, 2, 3)
    p[0] += 1
    assert c.match(p) == (None, 0)
    assert c.match(_toks(2, 1, 3)) == (None, 0)
    _check_trie(c)


def test_duplicate_insert_and_capacity():
    from swiftllm_amd.server.prefix_cache import PrefixCache
    c = PrefixCache(BLOCK, 2)
    assert not c.insert(1, _toks(1)[:15], 1)                # no whole block
    assert c.insert(1, _toks(1, 2, 3), 4)
    assert not c.insert(2, _toks(1, 2, 3), 4)               # the same prompt twice adds nothing
    assert not c.insert(2, _toks(1, 2, tail=[5]), 3)        # ... nor does a prefix of it: its deepest node holds an entry
    assert c.holds(_toks(1, 2)) and c.holds(_toks(1, 2, 3, tail=[4])) and not c.holds(_toks(1, 2, 3, 4))
    assert not c.insert(1, _toks(9), 1)                     # the row is an entry already
    assert c.insert(2, _toks(1, 2, 3, 4), 5)                # a longer chain is new
    assert not c.insert(3, _toks(7), 1) and len(c) == 2     # full: the caller evicts first
    assert c.num_blocks_held == 9
    _check_trie(c)


def test_eviction_unlinks_the_entrys_path_and_keeps_the_others():
    from swiftllm_amd.server.prefix_cache import PrefixCache
    for evict_long_first in (True, False):
        c = PrefixCache(BLOCK, 8)
        assert c.insert(1, _toks(1, 2), 2)                  # short
        assert c.insert(2, _toks(1, 2, 3, 4), 4)            # long, shares the chain
        assert c.insert(3, _toks(1, 9), 2)                  # a branch
        assert _node_count(c) == 5
        short, long_ = (next(e for e in c.entries() if e.seq_id == s) for s in (1, 2))
        if evict_long_first:
            assert c.evict_lru(exclude=[1, 3]) is long_
            assert _node_count(c) == 3                      # nodes 3 and 4 went, 1 and 2 stay with the short entry
            assert c.match(_toks(1, 2, 3, 4, 5)) == (short, 32)
        else:
            assert c.evict_lru(exclude=[2, 3]) is short
            assert _node_count(c) == 5                      # the long entry still needs every node
            assert c.match(_toks(1, 2, 3, 4, 5)) == (long_, 64)
        _check_trie(c)
        assert c.match(_toks(1, 9, 9))[0].seq_id == 3
        assert len(c) == 2
    c.clear()
    assert len(c) == 0 and _node_count(c) == 0 and c.num_blocks_held == 0


def test_lru_order_ties_and_exclude():
    from swiftllm_amd.server.prefix_cache import PrefixCache
    c = PrefixCache(BLOCK, 8)
    for sid, blocks in ((1, (1, 2)), (2, (1, 3)), (3, (4,)), (4, (1, 5))):
        assert c.insert(sid, _toks(*blocks), len(blocks))
    # several entries share block 1: the tie goes to the most recently used (inserted last: 4)
    assert c.match(_toks(1, 8))[0].seq_id == 4
    assert c.match(_toks(1, 2, 8))[0].seq_id == 1           # touches 1
    assert c.match(_toks(1, 8))[0].seq_id == 1              # ... which now wins the tie (and is touched again)
    # LRU order now: 2, 3, 4, 1
    assert c.evict_lru(exclude={2}).seq_id == 3
    assert c.evict_lru().seq_id == 2
    assert c.evict_lru(exclude=[4, 1]) is None
    assert c.evict_lru().seq_id == 4
    assert c.evict_lru().seq_id == 1
    assert c.evict_lru() is None and _node_count(c) == 0
    assert c.insert(1, _toks(1, 2), 2) and sorted(c.clear()) == [1] and c.match(_toks(1, 2, 3)) == (None, 0)


# ---- the scheduler's invariant ---------------------------------------------------------------------------------------
def _request(prompt, output_len, **kw):
    from swiftllm_amd.server import RawRequest, Request
    return Request(RawRequest("", output_len, list(prompt), **kw))


def _finish_step(sch, batch, cache_on):
    """What the engine does with a step's tokens, without a data plane."""
    finished = []
    for r in batch:
        if not r.is_prompt_resident():
            r.num_prefilled += r.prefill_take or r.prompt_len - r.num_prefilled
            r.prefill_take = 0
            if r.num_prefilled < r.prompt_len:
                continue
        r.output_token_ids.append((r.prompt_len * 31 + len(r.output_token_ids)) % 1000)
        if r.is_finished():
            finished.append(r)
    kept = [r for r in finished if sch.retire(r)]
    assert cache_on or not kept
    sch.on_batch_finish(batch)
    return kept


def test_cached_blocks_never_change_what_the_scheduler_grants():
    """One arrival trace without shared prefixes through two schedulers, cache on and off, requests finishing in lockstep:
    the same batch, the same prompt-token takes and the same swaps in every step; with the cache on, running blocks plus
    cached blocks fit the pool once the step's evictions are applied. (Block-table rows differ — cached entries hold
    theirs — so requests are compared by arrival index.)"""
    from swiftllm_amd.server.scheduler import Scheduler
    rng = random.Random(11)
    num_blocks = 26
    trace = [(step // 2, [rng.randrange(1000) for _ in range(rng.randint(20, 90))], rng.randint(8, 30)) for step in range(60)]
    kw = dict(max_prefill_chunk=48, max_seqs_in_block_table=32)
    schedulers = [Scheduler(None, _cfg(**kw), num_blocks, piggyback=True),
                  Scheduler(None, _cfg(enable_prefix_caching=True, prefix_cache_max_seqs=6, **kw), num_blocks, piggyback=True)]
    reqs = [[_request(p, n) for _, p, n in trace] for _ in schedulers]
    for rs in reqs:
        for i, r in enumerate(rs):
            r.index = i
    swaps = evictions = cached_peak = 0
    for step in range(2000):
        shapes = []
        for which, (sch, rs) in enumerate(zip(schedulers, reqs)):
            sch.on_requests_arrival([r for r, (at, _, _) in zip(rs, trace) if at == step])
            batch, swap_in, swap_out = sch.get_next_batch()
            evicted, copies = sch.take_cache_work()
            if which == 0:
                assert not evicted and not copies
            else:
                assert not copies                       # (no shared prefixes)
                evictions += len(evicted)
                cached = sch.prefix_cache.num_blocks_held
                cached_peak = max(cached_peak, cached)
                assert sch._running_blocks() + cached <= num_blocks, step
                assert len(sch.prefix_cache) <= 6
                # rows: the running, the swapped and the cached ones, nothing lost
                assert (sch.request_id_manager.num_free() + len(sch.running_q) + len(sch.swapped_q)
                        + len(sch.prefix_cache)) == 32
            shapes.append(([r.index for r in batch], [r.prefill_take for r in batch], [r.index for r in swap_in],
                           [r.index for r in swap_out]))
            swaps += len(swap_out)
            _finish_step(sch, batch, cache_on=bool(which))
            evicted, _ = sch.take_cache_work()
            evictions += len(evicted)
        assert shapes[0] == shapes[1], (step, shapes)
        if step > 30 and not any(s.has_work() for s in schedulers):
            break
    else:
        raise AssertionError("the trace did not finish")
    assert all(r.is_finished() for rs in reqs for r in rs)
    assert swaps > 0 and evictions > 0 and cached_peak > 0, (swaps, evictions, cached_peak)
    on = schedulers[1]
    freed = on.drop_prefix_cache()
    assert len(freed) > 0 and on.request_id_manager.num_free() == 32 and not on.take_cache_work()[0]


def test_a_pinned_donor_never_refuses_an_admission():
    """Pool of 12 blocks, one entry of 4. A (hits the entry, 5 blocks) and B (5 blocks) wait: the scheduler without the
    cache admits both in one step. With the cache, B's room needs the entry A would copy from, so the step is redone
    without hits: both admitted, A prefills whole, the entry goes."""
    from swiftllm_amd.server.scheduler import Scheduler
    rng = random.Random(3)
    shared = [rng.randrange(1000) for _ in range(48)]
    donor = _request(shared + [1] * 10, 3)
    a = _request(shared + [2] * 22, 5)
    b = _request([rng.randrange(1000) for _ in range(70)], 5)
    sch = Scheduler(None, _cfg(enable_prefix_caching=True, prefix_cache_max_seqs=4, max_prefill_chunk=96), 12)
    sch.on_requests_arrival([donor])
    while not donor.is_finished():
        batch, _, _ = sch.get_next_batch()
        _finish_step(sch, batch, True)
    assert len(sch.prefix_cache) == 1 and sch.prefix_cache.num_blocks_held == 4
    donor_row = donor.request_id
    # alone, A hits
    sch.on_requests_arrival([a])
    batch, _, _ = sch.get_next_batch()
    assert batch == [a] and (a.num_prefilled, a.prefill_take) == (48, 22)
    assert sch.take_cache_work() == ([], [(donor_row, a.request_id, 48)])
    # (undo: put A back as a new arrival)
    sch.running_q.clear()
    sch.request_id_manager.free_id(a.request_id)
    a.request_id, a.num_prefilled, a.prefill_take = -1, 0, 0
    sch.on_requests_arrival([a, b])
    batch, swap_in, swap_out = sch.get_next_batch()
    assert batch == [a, b] and not swap_in and not swap_out
    assert (a.num_prefilled, a.prefill_take, b.num_prefilled, b.prefill_take) == (0, 70, 0, 26)
    assert sch.take_cache_work() == ([donor_row], [])
    assert len(sch.prefix_cache) == 0 and a.request_id != b.request_id


# ---- the real Engine against a data plane with a token ledger ------------------------------------------------------------
class LedgerModel(_churn.ClosedFormModel):
    """ClosedFormModel (it remembers every row's tokens and counts its blocks against the pool) + copy_kv_prefix, and a
    ledger check: `truth(row)` gives the tokens of the request that holds the row, and every forward's context — what the
    row really holds, copied tokens included — must equal them."""

    def __init__(self, engine_config, perm, num_blocks):
        super().__init__(engine_config, perm, num_blocks)
        self.truth = None
        self.calls = []         # ("free", rows) | ("copy", src, dst, tokens) | ("forward", rows, contexts, tokens fed)

    def copy_kv_prefix(self, src_seq_ids, dst_seq_ids, num_tokens):
        self.calls.append(("copy", list(src_seq_ids), list(dst_seq_ids), list(num_tokens)))
        assert len(src_seq_ids) == len(dst_seq_ids) == len(num_tokens) and len(set(dst_seq_ids)) == len(dst_seq_ids)
        for src, dst, n in zip(src_seq_ids, dst_seq_ids, num_tokens):
            assert n > 0 and n % BLOCK == 0 and dst not in self.seqs and src in self.seqs and src not in self.on_host
            assert len(self.seqs[src]) >= n and dst not in src_seq_ids
            self.seqs[dst] = list(self.seqs[src][:n])
            self.prompt_lens[dst] = n
            self.blocks[dst] = n // BLOCK
        self._check_pools()

    def forward(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, sampling_params=None, prefill_ctx_lens=None,
                lora=None):
        n_pre = len(input_ids_list) - len(decoding_seq_lens_list)
        ctx = list(prefill_ctx_lens or [0] * n_pre) + [n - 1 for n in decoding_seq_lens_list]
        self.calls.append(("forward", list(seq_ids_list), ctx, [len(x) for x in input_ids_list]))
        for i, (ids, sid, c) in enumerate(zip(input_ids_list, seq_ids_list, ctx)):
            want = self.truth(sid)
            assert want[c:c + len(ids)] == list(ids), f"row {sid}: fed tokens are not the request's at {c}"
            if c:
                assert self.seqs[sid][:c] == want[:c], f"row {sid}: its {c} resident tokens are not the request's"
            if i < n_pre and c:     # (ClosedFormModel starts a row at a context-0 prefill; a copied row exists already)
                assert sid in self.seqs
        return super().forward(input_ids_list, seq_ids_list, decoding_seq_lens_list, sampling_params=sampling_params,
                               prefill_ctx_lens=prefill_ctx_lens)

    def free_seqs_resources(self, seq_ids_list):
        self.calls.append(("free", list(seq_ids_list)))
        super().free_seqs_resources(seq_ids_list)


def _engine(num_blocks, piggyback=True, **kw):
    from swiftllm_amd import Engine
    _, _, perm = _churn.decisive("float16")
    base = dict(max_prefill_chunk=32, enable_prefix_caching=True, prefix_cache_max_seqs=8, num_cpu_blocks=48)
    base.update(kw)
    ecfg = _cfg(**base)
    model = LedgerModel(ecfg, perm, num_blocks)
    eng = Engine(ecfg, model=model, piggyback=piggyback)

    def truth(row):
        held = [r for r in eng.scheduler.running_q if r.request_id == row]
        assert len(held) == 1
        return held[0].prompt_token_ids + held[0].output_token_ids
    model.truth = truth
    return eng, model, perm


async def _serve_one_by_one(eng, num_blocks, reqs):
    if not eng.initialized:
        await eng.initialize(num_blocks)
    eng.event_loop = asyncio.get_running_loop()     # (a test calls this under several asyncio.run)
    for r in reqs:
        eng.scheduler.on_requests_arrival([r])
        for _ in range(200):
            if r.is_finished():
                break
            assert await eng.step()
        assert r.is_finished()


def _prompts(perm, seed=5):
    rng = random.Random(seed)
    vocab = len(perm)
    shared = [rng.randrange(vocab) for _ in range(48)]
    return shared, [shared + [rng.randrange(vocab) for _ in range(12 + 3 * i)] for i in range(4)]


def test_engine_hits_copies_before_the_forward_and_gives_everything_back():
    from swiftllm_amd.sampling_params import SamplingParams
    eng, model, perm = _engine(64)
    shared, prompts = _prompts(perm)
    out_len = 9
    reqs = [_request(p, out_len) for p in prompts]
    hits = []

    async def run():
        for r in reqs:
            before = eng.num_prefix_hit_tokens
            await _serve_one_by_one(eng, 64, [r])
            hits.append(eng.num_prefix_hit_tokens - before)
        # a follow-up chat turn: the first prompt plus the first request's own output
        follow = _request(prompts[0] + reqs[0].output_token_ids, 20)      # (long enough to add a block of its own)
        before = eng.num_prefix_hit_tokens
        await _serve_one_by_one(eng, 64, [follow])
        hits.append(eng.num_prefix_hit_tokens - before)
        return follow
    follow = asyncio.run(run())
    whole = (len(prompts[0]) + out_len - 1) // BLOCK * BLOCK
    assert hits == [0, 48, 48, 48, whole] and whole == 64
    assert (eng.num_prefix_hits, eng.num_prefix_hit_tokens, eng.num_prefix_evictions) == (4, 3 * 48 + whole, 0)
    for r in reqs + [follow]:
        assert r.output_token_ids == _churn.closed_form(r.prompt_token_ids, perm, r.output_len)
    # every copy is followed at once by the forward that uses it: its row, behind a context of the copied tokens, fed
    # the rest of the prompt (chunked: at most 32 tokens of it)
    copies = [i for i, c in enumerate(model.calls) if c[0] == "copy"]
    assert len(copies) == 4
    for i in copies:
        _, src, dst, tokens = model.calls[i]
        kind, rows, ctx, fed = model.calls[i + 1]
        assert kind == "forward" and rows[0] == dst[0] and ctx[0] == tokens[0] and 0 < fed[0] <= 32
    # no forward of a missed prompt starts behind a context
    first = next(c for c in model.calls if c[0] == "forward")
    assert first[2] == [0] and first[3] == [32]
    assert len(eng.scheduler.prefix_cache) == 5 and not eng.scheduler.has_work()

    # LoRA and logit-processing requests neither hit nor donate
    calls_before, entries_before = len(model.calls), len(eng.scheduler.prefix_cache)
    plain = [_request(prompts[0] + [7, 7, 7], 4, lora="adapter"),
             _request(prompts[1] + [8, 8, 8], 4, sampling_params=SamplingParams(repetition_penalty=1.05))]
    asyncio.run(_serve_one_by_one(eng, 64, plain))
    assert eng.num_prefix_hits == 4 and len(eng.scheduler.prefix_cache) == entries_before
    assert not any(c[0] == "copy" for c in model.calls[calls_before:])
    assert sum(len(c[1]) for c in model.calls[calls_before:] if c[0] == "free") == 2      # freed as always
    # a plain sampled request is eligible: it hits
    sampled = _request(prompts[2] + [9, 9], 14, sampling_params=SamplingParams(temperature=0.8, top_p=0.9, seed=4))
    asyncio.run(_serve_one_by_one(eng, 64, [sampled]))
    assert eng.num_prefix_hits == 5 and len(eng.scheduler.prefix_cache) == entries_before + 1

    assert not model.is_empty()
    assert eng.drop_prefix_cache() == entries_before + 1
    assert model.is_empty() and len(eng.scheduler.prefix_cache) == 0
    _churn.assert_scheduler_empty(eng)
    assert eng.drop_prefix_cache() == 0


def test_engine_evicts_before_it_copies_and_never_swaps_for_the_cache():
    """Pool of 12 blocks, requests of 5: the third request hits one entry and needs the other one's blocks. The entry goes
    first (free), then the copy, then the forward — the ledger model counts blocks at every call — and nothing is swapped."""
    eng, model, perm = _engine(12)
    _, prompts = _prompts(perm)
    reqs = [_request(p, 8) for p in prompts]
    asyncio.run(_serve_one_by_one(eng, 12, reqs))
    for r in reqs:
        assert r.output_token_ids == _churn.closed_form(r.prompt_token_ids, perm, 8)
    assert (eng.num_swapped_out, eng.num_swapped_in) == (0, 0)
    assert eng.num_prefix_hits == 3 and eng.num_prefix_hit_tokens == 3 * 48 and eng.num_prefix_evictions == 2
    kinds = [c[0] for c in model.calls]
    both = [i for i in range(len(kinds) - 2) if kinds[i:i + 3] == ["free", "copy", "forward"]]
    assert len(both) == 2
    for i in both:
        assert set(model.calls[i][1]).isdisjoint(model.calls[i + 1][1])       # the donor is not the entry that went
    eng.drop_prefix_cache()
    assert model.is_empty()
    _churn.assert_scheduler_empty(eng)


def test_engine_with_the_option_off_never_touches_the_cache():
    eng, model, perm = _engine(64, enable_prefix_caching=False)
    _, prompts = _prompts(perm)
    reqs = [_request(p, 6) for p in prompts]
    asyncio.run(_serve_one_by_one(eng, 64, reqs))
    assert eng.scheduler.prefix_cache is None and not any(c[0] == "copy" for c in model.calls)
    assert (eng.num_prefix_hits, eng.num_prefix_hit_tokens, eng.num_prefix_evictions) == (0, 0, 0)
    assert all(c[2][0] == 0 or c[3][0] <= 32 for c in model.calls if c[0] == "forward")
    assert model.is_empty() and eng.drop_prefix_cache() == 0
    _churn.assert_scheduler_empty(eng)


def test_engine_with_speculation_a_verified_request_donates():
    """The scenario of tests/test_gpu_prefix_cache.py on the ledger model: the first request takes verify steps (accepted
    and rejected drafts store tokens past its length; the ledger forgets them when the length is placed again), donates
    the whole blocks under num_tokens - 1, and the follow-up hits all 96 of them — 21 generated, some stored by verify."""
    eng, model, perm = _engine(40, speculative_ngram=3)
    rng = random.Random(0)
    first = _request(_churn._plant_pairs([rng.randrange(len(perm)) for _ in range(75)], perm), 30)
    asyncio.run(_serve_one_by_one(eng, 40, [first]))
    assert eng.num_verify_steps > 0 and 0 < eng.num_accepted_tokens < eng.num_draft_tokens
    # drafts are clipped to output_len: a request that runs to output_len reserves nothing past its last stored token
    assert 0 < first.kv_reserved_tokens <= first.num_tokens() - 1
    entry = eng.scheduler.prefix_cache.entries()[0]
    assert (entry.seq_id, entry.num_cached_tokens, entry.num_blocks_held) == (first.request_id, 96, 7)
    follow = _request((first.prompt_token_ids + first.output_token_ids)[:96] + [rng.randrange(len(perm)) for _ in range(5)], 30)
    asyncio.run(_serve_one_by_one(eng, 40, [follow]))
    assert (eng.num_prefix_hits, eng.num_prefix_hit_tokens) == (1, 96)
    for r in (first, follow):
        assert r.output_token_ids == _churn.closed_form(r.prompt_token_ids, perm, 30)
    i = next(i for i, c in enumerate(model.calls) if c[0] == "copy")
    assert model.calls[i][1:] == ([first.request_id], [follow.request_id], [96])
    assert model.calls[i + 1] == ("forward", [follow.request_id], [96], [5])
    eng.drop_prefix_cache()
    assert model.is_empty()
    _churn.assert_scheduler_empty(eng)
