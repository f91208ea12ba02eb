"""Prompt-lookup speculative decoding on the CPU: the n-gram proposer against a brute-force scan, accept(), the config and
CLI, the verify plan, the scheduler's block counts, and the Engine over fake data planes whose streams make every draft
right, every draft wrong, or one of three right (token streams identical to the same engine with the option off)."""
import argparse
import asyncio
import dataclasses
import types

import numpy as np
import pytest

from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.sampling_params import SamplingParams
from swiftllm_amd.server import Engine, RawRequest, Request, Scheduler
from swiftllm_amd.server.speculative import MAX_NGRAM, NgramProposer, accept
from swiftllm_amd.worker.batch_plan import plan_batch, plan_verify

BS = 16


# ---- proposer --------------------------------------------------------------------------------------------------------
def _brute(tokens, k):
    """n from 3 down to 1: the most recent EARLIER occurrence of the last n tokens, the up-to-k tokens after it."""
    if k <= 0:
        return []
    size = len(tokens)
    for n in range(min(MAX_NGRAM, size - 1), 0, -1):
        tail = tokens[size - n:]
        for s in range(size - n - 1, -1, -1):
            if tokens[s:s + n] == tail:
                return tokens[s + n:s + n + k]
    return []


@pytest.mark.parametrize("vocab,period", [(3, 0), (50, 0), (1000, 0), (1000, 7), (1000, 1), (5, 4)])
def test_incremental_index_equals_a_brute_force_scan(vocab, period):
    rng = np.random.RandomState(vocab + period)
    hist = rng.randint(0, vocab, size=300).tolist()
    if period:
        hist = (hist[:period] * 300)[:300]
        hist[100] = vocab + 1           # one break in the period
    prop = NgramProposer()
    for i, t in enumerate(hist):
        prop.append(t)
        assert len(prop) == i + 1
        for k in (0, 1, 3, 5):
            got = prop.propose(k)
            assert got == _brute(hist[:i + 1], k), (i, k)
            assert len(got) <= k
    # sync() from prompt + output in pieces gives the same index as appending one by one
    other = NgramProposer(hist[:10])
    other.sync(hist[:120], [])
    other.sync(hist[:120], hist[120:200])
    other.sync(hist[:120], hist[120:])
    assert other.tokens == prop.tokens and other.propose(3) == prop.propose(3)


def test_longest_ngram_and_most_recent_match_win():
    # the last 3 tokens (1, 2, 3) occurred once, followed by 7; the 1-gram (3) occurred later, followed by 9
    assert NgramProposer([1, 2, 3, 7, 5, 3, 9, 1, 2, 3]).propose(2) == [7, 5]
    # without the 3-gram the 2-gram decides, then the 1-gram
    assert NgramProposer([4, 2, 3, 7, 5, 3, 9, 1, 2, 3]).propose(2) == [7, 5]
    assert NgramProposer([4, 2, 8, 7, 5, 3, 9, 1, 2, 3]).propose(2) == [9, 1]
    # two earlier occurrences of the same n-gram: the most recent one
    assert NgramProposer([1, 2, 3, 7, 1, 2, 3, 8, 1, 2, 3]).propose(1) == [8]
    # never more than k, fewer when the history ends, [] on no match / nothing to match / k = 0
    assert NgramProposer([5, 6, 5]).propose(3) == [6, 5]
    assert NgramProposer([1, 2, 3]).propose(3) == []
    assert NgramProposer([]).propose(3) == [] and NgramProposer([1]).propose(3) == []
    assert NgramProposer([5, 6, 5]).propose(0) == []
    # the suffix is never its own match
    assert NgramProposer([9, 9]).propose(3) == [9]


def test_accept_is_the_longest_equal_prefix():
    assert accept([], [5]) == 0
    assert accept([1, 2, 3], [1, 2, 3, 4]) == 3
    assert accept([1, 2, 3], [1, 9, 3, 4]) == 1
    assert accept([1, 2, 3], [7, 2, 3, 4]) == 0
    assert accept([1, 2], [1, 2]) == 2


# ---- config ----------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    base = dict(model_path="", use_dummy=True, block_size=BS, gpu_mem_utilization=0.9, num_cpu_blocks=512,
                max_seqs_in_block_table=16, max_blocks_per_seq=64, max_batch_size=16, max_tokens_in_batch=1024)
    base.update(kw)
    return EngineConfig(**base)


def test_config_defaults_refusals_and_cli():
    cfg = _cfg()
    assert cfg.speculative_ngram == 0 and cfg.speculative_max_batch == 8
    assert _cfg(speculative_ngram=3, speculative_max_batch=4).speculative_ngram == 3
    with pytest.raises(ValueError, match="speculative_ngram"):
        _cfg(speculative_ngram=-1)
    with pytest.raises(ValueError, match="speculative_max_batch"):
        _cfg(speculative_max_batch=-1)
    with pytest.raises(ValueError, match="fp8_e4m3"):
        _cfg(speculative_ngram=2, kv_cache_dtype="fp8_e4m3")
    with pytest.raises(ValueError, match="decode_engine"):
        _cfg(speculative_ngram=2, tuning={"decode_engine": True})
    _cfg(speculative_ngram=0, kv_cache_dtype="fp8_e4m3")        # off: nothing to refuse
    ap = argparse.ArgumentParser()
    EngineConfig.add_cli_args(ap)
    args = ap.parse_args(["--model-path", "x"])
    assert args.speculative_ngram == 0 and args.speculative_max_batch == 8
    args = ap.parse_args(["--model-path", "x", "--speculative-ngram", "3", "--speculative-max-batch", "4"])
    fields = {f.name for f in dataclasses.fields(EngineConfig)}
    cfg = EngineConfig(**{k: v for k, v in vars(args).items() if k in fields})
    assert cfg.speculative_ngram == 3 and cfg.speculative_max_batch == 4


# ---- plan ------------------------------------------------------------------------------------------------------------
def test_plan_verify_by_hand_and_other_plans_unchanged():
    plan = plan_verify([[7, 8, 9], [4], [1, 2]], [3, 0, 6], [5, 40, 15], num_kv_heads=2)
    assert plan.num_prefill_seqs == 3 and plan.num_decoding_seqs == 0 and plan.num_tokens == 6
    assert plan.position_indices.tolist() == [5, 6, 7, 40, 15, 16]
    assert plan.verify_row_lens.dtype == np.int32 and plan.verify_row_lens.tolist() == [6, 7, 8, 41, 16, 17]
    assert plan.last_token_indices.tolist() == [0, 1, 2, 3, 4, 5]             # every row is a last token
    assert plan.prefill_ctx_lens.tolist() == [5, 40, 15] and plan.seq_lengths_list == [8, 41, 17]
    assert plan.max_prefill_len == 3 and plan.max_prefill_total_len == 41
    assert plan.seq_block_size % BS == 0 and plan.num_seq_blocks == -(-41 // plan.seq_block_size)
    layout, total = plan.packed_layout()
    assert [n for n, _, _ in layout][-2:] == ["prefill_ctx_lens", "verify_row_lens"]
    buf = np.zeros(total, dtype=np.int32)
    assert plan.pack_into(buf) == total
    off = dict((n, o) for n, o, _ in layout)["verify_row_lens"]
    assert buf[off:off + 6].tolist() == [6, 7, 8, 41, 16, 17]
    # a long context is split as a decode of that length would be
    long = plan_verify([[1, 2, 3, 4]], [0], [16000], num_kv_heads=8)
    assert long.num_seq_blocks > 1 and long.seq_block_size * long.num_seq_blocks >= 16004
    # no new segment, no new value in any other plan
    for p in (plan_batch([[1, 2], [3]], [0, 1], [9], 2), plan_batch([[1, 2]], [0], [], 2, prefill_ctx_lens=[4])):
        assert p.verify_row_lens is None
        assert "verify_row_lens" not in [n for n, _, _ in p.packed_layout()[0]]


# ---- scheduler -------------------------------------------------------------------------------------------------------
def test_scheduler_counts_the_blocks_rejected_drafts_claimed():
    sch = Scheduler(types.SimpleNamespace(vocab_size=1000), _cfg(), num_gpu_blocks=10)
    a, b = Request(RawRequest("", 8, list(range(30)))), Request(RawRequest("", 8, list(range(40))))
    assert a.kv_reserved_tokens == 0
    sch.running_q = [a, b]
    assert sch._running_blocks() == 2 + 3 and sch._blocks(a) == 2 and sch._blocks(a, 3) == 3
    a.output_token_ids = [1, 2]                 # 32 tokens; a verify step stored drafts up to 35
    a.kv_reserved_tokens = 35
    assert sch._blocks(a) == 3 and sch._running_blocks() == 3 + 3
    a.output_token_ids = [1, 2, 3, 4, 5, 6]     # grown past the mark: the arithmetic of always
    assert sch._blocks(a) == 3 and sch._blocks(a, 13) == 4


# ---- engine over a fake data plane -----------------------------------------------------------------------------------
def periodic(hist):
    return hist[len(hist) - 5]                  # repeats the last five tokens for ever: prompt lookup is always right


def marker(hist):
    return 1000 + len(hist) if hist[-1] == 0 else 0     # 0, fresh, 0, fresh, ..: what followed the last 0 is never next


def one_of_three(hist):
    r = len(hist) % 3                           # 1, 2, fresh, 1, 2, fresh, ..: after a 1 the draft (2, old fresh, 1) gets 1
    return 1 if r == 0 else 2 if r == 1 else 1000 + len(hist)


class FakeAllocator:
    """Blocks per sequence, as BlockManager's host mirror keeps them: a sequence owns ceil(tokens / 16) blocks of the
    longest length anybody stored for it, until it is freed. Raises when the pool is exhausted."""

    def __init__(self, num_blocks):
        self.num_blocks = num_blocks
        self.held = {}
        self.host = self

    @property
    def num_free_blocks(self):
        return self.num_blocks - sum(self.held.values())

    def num_allocated(self, sid):
        return self.held.get(sid, 0)

    def grow(self, sid, tokens):
        want = max(self.held.get(sid, 0), -(-tokens // BS))
        if want - self.held.get(sid, 0) > self.num_free_blocks:
            raise RuntimeError(f"fake pool exhausted: sequence {sid} wants {want} blocks")
        self.held[sid] = want


class SpecModel:
    """The token after a history is `rule(history)`. Keeps, per sequence, what was stored at every position (a verify
    step stores its drafts too; later steps overwrite them) and every call it received."""

    def __init__(self, num_blocks, rule, max_draft_tokens=3):
        self.model_config = types.SimpleNamespace()
        self.num_blocks = num_blocks
        self.rule = rule
        self.max_draft_tokens = max_draft_tokens
        self.gpu_block_manager = FakeAllocator(num_blocks)
        self.slots = {}
        self.calls = []         # ("forward", args, kwargs) / ("verify", input_ids, seq_ids, ctx_lens)
        self.events = []

    def forward(self, input_ids, seq_ids, decoding_lens, **kwargs):
        self.calls.append(("forward", ([list(x) for x in input_ids], list(seq_ids), list(decoding_lens)), dict(kwargs)))
        n_prefill = len(input_ids) - len(decoding_lens)
        out = []
        for i, (ids, sid) in enumerate(zip(input_ids, seq_ids)):
            if i < n_prefill:
                assert sid not in self.slots
                self.slots[sid] = list(ids)
            else:
                assert len(ids) == 1
                resident = decoding_lens[i - n_prefill] - 1
                assert resident <= len(self.slots[sid])
                self.slots[sid] = self.slots[sid][:resident] + list(ids)
            self.gpu_block_manager.grow(sid, len(self.slots[sid]))
            out.append(self.rule(self.slots[sid]))
        return out

    def forward_verify(self, input_ids, seq_ids, ctx_lens):
        self.calls.append(("verify", [list(x) for x in input_ids], list(seq_ids), list(ctx_lens)))
        out = []
        for ids, sid, ctx in zip(input_ids, seq_ids, ctx_lens):
            assert 1 <= len(ids) <= self.max_draft_tokens + 1 and ctx <= len(self.slots[sid])
            self.slots[sid] = self.slots[sid][:ctx] + list(ids)
            self.gpu_block_manager.grow(sid, ctx + len(ids))
            out.append([self.rule(self.slots[sid][:ctx + j + 1]) for j in range(len(ids))])
        return out

    def swap_in_seqs(self, ids):
        self.events.append(("in", list(ids)))

    def swap_out_seqs(self, ids):
        self.events.append(("out", list(ids)))

    def free_seqs_resources(self, ids):
        self.events.append(("free", list(ids)))
        for i in ids:
            self.slots.pop(i, None)
            self.gpu_block_manager.held.pop(i, None)


def _expected(rule, prompt, n):
    hist = list(prompt)
    for _ in range(n):
        hist.append(rule(hist))
    return hist[len(prompt):]


def _prompts(count, base=23):
    rng = np.random.RandomState(5)
    return [rng.permutation(np.arange(3, 900))[:base + 6 * i].tolist() for i in range(count)]     # distinct tokens >= 3


def _run(cfg, rule, jobs, num_blocks=200, sampling=None, check=None):
    """Single-step the engine until every request is done. jobs: [(prompt, output_len)]. Returns (engine, model, requests,
    streamed tokens per request)."""
    async def run():
        model = SpecModel(num_blocks, rule)
        eng = Engine(cfg, model=model)
        await eng.initialize()
        reqs = [Request(RawRequest("", n, p, sampling_params=(sampling or {}).get(i))) for i, (p, n) in enumerate(jobs)]
        eng.scheduler.on_requests_arrival(reqs)
        for _ in range(2000):
            if all(r.is_finished() for r in reqs):
                break
            assert await eng.step()
            if check is not None:
                check(eng, model)
        streamed = []
        for r in reqs:
            toks = []
            while not r.output_q.empty():
                toks.append(r.output_q.get_nowait().token_id)
            streamed.append(toks)
            assert r.finished_event.is_set()
        return eng, model, reqs, streamed
    return asyncio.run(run())


def _hold_streams(rule, jobs, reqs, streamed):
    for (prompt, n), r, s in zip(jobs, reqs, streamed):
        want = _expected(rule, prompt, n)
        assert r.error is None and r.output_token_ids == want           # never more than output_len tokens
        assert s == want                                                 # every token its own StepOutput, in order


@pytest.mark.parametrize("rule,name", [(periodic, "all"), (marker, "none"), (one_of_three, "one")])
def test_engine_streams_equal_the_plain_engine_and_counters_are_right(rule, name):
    jobs = [(p, 20 + 3 * i) for i, p in enumerate(_prompts(4, base=24))]      # prompt lengths 24, 30, 36, 42
    eng0, model0, reqs0, streamed0 = _run(_cfg(), rule, jobs)
    _hold_streams(rule, jobs, reqs0, streamed0)
    assert all(c[0] == "forward" for c in model0.calls) and eng0.num_verify_steps == 0
    eng, model, reqs, streamed = _run(_cfg(speculative_ngram=3), rule, jobs)
    _hold_streams(rule, jobs, reqs, streamed)
    assert eng.speculative_k == 3
    verifies = [c for c in model.calls if c[0] == "verify"]
    assert eng.num_verify_steps == len(verifies) > 0
    assert eng.num_forwards == len(model.calls)
    proposed = sum(len(ids) - 1 for c in verifies for ids in c[1])
    assert eng.num_draft_tokens == proposed > 0
    assert all(len(ids) <= 4 for c in verifies for ids in c[1])
    generated = sum(n for _, n in jobs)
    assert sum(len(s) for s in streamed) == generated
    if name == "all":
        assert eng.num_accepted_tokens == proposed
        assert len(model.calls) < len(model0.calls)                     # fewer forwards than the plain engine
    elif name == "none":
        assert eng.num_accepted_tokens == 0
        assert len(model.calls) == len(model0.calls)                    # nothing gained, nothing lost
    else:
        # every step that proposes three accepts exactly the first
        threes = [c for c in verifies if any(len(ids) == 4 for ids in c[1])]
        assert threes and 0 < eng.num_accepted_tokens < proposed
        assert eng.num_accepted_tokens == sum(1 for c in verifies for ids in c[1] if len(ids) > 1)
        assert len(model.calls) < len(model0.calls)
    # every request's blocks went back
    assert model.gpu_block_manager.held == {} and model0.gpu_block_manager.held == {}


def test_off_by_default_the_data_plane_sees_the_calls_of_always():
    jobs = [(p, 12) for p in _prompts(3)]
    _, model, _, _ = _run(_cfg(), periodic, jobs)
    assert model.calls and all(c[0] == "forward" for c in model.calls)
    for _, (input_ids, seq_ids, dec_lens), kwargs in model.calls:
        assert kwargs == {}                                             # the reference's three-argument call
        assert all(len(ids) == 1 for ids in input_ids[len(input_ids) - len(dec_lens):])
    # the first call is the prompts, then one token per request and step
    assert model.calls[0][1][0] == [p for p, _ in jobs] and len(model.calls) == 12


def test_a_sampled_request_or_a_large_batch_suppresses_the_step():
    jobs = [(p, 15) for p in _prompts(3)]
    sp = SamplingParams(temperature=0.8, seed=1)
    eng, model, reqs, _ = _run(_cfg(speculative_ngram=3), periodic, jobs, sampling={1: sp})
    assert eng.num_verify_steps == 0 and all(c[0] == "forward" for c in model.calls)
    assert all("sampling_params" in c[2] for c in model.calls)
    eng, model, reqs, streamed = _run(_cfg(speculative_ngram=3, speculative_max_batch=2), periodic, jobs)
    _hold_streams(periodic, jobs, reqs, streamed)
    assert eng.num_verify_steps == 0 and all(c[0] == "forward" for c in model.calls)
    # ... and verifies again once the batch has shrunk to the limit
    jobs = [(p, 8 + 12 * i) for i, p in enumerate(_prompts(3))]
    eng, model, reqs, streamed = _run(_cfg(speculative_ngram=3, speculative_max_batch=2), periodic, jobs)
    _hold_streams(periodic, jobs, reqs, streamed)
    assert eng.num_verify_steps > 0
    assert all(len(c[2]) <= 2 for c in model.calls if c[0] == "verify")


def test_effective_k_is_capped_by_the_model_and_clipped_by_the_budgets():
    jobs = [(p, 30) for p in _prompts(2)]

    async def run(cfg, max_draft):
        model = SpecModel(200, periodic, max_draft_tokens=max_draft)
        eng = Engine(cfg, model=model)
        await eng.initialize()
        return eng.speculative_k
    assert asyncio.run(run(_cfg(speculative_ngram=7), 3)) == 3
    assert asyncio.run(run(_cfg(speculative_ngram=2), 3)) == 2
    assert asyncio.run(run(_cfg(speculative_ngram=2), 0)) == 0
    # rows never pass max_tokens_in_batch: 2 requests, 5 rows
    eng, model, reqs, streamed = _run(_cfg(speculative_ngram=3, max_tokens_in_batch=64), periodic, jobs)
    _hold_streams(periodic, jobs, reqs, streamed)
    prompts_fit = max(len(p) for p, _ in jobs) <= 64
    assert prompts_fit and eng.num_verify_steps > 0
    eng, model, reqs, streamed = _run(_cfg(speculative_ngram=3, max_tokens_in_batch=47), periodic,
                                      [(_prompts(2)[0][:20], 30), (_prompts(2)[1][:20], 30)])
    assert all(sum(len(ids) for ids in c[1]) <= 47 for c in model.calls if c[0] == "verify")
    # positions never pass the rotary limit the engine knows
    async def limited():
        model = SpecModel(200, periodic)
        model._cos_cached = np.zeros((40, 4))
        eng = Engine(_cfg(speculative_ngram=3), model=model)
        await eng.initialize()
        req = Request(RawRequest("", 17, _prompts(1)[0]))        # 23 + 17 = 40 positions exactly
        eng.scheduler.on_requests_arrival([req])
        while not req.is_finished():
            assert await eng.step()
        return model, req
    model, req = asyncio.run(limited())
    assert req.output_token_ids == _expected(periodic, _prompts(1)[0], 17)
    assert all(ctx + len(ids) <= 40 for c in model.calls if c[0] == "verify" for ids, ctx in zip(c[1], c[3]))


def test_drafts_are_dropped_under_block_pressure_not_swapped():
    """Two requests at 30 and 31 tokens in a pool of exactly the blocks their plain decode needs: drafts that would claim
    a block are cut to what fits the blocks the requests hold, nothing is swapped, the fake pool never overflows."""
    prompts = [p[:30] for p in _prompts(2, base=40)]
    prompts[1] = prompts[1] + [901]
    jobs = [(prompts[0], 16), (prompts[1], 16)]                 # both end at 46 / 47 tokens: 3 blocks each
    eng, model, reqs, streamed = _run(_cfg(speculative_ngram=3), periodic, jobs, num_blocks=6)
    _hold_streams(periodic, jobs, reqs, streamed)
    assert eng.num_swapped_out == 0 and not [e for e in model.events if e[0] in ("in", "out")]
    assert eng.num_verify_steps > 0
    # a pool with no spare block at all while both hold two: drafts past the block edge were cut, not refused wholesale
    cut = [c for c in model.calls if c[0] == "verify" and any(len(ids) < 4 for ids in c[1])]
    assert cut


def test_scheduler_and_allocator_agree_after_rejections():
    """After every step: the fake allocator holds, for every running request, the blocks of max(resident tokens, reserved
    high-water mark), the scheduler counts max(num_tokens, reserved) — and at some step the mark is what decides."""
    seen = {"mark_decides": 0, "steps": 0}

    def check(eng, model):
        sch = eng.scheduler
        total = 0
        for r in sch.running_q:
            held = model.gpu_block_manager.num_allocated(r.request_id)
            assert held == -(-max(r.num_tokens() - 1, r.kv_reserved_tokens) // BS)
            assert sch._blocks(r) == -(-max(r.num_tokens(), r.kv_reserved_tokens) // BS) >= held
            total += sch._blocks(r)
            if -(-r.kv_reserved_tokens // BS) > -(-r.num_tokens() // BS):
                seen["mark_decides"] += 1
        assert sch._running_blocks() == total
        seen["steps"] += 1
    jobs = [(p, 40) for p in _prompts(3, base=27)]
    eng, model, reqs, streamed = _run(_cfg(speculative_ngram=3), one_of_three, jobs, check=check)
    _hold_streams(one_of_three, jobs, reqs, streamed)
    assert eng.num_accepted_tokens < eng.num_draft_tokens
    assert seen["mark_decides"] > 0 and seen["steps"] > 10
    assert model.gpu_block_manager.held == {}


# ---- allocator -------------------------------------------------------------------------------------------------------
def test_allocator_tolerates_a_surplus_block_only_for_sequences_that_verified():
    from swiftllm_amd.worker.block_manager import BlockAllocatorHost
    host = BlockAllocatorHost("GPU", 16, 8, 8, BS)
    host.plan_allocation([0, 1], [35, 35])                      # three blocks each (a verify step stored drafts up to 35)
    host.surplus_ok.add(0)
    needed, picked = host.plan_allocation([0], [31])            # rejected: the sequence is 31 tokens long again
    assert needed.tolist() == [0] and picked.size == 0 and host.num_allocated(0) == 3
    with pytest.raises(AssertionError, match="Logic error"):
        host.plan_allocation([1], [31])                         # a sequence that never verified: still a logic error
    needed, _ = host.plan_allocation([0], [50])                 # grows past the surplus as always
    assert needed.tolist() == [1] and host.num_allocated(0) == 4
    host.release([0])
    assert 0 not in host.surplus_ok and host.num_free_blocks == 13
    host.plan_allocation([0], [40])                             # the id's next owner starts without the mark
    with pytest.raises(AssertionError, match="Logic error"):
        host.plan_allocation([0], [20])
