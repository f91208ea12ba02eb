"""Chunked prefill on the CPU: the batch plan with resident contexts, the scheduler / engine feeding a prompt in
pieces (recording fake data plane), and the argument validation of the three new C entry points (no device needed)."""
import asyncio
import ctypes
import dataclasses
import types

import numpy as np
import pytest

from swiftllm_amd import _hip
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.server import Engine, RawRequest, Request, Scheduler
from swiftllm_amd.worker.batch_plan import plan_batch


# ---- plan ------------------------------------------------------------------------------------------------------------
def test_plan_batch_with_contexts_by_hand():
    # two prompt chunks (3 tokens behind 5 resident ones; 2 tokens behind 0) and one decode of length 9
    plan = plan_batch([[7, 8, 9], [1, 2], [4]], [3, 0, 6], [9], num_kv_heads=2, prefill_ctx_lens=[5, 0])
    assert plan.position_indices.tolist() == [5, 6, 7, 0, 1, 8]
    assert plan.seq_lengths.tolist() == [8, 2, 9] and plan.seq_lengths_list == [8, 2, 9]
    assert plan.prefill_seq_lens.tolist() == [3, 2]                     # NEW tokens: what the kernels walk
    assert plan.prefill_start_locs_with_end.tolist() == [0, 3, 5]
    assert plan.last_token_indices.tolist() == [2, 4, 5]               # unchanged by a context
    assert plan.prefill_ctx_lens.dtype == np.int32 and plan.prefill_ctx_lens.tolist() == [5, 0]
    assert plan.max_prefill_len == 3 and plan.max_prefill_total_len == 8
    assert plan.num_prefill_tokens == 5 and plan.num_tokens == 6
    layout, total = plan.packed_layout()
    assert layout[-1][0] == "prefill_ctx_lens" and layout[-1][2] == 2
    buf = np.full(total, -1, dtype=np.int32)
    assert plan.pack_into(buf) == total
    off = layout[-1][1]
    assert buf[off:off + 2].tolist() == [5, 0]
    with pytest.raises(ValueError):
        plan_batch([[1, 2], [3]], [0, 1], [4], 2, prefill_ctx_lens=[1, 2])      # one entry per PREFILL sequence
    with pytest.raises(ValueError):
        plan_batch([[1, 2]], [0], [], 2, prefill_ctx_lens=[-1])


def test_plan_batch_without_contexts_is_the_plan_of_always():
    args = ([[7, 8, 9], [1, 2], [4]], [3, 0, 6], [9])
    plain = plan_batch(*args, num_kv_heads=2)
    again = plan_batch(*args, num_kv_heads=2, prefill_ctx_lens=None)
    assert plain.prefill_ctx_lens is None and again.prefill_ctx_lens is None
    zero = plan_batch(*args, num_kv_heads=2, prefill_ctx_lens=[0, 0])
    for f in dataclasses.fields(plain):
        a, b, z = getattr(plain, f.name), getattr(again, f.name), getattr(zero, f.name)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and np.array_equal(a, b), f.name
            assert np.array_equal(a, z), f.name
        elif f.name != "prefill_ctx_lens":
            assert a == b == z, f.name
    assert [n for n, _, _ in plain.packed_layout()[0]] == list(plain.SEGMENTS)      # no segment without contexts
    # the segments of a plan with contexts sit where they always sat; the new one comes after them
    assert zero.packed_layout()[0][:len(plain.SEGMENTS)] == plain.packed_layout()[0]
    assert plain.position_indices.tolist() == [0, 1, 2, 0, 1, 8] and plain.max_prefill_total_len == 3


# ---- scheduler + engine over a recording fake data plane --------------------------------------------------------------
def _cfg(**kw):
    base = dict(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=512,
                max_seqs_in_block_table=16, max_blocks_per_seq=256, max_batch_size=8, max_tokens_in_batch=1024)
    base.update(kw)
    return EngineConfig(**base)


class RecordingModel:
    """Deterministic and chunk-invariant: the token after a sequence is (sum of all its tokens + its length) % 97,
    whatever pieces the tokens arrived in. Keeps what it was fed, per sequence and per call."""

    def __init__(self, num_blocks):
        self.model_config = types.SimpleNamespace()
        self.num_blocks = num_blocks
        self.state = {}         # seq id -> [sum, length]
        self.calls = []         # per forward: dict(prefill=[(seq, ids, ctx)], decode=[seq...])
        self.events = []        # ("out" / "in" / "free", ids) and ("fwd", index into calls)

    def forward(self, input_ids, seq_ids, decoding_lens, sampling_params=None, prefill_ctx_lens=None):
        n_prefill = len(input_ids) - len(decoding_lens)
        ctx = list(prefill_ctx_lens) if prefill_ctx_lens is not None else [0] * n_prefill
        assert len(ctx) == n_prefill
        call = dict(prefill=[], decode=[])
        out = []
        for i, (ids, sid) in enumerate(zip(input_ids, seq_ids)):
            if i < n_prefill:
                st = self.state.setdefault(sid, [0, 0])
                assert ctx[i] == st[1], f"sequence {sid}: context {ctx[i]} but {st[1]} tokens were forwarded before"
                call["prefill"].append((sid, list(ids), ctx[i]))
            else:
                st = self.state[sid]
                assert len(ids) == 1 and decoding_lens[i - n_prefill] == st[1] + 1
                call["decode"].append(sid)
            st[0] += sum(ids)
            st[1] += len(ids)
            out.append((st[0] + st[1]) % 97)
        self.events.append(("fwd", len(self.calls)))
        self.calls.append(call)
        return out

    def swap_in_seqs(self, ids):
        self.events.append(("in", list(ids)))

    def swap_out_seqs(self, ids):
        self.events.append(("out", list(ids)))

    def free_seqs_resources(self, ids):
        self.events.append(("free", list(ids)))
        for i in ids:
            self.state.pop(i, None)


def _expected(prompt, n):
    s, length, out = sum(prompt), len(prompt), []
    for _ in range(n):
        tok = (s + length) % 97
        out.append(tok)
        s += tok
        length += 1
    return out


def _serve(cfg, num_blocks, jobs, piggyback=True):
    """jobs: [(prompt, output_len)], all submitted at once, in order. Returns (model, [(request, tokens)])."""
    async def run():
        model = RecordingModel(num_blocks)
        eng = Engine(cfg, model=model, piggyback=piggyback)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        waits = [asyncio.ensure_future(eng.add_request_and_wait(RawRequest("", n, p))) for p, n in jobs]
        done = await asyncio.wait_for(asyncio.gather(*waits), timeout=60)
        loops.cancel()
        return model, done
    return asyncio.run(run())


def _jobs():
    rng = np.random.RandomState(3)
    shapes = [(20, 30), (37, 25), (3000, 6), (300, 5), (5, 12), (700, 3)]       # (prompt tokens, tokens to generate)
    return [(rng.randint(0, 1000, size=n).tolist(), m) for n, m in shapes]


@pytest.mark.parametrize("piggyback", [True, False])
def test_long_prompt_is_fed_in_chunks_among_short_ones_and_decodes(piggyback):
    jobs = _jobs()
    model, done = _serve(_cfg(max_prefill_chunk=256), 400, jobs, piggyback)
    # outputs: the closed form of the deterministic model, for every request (the 3 000-token one included)
    for (req, toks), (prompt, n) in zip(done, jobs):
        assert req.error is None and toks == _expected(prompt, n)
        assert req.num_prefilled == len(prompt) and req.is_prompt_resident()
    # every prompt token forwarded exactly once and in order; a chunk's context = the tokens forwarded before it (the
    # model asserts that on every call)
    fed, first_seen = {}, []
    ids_of = {}
    for call in model.calls:
        prompt_tokens = sum(len(ids) for _, ids, _ in call["prefill"])
        assert prompt_tokens <= 256                                            # the chunk cap, in total per step
        assert prompt_tokens + len(call["decode"]) <= 1024                     # max_tokens_in_batch
        for sid, ids, ctx in call["prefill"]:
            key = (sid, ctx == 0 and len(ids_of.get(sid, [])))                 # (ids are reused after a request ends)
            if ctx == 0:
                ids_of.setdefault(sid, []).append([])
                first_seen.append(ids)
            ids_of[sid][-1].extend(ids)
            del key
    streams = [s for lst in ids_of.values() for s in lst]
    for prompt, _ in jobs:
        assert sum(1 for s in streams if s == prompt) == 1
    assert len(streams) == len(jobs)
    # arrival order: first chunks appear in the order the requests were submitted
    assert [f[:5] for f in first_seen] == [p[:5] for p, _ in jobs]
    # the 3 000-token prompt took ceil(3000 / 256) or more steps, and decodes rode along with its chunks
    long_calls = [c for c in model.calls if any(len(ids) + ctx > 256 or (len(ids) == 256 and ctx > 0)
                                                for _, ids, ctx in c["prefill"])]
    assert len(long_calls) >= 11
    mixed = [c for c in model.calls if c["prefill"] and c["decode"]]
    assert bool(mixed) == piggyback
    if piggyback:
        assert sum(1 for c in long_calls if c["decode"]) >= 10                 # decodes progress during the long prefill


def test_chunking_off_refuses_the_long_prompt_and_serves_the_rest_identically():
    jobs = _jobs()
    _, on = _serve(_cfg(max_prefill_chunk=256), 400, jobs)
    model, off = _serve(_cfg(), 400, jobs)
    for (r_on, t_on), (r_off, t_off), (prompt, n) in zip(on, off, jobs):
        if len(prompt) > 1024:
            assert r_off.error is not None and "max_tokens_in_batch" in r_off.error and t_off == []
            assert r_on.error is None and len(t_on) == n
        else:
            assert r_off.error is None and t_on == t_off == _expected(prompt, n)
    # off: a prompt is one forward, no context is ever passed
    assert all(ctx == 0 for c in model.calls for _, _, ctx in c["prefill"])


def test_why_unservable_with_and_without_chunking():
    big = Request(RawRequest("", 4, list(range(3000))))
    assert "max_tokens_in_batch" in Scheduler(None, _cfg(), 400).why_unservable(big)
    on = Scheduler(None, _cfg(max_prefill_chunk=256), 400)
    assert on.why_unservable(big) is None
    # every other refusal stays
    assert "KV blocks" in Scheduler(None, _cfg(max_prefill_chunk=256), 100).why_unservable(big)
    assert on.why_unservable(Request(RawRequest("", 4, []))) == "empty prompt"
    assert on.why_unservable(Request(RawRequest("", 0, [1]))) == "output_len must be positive"
    with pytest.raises(ValueError):
        _cfg(max_prefill_chunk=-1)
    assert _cfg().max_prefill_chunk == 0


def test_chunk_cap_is_the_smaller_of_the_two_limits():
    s = Scheduler(None, _cfg(max_prefill_chunk=4096, max_tokens_in_batch=100), 400)
    r = Request(RawRequest("", 2, list(range(250))))
    s.on_requests_arrival([r])
    batch, _, _ = s.get_next_batch()
    assert batch == [r] and r.prefill_take == 100 and r.request_id == 0
    assert r in s.running_q and not r.is_prompt_resident() and r.is_prefill_stage()


def test_swapped_out_partly_prefilled_request_resumes_at_its_offset():
    """A decoding request outgrows a pool that holds it and a 600-token prompt being fed in chunks of 256: the prompt
    (most recently admitted) is swapped out after its first chunk, waits for the pool, swaps in and continues where it was."""
    rng = np.random.RandomState(5)
    a = rng.randint(0, 1000, size=31).tolist()
    b = rng.randint(0, 1000, size=600).tolist()
    model, done = _serve(_cfg(max_prefill_chunk=256), 40, [(a, 40), (b, 4)])
    assert [t for _, t in done] == [_expected(a, 40), _expected(b, 4)]
    b_chunks = [(i, ctx, len(ids)) for i, c in enumerate(model.calls) for _, ids, ctx in c["prefill"] if len(ids) > 31
                or ctx > 0]
    # (both arrive together: the first step carries all of a and the first 225 tokens of b)
    assert [(ctx, n) for _, ctx, n in b_chunks] == [(0, 225), (225, 256), (481, 119)]
    ev = model.events
    out_at = next(i for i, e in enumerate(ev) if e[0] == "out")
    in_at = next(i for i, e in enumerate(ev) if e[0] == "in")
    assert ev[out_at][1] == ev[in_at][1] and len(ev[out_at][1]) == 1
    fwd_index = {e[1]: i for i, e in enumerate(ev) if e[0] == "fwd"}
    # (a's decode crosses into its third block while riding with b's second chunk) two chunks before the swap-out, the
    # last one — at context 481 — only after the swap-in
    assert fwd_index[b_chunks[1][0]] < out_at < in_at < fwd_index[b_chunks[2][0]]


# ---- ABI without a device -------------------------------------------------------------------------------------------
def test_new_entry_points_validate_before_any_launch():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16          # non-null, 16-byte aligned (never dereferenced: no launch)
    F = _hip.SWL_F16

    def attn(o=p, q=p, kc=p, vc=p, bt=p, ids=p, cu=p, ctx=p, n=1, max_new=4, max_total=8, H=4, KVH=2, D=64, L=2, bs=16,
             layer=1, mbps=8, qs=256, os_=256, dt=F):
        return lib.swl_prefill_attn_paged(o, q, kc, vc, bt, ids, cu, ctx, n, max_new, max_total, H, KVH, D, L, bs, layer,
                                          mbps, 0.125, qs, os_, dt, None)

    def store(kc=p, vc=p, k=p, v=p, bt=p, ids=p, st=p, ln=p, ctx=p, n=1, max_len=4, D=64):
        return lib.swl_store_kv_prefill_at(kc, vc, k, v, bt, ids, st, ln, ctx, n, max_len, 1, 2, 2, 16, D, 8, 128, 128, F,
                                           None)

    def rstore(q=p, k=p, v=p, cos=p, sin=p, kc=p, ctx=p, n=1, max_len=4, D=64):
        return lib.swl_rotary_store_kv_prefill_at(q, k, v, cos, sin, None, kc, p, p, p, p, p, ctx, n, max_len, 1, 2, 4, 2,
                                                  16, D, 8, 256, 128, 128, F, None)

    # zero-size calls: SWL_OK, nothing launched, pointers not looked at
    assert attn(None, None, None, None, None, None, None, None, n=0) == 0
    assert attn(max_new=0, max_total=0) == 0
    assert store(None, None, None, None, None, None, None, None, None, n=0) == 0 and store(max_len=0) == 0
    assert rstore(None, None, None, None, None, None, None, n=0) == 0 and rstore(max_len=0) == 0
    # nulls, negative sizes, misalignment: SWL_ERR_BAD_ARG
    assert attn(ctx=None) == -1 and attn(kc=None) == -1 and attn(bt=None) == -1 and attn(o=None) == -1
    assert attn(n=-1) == -1 and attn(max_new=-1) == -1 and attn(q=p + 2) == -1 and attn(qs=252) == -1
    assert attn(H=5) == -1 and attn(layer=2) == -1 and attn(dt=7) == -1
    assert attn(max_total=200, mbps=8) == -1            # a table row cannot hold the longest sequence
    assert attn(max_new=9, max_total=8) == -1
    assert store(ctx=None) == -1 and store(kc=None) == -1 and store(n=-1) == -1 and store(k=p + 2) == -1
    assert rstore(ctx=None) == -1 and rstore(q=None) == -1 and rstore(cos=None) == -1 and rstore(n=-1) == -1
    # shapes the kernels are not built for: SWL_ERR_UNSUPPORTED
    assert attn(D=48) == -2 and attn(D=256) == -2 and attn(bs=32, mbps=8) == -2
    assert store(D=20) == -2 and rstore(D=48) == -2
    with pytest.raises(_hip.HipLibraryError):
        _hip.call("swl_prefill_attn_paged", p, p, p, p, p, p, p, p, 1, 4, 8, 4, 2, 48, 2, 16, 1, 8, 0.125, 256, 256, F, None)
