"""Logits processing on the CPU: SamplingParams' new fields, the token history and the merged entries of a row, the layout
of the entry buffer, and how the engine, the scheduler and the HTTP layer carry stop tokens, min_tokens and the penalties."""
import asyncio
import math
import types
from collections import Counter

import numpy as np
import pytest

from swiftllm_amd import SamplingParams
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.server import Engine, RawRequest, Request
from swiftllm_amd.worker.kernels.logits_process import RowEdits, buffer_len, edit_capacity, pack_edits
from swiftllm_amd.worker.token_history import COUNT_MASK, TokenHistory, row_entries

INF = math.inf


def _cfg(**kw):
    base = dict(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=64,
                max_seqs_in_block_table=16, max_blocks_per_seq=64, max_batch_size=4, max_tokens_in_batch=100)
    base.update(kw)
    return EngineConfig(**base)


# ---- SamplingParams ------------------------------------------------------------------------------------------------------
def test_positional_construction_is_unchanged():
    sp = SamplingParams(0.7, 40, 0.9, 11)
    assert (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (0.7, 40, 0.9, 11)
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.min_p, sp.logit_bias, sp.stop_token_ids,
            sp.min_tokens) == (1.0, 0.0, 0.0, 0.0, None, (), 0)
    assert not sp.processes_logits and not sp.plain and not sp.greedy
    assert SamplingParams().plain and SamplingParams(0.0, 5, 0.5, 3).plain


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=INF), dict(repetition_penalty=math.nan),
    dict(repetition_penalty="1"), dict(repetition_penalty=True),
    dict(presence_penalty=INF), dict(presence_penalty=math.nan), dict(presence_penalty="0"), dict(presence_penalty=False),
    dict(frequency_penalty=-INF), dict(frequency_penalty=math.nan), dict(frequency_penalty=None),
    dict(min_p=-0.1), dict(min_p=1.0), dict(min_p=math.nan), dict(min_p="0.1"), dict(min_p=True),
    dict(logit_bias={1: INF}), dict(logit_bias={1: math.nan}), dict(logit_bias={-1: 0.0}), dict(logit_bias={"1": 0.0}),
    dict(logit_bias={1.5: 0.0}), dict(logit_bias={2 ** 31: 0.0}), dict(logit_bias=[(1, 0.0), (1, 2.0)]), dict(logit_bias=5),
    dict(logit_bias=[(1, 2, 3)]), dict(logit_bias={1: "x"}), dict(logit_bias={True: 1.0}),
    dict(stop_token_ids=(-1,)), dict(stop_token_ids=(1.0,)), dict(stop_token_ids=5), dict(stop_token_ids="12"),
    dict(stop_token_ids=(True,)),
    dict(min_tokens=-1), dict(min_tokens=1.0), dict(min_tokens=True),
])
def test_new_fields_are_validated(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw)


def test_new_fields_normalise_hash_and_classify():
    a = SamplingParams(logit_bias={7: 1, 3: -INF}, stop_token_ids=[5, 2])
    b = SamplingParams(logit_bias=[(3, -INF), (7, 1.0)], stop_token_ids=(5, 2))
    assert a.logit_bias == ((3, -INF), (7, 1.0)) and a.stop_token_ids == (5, 2)
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert SamplingParams(logit_bias={}).logit_bias is None and SamplingParams(logit_bias={}).plain
    for kw in (dict(repetition_penalty=1.2), dict(presence_penalty=0.1), dict(frequency_penalty=-0.1), dict(min_p=0.05),
               dict(logit_bias={1: 0.0}), dict(min_tokens=2, stop_token_ids=(1,))):
        sp = SamplingParams(**kw)
        assert sp.processes_logits and sp.greedy and not sp.plain, kw
    assert not SamplingParams(min_tokens=3).processes_logits and SamplingParams(min_tokens=3).plain
    stop = SamplingParams(stop_token_ids=(9,))
    assert not stop.processes_logits and not stop.plain and stop.greedy
    assert SamplingParams(0.5, min_p=0.1).processes_logits and not SamplingParams(0.5, min_p=0.1).greedy
    # the gap: T * ln(min_p) in double precision; off for min_p == 0 and for greedy rows
    assert SamplingParams(0.5, min_p=0.1).min_p_gap() == 0.5 * math.log(0.1)
    assert SamplingParams(0.5).min_p_gap() == -INF and SamplingParams(0.0, min_p=0.3).min_p_gap() == -INF


# ---- TokenHistory and the entries of a row ----------------------------------------------------------------------------------
def _brute(prompt, outputs):
    cnt, seen = Counter(outputs), set(prompt)
    return {t: (cnt[t], t in seen) for t in set(prompt) | set(outputs)}


def _as_dict(ids, meta):
    assert len(set(ids.tolist())) == len(ids)
    return {int(t): (int(m) & COUNT_MASK, int(m) < 0) for t, m in zip(ids, meta)}


def test_token_history_against_a_counter():
    rng = np.random.default_rng(0)
    prompt = rng.integers(0, 50, 300).tolist()
    outputs = rng.integers(30, 90, 500).tolist()
    h = TokenHistory(capacity=4)
    for lo in range(0, 300, 64):        # prompt chunks
        h.add_prompt(prompt[lo:lo + 64])
        assert len(h) == min(lo + 64, 300) and h.num_output == 0
    assert _as_dict(*h.entries()) == _brute(prompt, [])
    for k, t in enumerate(outputs):
        h.add_output(t)
        if k % 97 == 0:
            assert _as_dict(*h.entries()) == _brute(prompt, outputs[:k + 1])
    assert _as_dict(*h.entries()) == _brute(prompt, outputs)
    assert len(h) == 800 and h.num_prompt == 300 and h.num_output == 500
    ids, meta = h.entries()
    assert ids.dtype == np.int32 and meta.dtype == np.int32 and h.size == len(h.index)


def test_token_history_rollback():
    h = TokenHistory(capacity=2)
    h.add_prompt([5, 6, 5])
    h.add_output(6)
    before = (_as_dict(*h.entries()), h.mark(), dict(h.index))
    mark, words = h.mark(), []
    h.add_output(6, words)
    h.add_output(9, words)
    h.add_prompt([9, 10, 11, 5], words)         # (grows the arrays)
    assert h.size == 5 and len(h) == 10
    h.rollback(mark, words)
    assert (_as_dict(*h.entries()), h.mark(), dict(h.index)) == before
    h.add_output(9)
    assert _as_dict(*h.entries()) == {5: (0, True), 6: (1, True), 9: (1, False)}


def test_row_entries_merge_to_one_entry_per_id():
    h = TokenHistory()
    h.add_prompt([5, 6, 5])
    h.add_output(6)
    h.add_output(8)
    sp = SamplingParams(repetition_penalty=1.3, logit_bias={6: 2.0, 40: -1.0, 41: 3.0}, stop_token_ids=(8, 41, 99),
                        min_tokens=3)
    ids, meta, bias = row_entries(sp, h)
    got = {int(t): (int(m) & COUNT_MASK, int(m) < 0, float(b)) for t, m, b in zip(ids, meta, bias)}
    assert len(got) == len(ids) == 6
    assert got == {5: (0, True, 0.0), 6: (1, True, 2.0), 8: (1, False, -INF), 40: (0, False, -1.0), 41: (0, False, -INF),
                   99: (0, False, -INF)}
    h.add_output(7)             # three output tokens: the ban is over, the bias of 41 is back
    ids, meta, bias = row_entries(sp, h)
    got = {int(t): float(b) for t, b in zip(ids, bias)}
    assert got == {5: 0.0, 6: 2.0, 8: 0.0, 7: 0.0, 40: -1.0, 41: 3.0}
    # no penalty: the history's tokens are not entries
    ids, meta, bias = row_entries(SamplingParams(logit_bias={6: 2.0}, stop_token_ids=(8,), min_tokens=9), h)
    assert sorted(zip(ids.tolist(), meta.tolist(), bias.tolist())) == [(6, 0, 2.0), (8, 0, -INF)]
    ids, _, _ = row_entries(SamplingParams(0.7, min_p=0.1), h)
    assert ids.size == 0
    ids, _, bias = row_entries(SamplingParams(presence_penalty=0.5), h)
    assert ids.tolist() == [5, 6, 8, 7] and not bias.any()


def test_pack_edits_layout():
    rows = [RowEdits(np.array([3, 9], np.int32), np.array([1, -2 ** 31], np.int32), np.array([0.5, -INF], np.float32),
                     1.3, 0.25, 0.125, -2.0),
            None,
            RowEdits(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), min_p_gap=-1.5),
            RowEdits(np.array([7], np.int32), np.array([4], np.int32), np.array([-3.0], np.float32))]
    cap, rows_cap = 5, 6
    buf = np.full(buffer_len(rows_cap, cap), -7, dtype=np.int32)
    assert buf.size == 5 * 6 + 1 + 15 and edit_capacity(buf.size, rows_cap) == cap
    assert pack_edits(rows, buf, rows_cap, vocab_size=10) == 3
    assert buf[:7].tolist() == [0, 2, 2, 2, 3, 3, 3]                # CSR offsets; rows past the batch: empty
    params = buf[7:31].view(np.float32).reshape(6, 4)
    assert params.tolist() == [[np.float32(1.3), 0.25, 0.125, -2.0], [1.0, 0.0, 0.0, -INF], [1.0, 0.0, 0.0, -1.5],
                               [1.0, 0.0, 0.0, -INF], [1.0, 0.0, 0.0, -INF], [1.0, 0.0, 0.0, -INF]]
    assert buf[31:34].tolist() == [3, 9, 7] and buf[36:39].tolist() == [1, -2 ** 31, 4]
    assert buf[41:44].view(np.float32).tolist() == [0.5, -INF, -3.0]
    assert buf[34:36].tolist() == [-7, -7]                          # past the entries: not written
    bad = lambda ids: [RowEdits(np.array(ids, np.int32), np.zeros(len(ids), np.int32), np.zeros(len(ids), np.float32))]
    for ids in ([10], [-1], [4, 4]):
        with pytest.raises(ValueError):
            pack_edits(bad(ids), buf, rows_cap, vocab_size=10)
    with pytest.raises(ValueError):
        pack_edits(bad([1, 2, 3, 4, 5, 6]), buf, rows_cap)          # more entries than the buffer holds
    with pytest.raises(ValueError):
        pack_edits([None] * 7, buf, rows_cap)
    with pytest.raises(ValueError):
        pack_edits(rows, buf[::2], 1)                               # a non-contiguous buffer


# ---- engine, scheduler and HTTP over a fake data plane ---------------------------------------------------------------------
class ThreeArgModel:
    num_blocks = 8

    def __init__(self):
        self.model_config = types.SimpleNamespace(vocab_size=97)
        self.calls = 0
        self.freed = []

    def forward(self, input_ids, seq_ids, decoding_lens):
        self.calls += 1
        return [len(x) % 97 for x in input_ids]

    def swap_in_seqs(self, ids):
        pass

    def swap_out_seqs(self, ids):
        pass

    def free_seqs_resources(self, ids):
        self.freed += list(ids)


class CountingModel(ThreeArgModel):
    """The token of a sequence is its length % 97 (prompt 3: 3, 4, 5, ...), unless its params ban it through min_tokens,
    in which case it is 96: what a data plane that honours the ban would do. Records every call's params."""

    def __init__(self):
        super().__init__()
        self.seen = []
        self.verify_calls = 0
        self.max_draft_tokens = 3
        self.cycle = None       # set: the token at length n is cycle[n % len(cycle)] (a stream the n-gram proposer drafts)

    def forward(self, input_ids, seq_ids, decoding_lens, sampling_params=None):
        n_pre = len(input_ids) - len(decoding_lens)
        lens = [len(x) for x in input_ids[:n_pre]] + list(decoding_lens)
        sps = sampling_params or [None] * len(input_ids)
        out = []
        for sid, n, sp, ids in zip(seq_ids, lens, sps, input_ids):
            self.seen.append((sid, n, sp))
            tok = n % 97 if self.cycle is None else self.cycle[n % len(self.cycle)]
            prompt = 3
            if sp is not None and tok in sp.stop_token_ids and n - prompt < sp.min_tokens:
                tok = 96
            out.append(tok)
        return out

    def forward_verify(self, input_ids, seq_ids, ctx_lens):
        self.verify_calls += 1
        tok = (lambda n: n % 97) if self.cycle is None else (lambda n: self.cycle[n % len(self.cycle)])
        return [[tok(c + 1 + k) for k in range(len(ids))] for ids, c in zip(input_ids, ctx_lens)]


def _run(model, raws, **cfg):
    async def run():
        eng = Engine(_cfg(**cfg), model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        done = await asyncio.wait_for(asyncio.gather(*(eng.add_request_and_wait(r) for r in raws)), timeout=20)
        loops.cancel()
        return eng, done
    return asyncio.run(run())


def test_request_keeps_params_that_ask_for_something():
    assert Request(RawRequest("", 2, [1], sampling_params=SamplingParams())).sampling_params is None
    assert Request(RawRequest("", 2, [1], sampling_params=SamplingParams(0.0, top_k=4))).sampling_params is None
    pen = SamplingParams(repetition_penalty=1.2)
    r = Request(RawRequest("", 2, [1], sampling_params=pen))
    assert r.sampling_params is pen and r.sampling_params.seed is None      # greedy: no seed to resolve
    stop = SamplingParams(stop_token_ids=(4,))
    assert Request(RawRequest("", 2, [1], sampling_params=stop)).sampling_params is stop
    assert Request(RawRequest("", 2, [1], sampling_params=SamplingParams(0.5, min_p=0.1))).sampling_params.seed is not None


def test_is_finished_on_stop_tokens_and_min_tokens():
    r = Request(RawRequest("", 10, [1], sampling_params=SamplingParams(stop_token_ids=(4, 6))))
    r.output_token_ids += [5, 7]
    assert not r.is_finished()
    r.output_token_ids.append(6)
    assert r.is_finished()
    r = Request(RawRequest("", 4, [1], sampling_params=SamplingParams(stop_token_ids=(4,), min_tokens=2)))
    r.output_token_ids += [4, 4]            # (a data plane that ignores the ban: the request does not end on them)
    assert not r.is_finished()
    r.output_token_ids.append(4)
    assert r.is_finished()
    r = Request(RawRequest("", 2, [1]))
    r.output_token_ids += [4, 4]
    assert r.is_finished()


def test_engine_stops_on_the_stop_token_delivers_it_and_frees_the_sequence():
    model = CountingModel()
    stop = RawRequest("", 20, [1, 2, 3], sampling_params=SamplingParams(stop_token_ids=(50, 7)))
    full = RawRequest("", 6, [1, 2, 3])
    eng, ((rs, ts), (rf, tf)) = _run(model, [stop, full])
    assert ts == [3, 4, 5, 6, 7] and tf == [3, 4, 5, 6, 7, 8]
    assert rs.error is None and rs.is_finished() and sorted(model.freed) == [0, 1]
    assert not eng.scheduler.has_work()
    assert all(sp is None for sid, _, sp in model.seen if sid == rf.request_id)
    assert {sp for sid, _, sp in model.seen if sid == rs.request_id} == {stop.sampling_params}


def test_engine_min_tokens():
    model = CountingModel()
    sp = SamplingParams(stop_token_ids=(5, 9), min_tokens=4)
    _, ((r, toks),) = _run(model, [RawRequest("", 20, [1, 2, 3], sampling_params=sp)])
    # 3, 4, then 5 is banned (two tokens so far), 6; 7 and 8 are free; 9 ends it
    assert toks == [3, 4, 96, 6, 7, 8, 9] and model.freed == [r.request_id]
    _, ((r, toks),) = _run(model, [RawRequest("", 5, [1, 2, 3], sampling_params=SamplingParams(stop_token_ids=(60,)))])
    assert toks == [3, 4, 5, 6, 7]          # no stop token met: output_len ends it


def test_streaming_ends_at_the_stop_token():
    model = CountingModel()

    async def run():
        eng = Engine(_cfg(), model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        raw = RawRequest("", 20, [1, 2, 3], sampling_params=SamplingParams(stop_token_ids=(6,)))

        async def collect():
            return [s.token_id async for s in eng.add_request_and_stream(raw)]
        toks = await asyncio.wait_for(collect(), timeout=20)
        loops.cancel()
        return toks
    assert asyncio.run(run()) == [3, 4, 5, 6]


def test_plain_batches_keep_the_three_argument_call():
    model = ThreeArgModel()
    _, done = _run(model, [RawRequest("", 3, [1, 2]), RawRequest("", 2, [5], sampling_params=SamplingParams()),
                           RawRequest("", 2, [6, 6], sampling_params=SamplingParams(0.0, min_tokens=5))])
    assert model.calls > 0 and all(req.error is None for req, _ in done)


def test_penalised_greedy_request_keeps_its_params_and_is_never_speculated():
    pen = SamplingParams(repetition_penalty=1.5, frequency_penalty=0.2)
    prompt = [1, 2, 3] * 4          # a prompt the n-gram proposer finds drafts in
    model = CountingModel()
    model.cycle = [1, 2, 3]
    eng, ((r, toks),) = _run(model, [RawRequest("", 8, prompt, sampling_params=pen)], speculative_ngram=3)
    assert toks == [1, 2, 3, 1, 2, 3, 1, 2] and model.verify_calls == 0 and eng.num_verify_steps == 0
    assert [sp for _, _, sp in model.seen] == [pen] * 8
    # the same engine does speculate for a plain request with that prompt
    model = CountingModel()
    model.cycle = [1, 2, 3]
    eng, ((r, toks),) = _run(model, [RawRequest("", 8, prompt)], speculative_ngram=3)
    assert toks == [1, 2, 3, 1, 2, 3, 1, 2] and eng.speculative_k == 3 and model.verify_calls > 0


def test_scheduler_refuses_ids_outside_the_vocabulary():
    model = CountingModel()
    raws = [RawRequest("", 3, [1, 2, 3], sampling_params=SamplingParams(logit_bias={97: 1.0})),
            RawRequest("", 3, [1, 2, 3], sampling_params=SamplingParams(stop_token_ids=(3, 200))),
            RawRequest("", 3, [1, 2, 3], sampling_params=SamplingParams(logit_bias={96: 1.0}, stop_token_ids=(96,)))]
    _, done = _run(model, raws)
    assert "logit_bias" in done[0][0].error and done[0][1] == []
    assert "stop_token_ids" in done[1][0].error and done[1][1] == []
    assert done[2][0].error is None and len(done[2][1]) == 3


def _client(model):
    from swiftllm_amd.server.api_server import build_app

    async def boot():
        eng = Engine(_cfg(), model=model)
        await eng.initialize()
        return eng
    eng = asyncio.new_event_loop().run_until_complete(boot())
    app = build_app(eng)

    @app.on_event("startup")
    async def start_loops():
        eng.event_loop = asyncio.get_running_loop()
        asyncio.ensure_future(eng.start_all_event_loops())
    return app


def test_api_fields():
    from fastapi.testclient import TestClient
    model = CountingModel()
    base = {"prompt_token_ids": [1, 2, 3], "output_len": 6}
    with TestClient(_client(model)) as client:
        for bad in (dict(repetition_penalty=0), dict(repetition_penalty=-2), dict(repetition_penalty="1.1"),
                    dict(repetition_penalty=True), dict(presence_penalty="x"), dict(presence_penalty=[1]),
                    dict(frequency_penalty="0"), dict(frequency_penalty=False), dict(min_p=1), dict(min_p=-0.5),
                    dict(min_p="0.1"), dict(logit_bias=[1, 2]), dict(logit_bias={"a": 1}), dict(logit_bias={"-1": 1}),
                    dict(logit_bias={"1.5": 1}), dict(logit_bias={"1": "x"}), dict(logit_bias={"1": None}),
                    dict(logit_bias={"1": True}), dict(logit_bias={"1": 1, "01": 2}), dict(logit_bias={"99999999999": 1}),
                    dict(stop_token_ids=5), dict(stop_token_ids=[1.5]), dict(stop_token_ids=[-1]),
                    dict(stop_token_ids=["1"]), dict(stop_token_ids=[True]), dict(min_tokens=-1), dict(min_tokens=1.5),
                    dict(min_tokens="2"), dict(min_tokens=True),
                    dict(logit_bias={"97": 1.0}), dict(stop_token_ids=[97])):      # (the scheduler's: outside the vocabulary)
            r = client.post("/generate", json={**base, **bad})
            assert r.status_code == 400 and "error" in r.json(), bad
        # numbers too large for a float, a key too long for int(): a 400 like any other bad field, not an exception
        huge = "1" + "0" * 400
        for field in ("presence_penalty", "frequency_penalty", "repetition_penalty", "min_p", "temperature", "top_p"):
            raw = '{"prompt_token_ids": [1, 2, 3], "output_len": 6, "%s": %s}' % (field, huge)
            r = client.post("/generate", content=raw, headers={"content-type": "application/json"})
            assert r.status_code == 400, field
        for raw_bias in ('{"%s": 1}' % ("9" * 5000), '{"": 1}', '{"5": %s}' % huge):
            raw = '{"prompt_token_ids": [1, 2, 3], "output_len": 6, "logit_bias": %s}' % raw_bias
            r = client.post("/generate", content=raw, headers={"content-type": "application/json"})
            assert r.status_code == 400, raw_bias[:20]
        raw_inf = '{"prompt_token_ids": [1, 2, 3], "output_len": 6, "logit_bias": {"1": -Infinity}}'
        r = client.post("/generate", content=raw_inf, headers={"content-type": "application/json"})
        assert r.status_code == 400         # finite numbers only over HTTP
        body = {**base, "repetition_penalty": 1.2, "presence_penalty": 0.5, "frequency_penalty": -0.25, "min_p": 0.05,
                "temperature": 0.5, "seed": 4, "logit_bias": {"7": -3, "2": 1.5}, "stop_token_ids": [5], "min_tokens": 1}
        r = client.post("/generate", json=body)
        assert r.status_code == 200 and r.json() == {"output_token_ids": [3, 4, 5]}
        r = client.post("/generate", json={**body, "stream": True})
        assert [int(x) for x in r.text.split()] == [3, 4, 5]
        want = SamplingParams(0.5, seed=4, repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=-0.25, min_p=0.05,
                              logit_bias={2: 1.5, 7: -3.0}, stop_token_ids=(5,), min_tokens=1)
        assert want in {sp for _, _, sp in model.seen}
        # a body with none of the new fields builds the params it built before
        model.seen.clear()
        assert client.post("/generate", json=base).status_code == 200
        assert client.post("/generate", json={**base, "temperature": 0.5, "seed": 1}).status_code == 200
        assert {sp for _, _, sp in model.seen} == {None, SamplingParams(0.5, seed=1)}


def test_router_forwards_the_new_fields_unchanged():
    import socket
    import threading
    import time
    import fastapi
    import uvicorn
    from fastapi.responses import JSONResponse
    from fastapi.testclient import TestClient
    from swiftllm_amd.server.router import ReplicaRouter, build_app

    got = []
    app = fastapi.FastAPI()

    @app.post("/generate")
    async def generate(req: fastapi.Request):
        got.append(await req.json())
        return JSONResponse({"output_token_ids": [1]})
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    server = uvicorn.Server(uvicorn.Config(app, host="127.0.0.1", port=port, log_level="error"))
    threading.Thread(target=server.run, daemon=True).start()
    deadline = time.time() + 10
    while not server.started:
        assert time.time() < deadline, "the fake replica did not start"
        time.sleep(0.02)
    try:
        body = {"prompt_token_ids": [1, 2], "output_len": 1, "repetition_penalty": 1.1, "presence_penalty": 0.5,
                "frequency_penalty": 0.25, "min_p": 0.1, "logit_bias": {"5": -2.5}, "stop_token_ids": [3, 4], "min_tokens": 2}
        with TestClient(build_app(ReplicaRouter([f"http://127.0.0.1:{port}"]))) as client:
            assert client.post("/generate", json=body).json() == {"output_token_ids": [1]}
        assert got == [body]
    finally:
        server.should_exit = True
