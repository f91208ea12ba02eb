"""Per-token logprobs on the CPU: SamplingParams.logprobs, the request and engine bookkeeping over a recording fake data
plane that sets `last_logprobs`, and the HTTP field and answer forms (no device needed)."""
import asyncio
import json
import math
import types

import numpy as np
import pytest

from swiftllm_amd import SamplingParams, TokenLogprob
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.server import Engine, RawRequest, Request
from swiftllm_amd.server.structs import StepOutput


def _cfg(**kw):
    base = dict(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=512,
                max_seqs_in_block_table=16, max_blocks_per_seq=256, max_batch_size=8, max_tokens_in_batch=1024)
    base.update(kw)
    return EngineConfig(**base)


# ---- SamplingParams and Request ---------------------------------------------------------------------------------------
def test_logprobs_field_is_validated():
    assert SamplingParams().logprobs is None
    for n in (0, 1, 5, 20):
        assert SamplingParams(logprobs=n).logprobs == n
    for bad in (-1, 21, 1.0, "3", True, False, [1], 2 ** 31):
        with pytest.raises(ValueError):
            SamplingParams(logprobs=bad)
    assert SamplingParams(0.7, 40, 0.9, 11) == SamplingParams(0.7, 40, 0.9, 11, logprobs=None)    # positional use stays


def test_logprobs_make_params_not_plain_and_nothing_else():
    sp = SamplingParams(logprobs=0)
    assert not sp.plain and sp.greedy and not sp.processes_logits and not sp.penalised
    assert SamplingParams().plain and SamplingParams(0.0, top_k=4).plain
    hot = SamplingParams(0.8, seed=3, logprobs=4)
    assert not hot.greedy and not hot.processes_logits and not hot.plain
    assert SamplingParams(repetition_penalty=1.2, logprobs=2).processes_logits
    assert hash(SamplingParams(logprobs=2)) != hash(SamplingParams(logprobs=3)) or SamplingParams(logprobs=2) != SamplingParams(logprobs=3)


def test_request_keeps_params_that_ask_for_logprobs():
    sp = SamplingParams(logprobs=0)
    r = Request(RawRequest("", 2, [1], sampling_params=sp))
    assert r.sampling_params is sp and r.output_logprobs == []
    assert Request(RawRequest("", 2, [1], sampling_params=SamplingParams())).sampling_params is None
    hot = Request(RawRequest("", 2, [1], sampling_params=SamplingParams(0.5, logprobs=3))).sampling_params
    assert hot.seed is not None and hot.logprobs == 3
    out = StepOutput(5, r)
    assert out.logprobs is None and StepOutput(5, r, TokenLogprob(5, -0.5, 1)).logprobs.rank == 1
    assert TokenLogprob(5, -0.5, 2).top == ()


# ---- the engine over a recording fake data plane -------------------------------------------------------------------------
def _score(tok, length, n):
    """What the fake reports for a token picked behind `length` tokens by a row that asks for n alternatives."""
    return TokenLogprob(tok, -length / 8.0, 1 + length % 5, tuple(((tok + j) % 97, -float(j)) for j in range(n)))


class ScoringModel:
    """Chunk-invariant tokens — (sum of a sequence's tokens + its length) % 97 — and, for the rows whose params ask, a
    TokenLogprob that is a function of the sequence's length (chunks included: the engine must drop those of non-final
    chunks). `last_logprobs` is None after a step in which no row asked, and every read of it is counted."""

    def __init__(self, num_blocks=400):
        self.model_config = types.SimpleNamespace(vocab_size=1000)
        self.num_blocks = num_blocks
        self.state = {}
        self.calls = []         # per forward: (n_prefill, [ctx...], n_decode, some row asked)
        self.events = []
        self.reads = 0
        self._last = None
        self.max_draft_tokens = 3
        self.verify_calls = 0

    @property
    def last_logprobs(self):
        self.reads += 1
        return self._last

    def forward(self, input_ids, seq_ids, decoding_lens, sampling_params=None, prefill_ctx_lens=None):
        n_prefill = len(input_ids) - len(decoding_lens)
        ctx = list(prefill_ctx_lens) if prefill_ctx_lens is not None else [0] * n_prefill
        sps = sampling_params or [None] * len(input_ids)
        out, scores = [], []
        for i, (ids, sid, sp) in enumerate(zip(input_ids, seq_ids, sps)):
            st = self.state.setdefault(sid, [0, 0]) if i < n_prefill else self.state[sid]
            if i < n_prefill:
                assert ctx[i] == st[1]
            st[0] += sum(ids)
            st[1] += len(ids)
            tok = (st[0] + st[1]) % 97
            out.append(tok)
            scores.append(None if sp is None or sp.logprobs is None else _score(tok, st[1], sp.logprobs))
        asked = any(s is not None for s in scores)
        self._last = scores if asked else None
        self.calls.append((n_prefill, ctx, len(decoding_lens), asked))
        self.events.append("fwd")
        return out

    def forward_verify(self, input_ids, seq_ids, ctx_lens):
        self.verify_calls += 1
        self._last = None
        raise AssertionError("a batch with a request that asks for logprobs is never verified")

    def swap_in_seqs(self, ids):
        self.events.append("in")

    def swap_out_seqs(self, ids):
        self.events.append("out")

    def free_seqs_resources(self, ids):
        for i in ids:
            self.state.pop(i, None)


def _expected(prompt, n, top_n):
    s, length, toks, scores = sum(prompt), len(prompt), [], []
    for _ in range(n):
        tok = (s + length) % 97
        toks.append(tok)
        scores.append(_score(tok, length, top_n) if top_n is not None else None)
        s += tok
        length += 1
    return toks, scores


def _serve(cfg, model, jobs, piggyback=True):
    """jobs: [(prompt, output_len, params)]; returns (engine, [(request, tokens)])."""
    async def run():
        eng = Engine(cfg, model=model, piggyback=piggyback)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        waits = [asyncio.ensure_future(eng.add_request_and_wait(RawRequest("", n, p, sampling_params=sp)))
                 for p, n, sp in jobs]
        done = await asyncio.wait_for(asyncio.gather(*waits), timeout=60)
        loops.cancel()
        return eng, done
    return asyncio.run(run())


def _check(done, jobs):
    for (req, toks), (prompt, n, sp) in zip(done, jobs):
        top_n = None if sp is None else sp.logprobs
        want_toks, want_scores = _expected(prompt, n, top_n)
        assert req.error is None and toks == want_toks
        if top_n is None:
            assert req.output_logprobs == []
        else:
            assert req.output_logprobs == want_scores
            assert [lp.token_id for lp in req.output_logprobs] == req.output_token_ids


@pytest.mark.parametrize("piggyback", [True, False])
def test_logprobs_stay_aligned_with_tokens_in_mixed_chunked_and_piggybacked_batches(piggyback):
    rng = np.random.RandomState(3)
    ask5, ask0 = SamplingParams(logprobs=5), SamplingParams(logprobs=0)
    shapes = [(20, 30, ask5), (37, 25, None), (900, 6, ask0), (300, 5, SamplingParams(0.7, seed=1, logprobs=20)),
              (5, 12, SamplingParams(stop_token_ids=(96,))), (700, 3, ask5)]
    jobs = [(rng.randint(0, 1000, size=n).tolist(), m, sp) for n, m, sp in shapes]
    model = ScoringModel()
    _, done = _serve(_cfg(max_prefill_chunk=256), model, jobs, piggyback)
    _check(done, jobs)
    # prompts were fed in chunks (their non-final chunks' values were reported by the fake, and dropped) ...
    assert any(c > 0 for _, ctx, _, _ in model.calls for c in ctx)
    # ... decodes rode along with chunks when piggybacking, and the engine read last_logprobs in the asking steps only
    assert any(n_pre and n_dec for n_pre, _, n_dec, _ in model.calls) == piggyback
    assert model.reads == sum(1 for *_, asked in model.calls if asked)
    quiet = ScoringModel()
    plain_jobs = [(p, n, None if sp is None or sp.logprobs is not None else sp) for p, n, sp in jobs]
    _, done = _serve(_cfg(max_prefill_chunk=256), quiet, plain_jobs, piggyback)
    _check(done, plain_jobs)
    assert quiet.reads == 0 and len(quiet.calls) > 0


def test_stop_token_end_delivers_that_tokens_logprobs():
    prompt = [1, 2, 3]
    toks, scores = _expected(prompt, 20, 2)
    stop_at = 4
    sp = SamplingParams(stop_token_ids=(toks[stop_at],), logprobs=2)
    assert toks[stop_at] not in toks[:stop_at]
    model = ScoringModel()

    async def run():
        eng = Engine(_cfg(), model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        steps = [s async for s in eng.add_request_and_stream(RawRequest("", 20, prompt, sampling_params=sp))]
        loops.cancel()
        return steps
    steps = asyncio.run(asyncio.wait_for(run(), timeout=30))
    assert [s.token_id for s in steps] == toks[:stop_at + 1]
    assert [s.logprobs for s in steps] == scores[:stop_at + 1]
    assert steps[-1].request.output_logprobs == scores[:stop_at + 1]


def test_logprobs_survive_a_swap_out_and_swap_in():
    """The scenario of tests/test_chunked_prefill_host.py: a decoding request outgrows a pool that also holds a prompt fed
    in chunks; the prompt is swapped out after its second chunk and continues after the swap-in. Both ask."""
    rng = np.random.RandomState(5)
    a, b = rng.randint(0, 1000, size=31).tolist(), rng.randint(0, 1000, size=600).tolist()
    jobs = [(a, 40, SamplingParams(logprobs=3)), (b, 4, SamplingParams(logprobs=1))]
    model = ScoringModel(num_blocks=40)
    eng, done = _serve(_cfg(max_prefill_chunk=256), model, jobs)
    assert "out" in model.events and "in" in model.events and eng.num_swapped_out == eng.num_swapped_in >= 1
    _check(done, jobs)


def test_a_batch_with_an_asking_request_is_never_speculated():
    prompt = [1, 2, 3] * 4
    model = ScoringModel()
    jobs = [(prompt, 8, SamplingParams(logprobs=1))]
    eng, done = _serve(_cfg(speculative_ngram=3), model, jobs)
    _check(done, jobs)
    assert eng.speculative_k == 3 and model.verify_calls == 0 and eng.num_verify_steps == 0
    req = Request(RawRequest("", 8, prompt, sampling_params=SamplingParams(logprobs=0)))
    req.num_prefilled, req.request_id = len(prompt), 0
    req.output_token_ids.append(1)
    plain = Request(RawRequest("", 8, prompt))
    plain.num_prefilled, plain.request_id = len(prompt), 1
    plain.output_token_ids.append(1)
    assert eng._propose_drafts([plain]) is not None        # (the engine does draft for this prompt)
    assert eng._propose_drafts([plain, req]) is None and eng._propose_drafts([req]) is None


class PlainModel:
    """A data plane without `last_logprobs` whose forward takes the reference's three arguments."""
    num_blocks = 8

    def __init__(self):
        self.model_config = types.SimpleNamespace(vocab_size=97)

    def forward(self, input_ids, seq_ids, decoding_lens):
        return [len(x) % 97 for x in input_ids]

    def swap_in_seqs(self, ids):
        pass

    swap_out_seqs = free_seqs_resources = swap_in_seqs


def test_a_data_plane_without_last_logprobs_serves_requests_that_do_not_ask():
    jobs = [([1, 2], 3, None), ([5], 2, SamplingParams())]
    _, done = _serve(_cfg(), PlainModel(), jobs)
    assert [t for _, t in done] == [[2, 1, 1], [1, 1]] and all(r.error is None and r.output_logprobs == [] for r, _ in done)


# ---- HTTP ---------------------------------------------------------------------------------------------------------------------
class NonFiniteModel(ScoringModel):
    """Every other asking row reports NaN for the token and -inf for its last alternative."""

    def forward(self, *args, **kw):
        out = super().forward(*args, **kw)
        if self._last is not None:
            self._last = [s if s is None or s.token_id % 2 else
                          s._replace(logprob=math.nan, top=s.top[:-1] + ((s.top[-1][0], -math.inf),)) for s in self._last]
        return out


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


def _as_json(lp):
    def num(v):
        return v if math.isfinite(v) else None
    return {"token_id": lp.token_id, "logprob": num(lp.logprob), "rank": lp.rank, "top": [[i, num(v)] for i, v in lp.top]}


def test_api_field_and_both_answer_forms():
    from fastapi.testclient import TestClient
    prompt = [1, 2, 3]
    base = {"prompt_token_ids": prompt, "output_len": 6}
    toks, scores = _expected(prompt, 6, 2)
    with TestClient(_client(ScoringModel())) as client:
        for bad in (-1, 21, 1.5, "2", True, [2], {"n": 2}):
            r = client.post("/generate", json={**base, "logprobs": bad})
            assert r.status_code == 400 and "logprobs" in r.json()["error"], bad
        r = client.post("/generate", json={**base, "logprobs": 2})
        assert r.status_code == 200
        assert r.json() == {"output_token_ids": toks, "logprobs": [_as_json(s) for s in scores]}
        r = client.post("/generate", json={**base, "logprobs": 0})
        assert [e["top"] for e in r.json()["logprobs"]] == [[]] * 6
        assert [e["logprob"] for e in r.json()["logprobs"]] == [s.logprob for s in scores]
        r = client.post("/generate", json={**base, "logprobs": 2, "stream": True})
        assert r.status_code == 200
        assert [json.loads(line) for line in r.text.splitlines()] == [_as_json(s) for s in scores]
        # a request without the field: today's bytes, in both forms (null is no request for logprobs either)
        for body in (base, {**base, "logprobs": None}):
            r = client.post("/generate", json=body)
            assert r.content == json.dumps({"output_token_ids": toks}, separators=(",", ":")).encode()
            r = client.post("/generate", json={**body, "stream": True})
            assert r.content == "".join(f"{t}\n" for t in toks).encode()
        # with other sampling fields the params carry both
        r = client.post("/generate", json={**base, "logprobs": 1, "temperature": 0.5, "seed": 4, "stop_token_ids": [toks[2]]})
        assert r.json()["output_token_ids"] == toks[:3] and len(r.json()["logprobs"]) == 3


def test_api_sends_null_for_values_that_are_not_finite():
    from fastapi.testclient import TestClient
    prompt = [1, 2, 3]
    base = {"prompt_token_ids": prompt, "output_len": 8, "logprobs": 2}
    toks, scores = _expected(prompt, 8, 2)
    want = [_as_json(s if s.token_id % 2 else s._replace(logprob=math.nan, top=s.top[:-1] + ((s.top[-1][0], -math.inf),)))
            for s in scores]
    assert any(e["logprob"] is None for e in want) and any(e["logprob"] is not None for e in want)
    with TestClient(_client(NonFiniteModel())) as client:
        r = client.post("/generate", json=base)
        assert r.status_code == 200 and r.json() == {"output_token_ids": toks, "logprobs": want}
        assert "NaN" not in r.text and "Infinity" not in r.text
        r = client.post("/generate", json={**base, "stream": True})
        assert "NaN" not in r.text and "Infinity" not in r.text
        assert [json.loads(line) for line in r.text.splitlines()] == want
        assert client.post("/generate", json=base).status_code == 200      # (the replica is still alive)


def test_router_forwards_the_field_and_the_answer_unchanged():
    import socket
    import threading
    import time
    import fastapi
    import uvicorn
    from fastapi.responses import JSONResponse
    from fastapi.testclient import TestClient
    from swiftllm_amd.server.router import ReplicaRouter, build_app

    got = []
    answer = {"output_token_ids": [1], "logprobs": [{"token_id": 1, "logprob": None, "rank": 3, "top": [[4, -0.25], [1, None]]}]}
    app = fastapi.FastAPI()

    @app.post("/generate")
    async def generate(req: fastapi.Request):
        got.append(await req.json())
        return JSONResponse(answer)
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
        body = {"prompt_token_ids": [1, 2], "output_len": 1, "logprobs": 2}
        with TestClient(build_app(ReplicaRouter([f"http://127.0.0.1:{port}"]))) as client:
            assert client.post("/generate", json=body).json() == answer
        assert got == [body]
    finally:
        server.should_exit = True
