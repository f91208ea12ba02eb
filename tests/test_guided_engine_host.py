"""Guided requests through the real Engine and scheduler, on the CPU, against a fake data plane (tests/_churn.py's
ClosedFormModel) that honours `guides=` through the reference masks: a guided row gets an allowed end id if there is one,
else the lowest allowed id. Requests go
in through the engine's own submission path (the tokenize loop), so a bad pattern and a full store are seen where a caller
sees them: in `request.error`."""
import asyncio
import re

import _churn
from _guided_ref import allowed_ids, ref_masks
from swiftllm_amd import Engine, EngineConfig, SamplingParams
from swiftllm_amd.guided import GuideStore, TokenVocab
from swiftllm_amd.server import RawRequest

# ids: 0..255 the single bytes, then a few longer tokens, then two specials (EOS last but one)
EXTRA = [b"ab", b"12", b"yes", b"no", b"2024", b"-0", b"-"]
TOKENS = [bytes([b]) for b in range(256)] + EXTRA + [None, None]
VOCAB = TokenVocab(TOKENS)
V = len(TOKENS)
EOS = V - 2
BLOCKS = 64


class GuidedModel(_churn.ClosedFormModel):
    """The closed-form data plane + `guides=`: an end id where the cursor's state allows one, else the lowest id it allows
    (the reference masks, computed once per guide). It records what the engine asked of it."""

    def __init__(self, ecfg, store_rows):
        super().__init__(ecfg, [(t * 7 + 3) % V for t in range(V)], BLOCKS)
        self.guide_store = GuideStore(store_rows, V, VOCAB) if store_rows else None
        self._masks = {}
        self.guided_calls = []          # per forward with guides: [(seq id, mask row)]
        self.verify_seqs = []           # per verify step: (seq ids, ids of the live guided requests at that moment)
        self.live_guided = set

    def forward(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, sampling_params=None, prefill_ctx_lens=None,
                guides=None):
        out = super().forward(input_ids_list, seq_ids_list, decoding_seq_lens_list, sampling_params, prefill_ctx_lens)
        if guides is None:
            return out
        assert len(guides) == len(input_ids_list) and any(c is not None for c in guides)
        call = []
        for i, c in enumerate(guides):
            if c is None:
                continue
            g = c.guide
            assert g.refs > 0 and not g.evicted
            if g.dfa is None:
                allowed = list(g.allowed)
            else:
                masks = self._masks.get(id(g))
                if masks is None:
                    masks = self._masks[id(g)] = ref_masks(g.dfa, VOCAB, g.end_ids)
                g.built = True
                allowed = allowed_ids(masks[c.state], V)
            ends = [t for t in allowed if t in g.end_ids]
            # (a state that allows nothing: every logit is -inf, and the argmax of such a row is id 0)
            out[i] = ends[0] if ends else allowed[0] if allowed else 0
            call.append((seq_ids_list[i], c.mask_row))
        self.guided_calls.append(call)
        return out

    def forward_verify(self, input_ids_list, seq_ids_list, ctx_lens, guides=None):
        assert guides is None
        self.verify_seqs.append((list(seq_ids_list), self.live_guided()))
        return super().forward_verify(input_ids_list, seq_ids_list, ctx_lens)


def prompt(n, salt):
    return [(salt * 31 + i * 7) % 250 for i in range(n)]


def serve(raws, store_rows=64, max_steps=400, spy=None):
    """Submit `raws` through the tokenize loop, single-step the engine until everything is answered."""
    ecfg = EngineConfig(model_path="", use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=16,
                        max_seqs_in_block_table=16, max_blocks_per_seq=16, max_batch_size=8, max_tokens_in_batch=96,
                        max_prefill_chunk=32, speculative_ngram=3, use_hip_graph=False, guided_max_states=store_rows)
    model = GuidedModel(ecfg, store_rows)

    async def run():
        eng = Engine(ecfg, model=model, piggyback=True)
        await eng.initialize(BLOCKS)
        feeder = asyncio.create_task(eng._tokenize_raw_request_event_loop())
        try:
            reqs = [eng._enqueue(raw) for raw in raws]
            for _ in range(2000):           # until the submission path has answered or queued every request
                if not eng.untokenized_raw_requests and (eng._inbox.qsize() or all(r.error for r in reqs)):
                    break
                await asyncio.sleep(0.001)
            for step in range(max_steps):
                if all(r.error is not None or r.is_finished() for r in reqs):
                    break
                if spy is not None:
                    spy(eng, reqs, step)
                if not await eng.step():
                    await asyncio.sleep(0.001)      # (the guided requests are queued once their guides are acquired)
            else:
                raise AssertionError("not finished")
            await asyncio.sleep(0)
            return eng, reqs
        finally:
            feeder.cancel()
    eng, reqs = asyncio.run(run())
    return eng, model, reqs


def text_of(req):
    return b"".join(TOKENS[t] or b"" for t in req.output_token_ids)


REGEX = "[1-9][0-9]*"


def test_guided_streams_match_their_patterns_and_completion_frees_the_blocks():
    raws = [RawRequest("", 30, prompt(40, 1), sampling_params=SamplingParams(guided_regex="(yes|no)!")),
            RawRequest("", 30, prompt(24, 2), sampling_params=SamplingParams(guided_choice=["2024", "12ab"])),
            RawRequest("", 12, prompt(33, 3)),                                   # plain
            RawRequest("", 30, prompt(21, 4), sampling_params=SamplingParams(guided_regex=REGEX, stop_token_ids=(EOS,))),
            RawRequest("", 6, prompt(20, 5), sampling_params=SamplingParams(allowed_token_ids=[258, 65, 66])),
            RawRequest("", 9, prompt(28, 6), sampling_params=SamplingParams(temperature=0.8, seed=5))]
    eng, model, reqs = serve(raws)
    assert [r.error for r in reqs] == [None] * 6
    # completion ends a request: nothing can follow "no!" / "12ab", so they end there, far short of output_len
    assert text_of(reqs[0]) == b"no!" and re.fullmatch(b"(yes|no)!", text_of(reqs[0]))
    assert text_of(reqs[1]) == b"12ab" and reqs[1].guide_cursor.complete
    assert len(reqs[0].output_token_ids) < 30 and len(reqs[1].output_token_ids) < 30
    # a stop token in an accepting state ends it: "1" is accepting (more digits may follow: not complete), EOS is allowed
    # there and nowhere before
    out = reqs[3].output_token_ids
    assert out == [ord("1"), EOS] and not reqs[3].guide_cursor.complete
    assert re.fullmatch(REGEX.encode(), text_of(reqs[3])) and reqs[3].guide_cursor.text == text_of(reqs[3])
    # allowed ids: run to output_len (never complete), only those ids
    assert len(reqs[4].output_token_ids) == 6 and set(reqs[4].output_token_ids) <= {65, 66, 258}
    # the others ran as always
    assert len(reqs[2].output_token_ids) == 12 and len(reqs[5].output_token_ids) == 9
    # everything was freed and every guide released (resident, idle)
    assert model.is_empty()
    _churn.assert_scheduler_empty(eng)
    assert model.guide_store.resident() and all(g.refs == 0 for g in model.guide_store.resident())
    assert all(r.guide_cursor is None or r.guide_cursor.released for r in reqs)


def test_a_non_final_chunk_does_not_advance_the_cursor():
    # a 70-token prompt is fed in chunks of <= 32: the guided row is in the batch three times before its first token counts
    raws = [RawRequest("", 10, prompt(70, 7), sampling_params=SamplingParams(guided_choice=["ab12", "yes"]))]
    eng, model, reqs = serve(raws)
    assert reqs[0].error is None and text_of(reqs[0]) == b"ab12"
    base = reqs[0].guide_cursor.guide.base
    rows = [call[0][1] for call in model.guided_calls]
    assert len(rows) >= 3 + 1
    assert rows[:3] == [base, base, base]                # three chunks, the cursor still at the start state
    assert rows[3] != base                               # ... and the first decode step sees the state after "ab"
    assert eng.num_forwards == len(model.guided_calls)


def test_guided_requests_are_never_speculated():
    # a plain request whose prompt repeats itself is speculated — but not in the company of a live guided request: a verify
    # step never carries a guided sequence, and none runs while one is in the batch
    rep = [5, 6, 7, 8] * 8

    def spy(eng, reqs, step):
        eng.model.live_guided = lambda: {r.request_id for r in reqs
                                         if r.guide_cursor is not None and r.request_id >= 0 and not r.is_finished()}

    raws = [RawRequest("", 40, rep), RawRequest("", 20, prompt(24, 8), sampling_params=SamplingParams(
        guided_regex="[ab]{12}"))]
    eng, model, reqs = serve(raws, spy=spy)
    assert re.fullmatch(b"[ab]{12}", text_of(reqs[1])) and len(reqs[0].output_token_ids) == 40
    assert model.verify_seqs                             # speculation did run (once the guided request was gone)
    assert all(live == set() for _, live in model.verify_seqs)
    assert reqs[1].sampling_params is not None           # what keeps it out of Engine._propose_drafts


def test_a_bad_pattern_and_a_full_store_are_request_errors_and_the_others_finish():
    raws = [RawRequest("", 8, prompt(20, 9), sampling_params=SamplingParams(guided_regex="(yes|no)")),       # 6 rows
            RawRequest("", 8, prompt(20, 10), sampling_params=SamplingParams(guided_regex="a(?=b)")),        # bad syntax
            RawRequest("", 8, prompt(20, 11), sampling_params=SamplingParams(guided_regex="[0-9]{3}")),      # 4 rows: full
            RawRequest("", 8, prompt(20, 12)),
            RawRequest("", 8, prompt(20, 13), sampling_params=SamplingParams(guided_regex="[ab]{30}")),      # never fits
            RawRequest("", 8, prompt(20, 14), sampling_params=SamplingParams(allowed_token_ids=[V + 5]))]
    eng, model, reqs = serve(raws, store_rows=8)
    assert reqs[0].error is None and text_of(reqs[0]) == b"no"
    assert reqs[3].error is None and len(reqs[3].output_token_ids) == 8
    assert "position" in reqs[1].error and not reqs[1].error_retryable and reqs[1].finished_event.is_set()
    assert "no room" in reqs[2].error and reqs[2].error_retryable                # HTTP 503: try again later
    assert "mask rows" in reqs[4].error and not reqs[4].error_retryable
    assert "allowed_token_ids" in reqs[5].error and not reqs[5].error_retryable
    for r in (reqs[1], reqs[2], reqs[4], reqs[5]):
        assert r.output_token_ids == [] and r.guide_cursor is None
    assert model.is_empty() and all(g.refs == 0 for g in model.guide_store.resident())


def test_a_guide_that_runs_into_a_state_without_tokens_ends_with_an_error_and_the_others_finish():
    # trimming promises a BYTE path to an accepting state, not a token path. Here the only token that spells "a" is the
    # request's stop id, which is banned in the start state (it does not accept): nothing is allowed at the first step.
    # And "xy\x00z" needs a byte after "xy" that only the stop id spells: the dead end comes after two tokens.
    a, nul = ord("a"), 0
    raws = [RawRequest("", 8, prompt(20, 21), sampling_params=SamplingParams(guided_regex="a", stop_token_ids=(a,))),
            RawRequest("", 8, prompt(22, 22), sampling_params=SamplingParams(guided_regex="(yes|no)")),
            RawRequest("", 8, prompt(24, 23)),
            RawRequest("", 8, prompt(26, 24), sampling_params=SamplingParams(guided_regex="xy\\x00z", stop_token_ids=(nul,)))]
    eng, model, reqs = serve(raws)
    assert "no token is allowed after b''" in reqs[0].error and reqs[0].aborted and reqs[0].output_token_ids == []
    assert "no token is allowed after b'xy'" in reqs[3].error and text_of(reqs[3]) == b"xy"
    for r in (reqs[0], reqs[3]):
        assert r.is_finished() and r.finished_event.is_set() and not r.error_retryable and r.guide_cursor.released
    assert reqs[1].error is None and text_of(reqs[1]) == b"no"
    assert reqs[2].error is None and len(reqs[2].output_token_ids) == 8
    assert model.is_empty() and all(g.refs == 0 for g in model.guide_store.resident())
    _churn.assert_scheduler_empty(eng)


def test_a_pattern_that_explodes_is_a_request_error_and_the_submission_loop_survives():
    raws = [RawRequest("", 4, prompt(20, 25), sampling_params=SamplingParams(guided_regex="((a{1000}){1000}){1000}")),
            RawRequest("", 4, prompt(20, 26), sampling_params=SamplingParams(guided_regex="(" * 3000 + "a" + ")" * 3000)),
            RawRequest("", 4, prompt(20, 27), sampling_params=SamplingParams(guided_regex="[ab]{3}")),
            RawRequest("", 4, prompt(20, 28))]
    eng, model, reqs = serve(raws)
    assert "NFA states" in reqs[0].error and reqs[1].error.startswith("guided decoding: ")
    assert reqs[2].error is None and re.fullmatch(b"[ab]{3}", text_of(reqs[2]))
    assert reqs[3].error is None and len(reqs[3].output_token_ids) == 4


def test_guided_requests_are_refused_when_the_option_is_off():
    raws = [RawRequest("", 5, prompt(20, 15), sampling_params=SamplingParams(guided_regex="a")),
            RawRequest("", 5, prompt(20, 16))]
    eng, model, reqs = serve(raws, store_rows=0)
    assert "guided_max_states" in reqs[0].error and reqs[1].error is None and len(reqs[1].output_token_ids) == 5
    assert model.guided_calls == []


def test_guides_are_released_when_the_engine_fails_its_live_requests():
    ecfg = EngineConfig(model_path="", use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=16,
                        max_seqs_in_block_table=16, max_blocks_per_seq=16, max_batch_size=8, max_tokens_in_batch=96, use_hip_graph=False,
                        guided_max_states=16)
    model = GuidedModel(ecfg, 16)

    async def run():
        eng = Engine(ecfg, model=model, piggyback=True)
        await eng.initialize(BLOCKS)
        feeder = asyncio.create_task(eng._tokenize_raw_request_event_loop())
        try:
            req = eng._enqueue(RawRequest("", 20, prompt(20, 17), sampling_params=SamplingParams(guided_regex="[ab]{9}")))
            for _ in range(2000):
                if eng._inbox.qsize():
                    break
                await asyncio.sleep(0.001)
            await eng.step()
            await eng.step()
            assert req.guide_cursor.guide.refs == 1 and len(req.output_token_ids) >= 1 and not req.is_finished()
            eng._fail_live("engine stopped: test")      # what an abort of everything in flight does
            assert req.guide_cursor.guide.refs == 0 and req.guide_cursor.released and req.error
            eng._fail_live("again")                     # once only
            assert req.guide_cursor.guide.refs == 0
        finally:
            feeder.cancel()
    asyncio.run(run())
