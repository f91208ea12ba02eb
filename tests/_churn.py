"""One churned serving scenario with every option on, and what it must produce (host only: no device, no kernels).

The decisive checkpoint (oracle/synth.py: make_decisive_state_dict) has a greedy stream that is a closed form of the
prompt — the token after position p is perm[token(p - OFFSET)] — so every greedy request of the scenario has an expected
stream that does not depend on the schedule that served it: chunked, piggybacked, speculated, swapped, replayed from a
graph or launched eagerly. `build_scenario` returns the engine options, the requests with their arrival steps and those
streams; `ClosedFormModel` is a data plane that answers the closed form on the CPU, so the real Engine and scheduler can
replay the scenario without a GPU; `TraceRecorder` wraps either data plane and records what the engine asked of it;
`coverage` turns a trace into the counters the tests hold to the conditions C2 of tests/test_serving_churn_host.py.
"""
import asyncio
import dataclasses
import functools
import random
from typing import List, Optional

from oracle import synth

DECISIVE = dict(num_hidden_layers=3, hidden_size=1024, num_attention_heads=16, num_key_value_heads=4,
                intermediate_size=2048, vocab_size=2048, max_position_embeddings=2048, rope_theta=500000.0)
OFFSET = 19
MAX_CONTEXT = 300
BLOCK = 16
MIN_TOKENS = 5          # of the stop-token request
STOP_INDEX = 11         # ... whose stream ends with the closed-form token at this output index
GPU_BLOCKS = 33         # of the GPU pool: the plain stretch overflows it twice (C2 was tuned on this and on S2, S3)
S2, S3 = 66, 96         # steps at which the second and third stretch begin to arrive
DECOY_INDEX = 2         # ... and whose second stop token is the closed-form token at this one (banned there: see Spec)

PLAIN, RUN, PAIRS, SAMPLED, PROCESSED, STOP, PASSENGER = "plain", "run", "pairs", "sampled", "processed", "stop", "passenger"


@functools.lru_cache(maxsize=None)
def decisive(dtype_name: str):
    """(config dict, state dict, perm) of the decisive checkpoint at the scenario's geometry, once per dtype."""
    import torch
    cfg = synth.make_config(**DECISIVE)
    sd, perm, _ = synth.make_decisive_state_dict(cfg, seed=5, dtype=getattr(torch, dtype_name), offset=OFFSET,
                                                 max_context=MAX_CONTEXT)
    return cfg, sd, [int(t) for t in perm]


def closed_form(prompt, perm, steps):
    """The first `steps` greedy outputs after `prompt` (one sequence of synth.decisive_expected_tokens)."""
    return [t[0] for t in synth.decisive_expected_tokens([prompt], perm, OFFSET, steps - 1)]


@dataclasses.dataclass
class Spec:
    """One request. `expected`: its whole output stream, or None (a free sampled passenger). `banned_at`: an output index
    at which the closed-form token is one of the request's stop tokens while fewer than min_tokens tokens exist — the data
    plane bans it there (SamplingParams: "the stop tokens cannot be picked"), so that one position holds whatever the
    runner-up is: it must differ from the banned token and is not held to a value. Every other position is exact."""
    kind: str
    prompt: List[int]
    output_len: int
    arrival: int
    sampling_params: object = None
    expected: Optional[List[int]] = None
    banned_at: Optional[int] = None

    @property
    def exact(self) -> bool:
        return self.expected is not None

    def mismatch(self, got: List[int]) -> Optional[str]:
        """None when `got` is this request's expected stream, else what is wrong with it."""
        want = self.expected
        if len(got) != len(want):
            return f"{len(got)} tokens, expected {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            if i == self.banned_at:
                if g == w:
                    return f"output {i} is the stop token {w}, banned below min_tokens"
            elif g != w:
                return f"output {i} is {g}, expected {w}"
        return None


@dataclasses.dataclass
class Scenario:
    engine: dict            # EngineConfig keywords (all but model_path and dtype)
    num_gpu_blocks: int
    requests: List[Spec]
    vocab: int


def _random_prompt(rng, n, vocab):
    return [rng.randrange(vocab) for _ in range(n)]


def _plant_run(prompt, perm, out_from, out_to, at):
    """Write outputs [out_from, out_to) of the prompt's own closed-form stream consecutively into prompt[at:]. The stream
    reads the prompt's last OFFSET + 1 tokens only (and itself), so planting before them does not move it: a 1-gram match
    on output out_from then proposes the next outputs correctly, draft after draft."""
    n = len(prompt)
    stream = closed_form(prompt, perm, out_to)
    assert at + (out_to - out_from) <= n - OFFSET - 1
    prompt[at:at + out_to - out_from] = stream[out_from:out_to]
    assert closed_form(prompt, perm, out_to) == stream
    return prompt


def _plant_pairs(prompt, perm):
    """tests/test_gpu_spec_decode.py: _planted_prompts — the pairs (t_s, t_s+1), s = 0, 2, .., 10 at positions 3j, 3j + 1: a
    1-gram match proposes the right next token, then junk."""
    n = len(prompt)
    for j, s in enumerate(range(0, 12, 2)):
        prompt[3 * j] = perm[prompt[n - OFFSET - 1 + s]]
        prompt[3 * j + 1] = perm[prompt[n - OFFSET - 1 + s + 1]]
    return prompt


def build_scenario(perm, use_hip_graph: bool = True, seed: int = 7, kv_cache_dtype: str = "auto") -> Scenario:
    """The churned scenario. Three stretches: plain requests only (speculation runs: whole drafts accepted on the planted
    runs, rejections on the planted pairs and on chance 1-gram matches; a long prompt is fed in chunks behind the
    decodes and the pool overflows: swaps); then sampled, processed and stop-token requests and the free passengers
    arrive (no verify steps while one of them lives; sampled / processed graphs); then plain requests only again, short
    late arrivals taking the ids of finished requests, speculation resuming on sequences that went to the host and back."""
    from swiftllm_amd.sampling_params import SamplingParams
    vocab = len(perm)
    rng = random.Random(seed)
    spec_on = kv_cache_dtype == "auto"      # (the config refuses FP8 pools with speculation)
    engine = dict(use_dummy=False, block_size=BLOCK, gpu_mem_utilization=0.9, num_cpu_blocks=48,
                  max_seqs_in_block_table=16, max_blocks_per_seq=16, max_batch_size=8, max_tokens_in_batch=96,
                  max_prefill_chunk=32, speculative_ngram=3 if spec_on else 0, use_hip_graph=use_hip_graph,
                  kv_cache_dtype=kv_cache_dtype)
    reqs: List[Spec] = []

    def add(kind, prompt, output_len, arrival, sp=None, expected=True, banned_at=None):
        assert OFFSET < len(prompt) <= 190 and len(prompt) + output_len <= 256
        exp = closed_form(prompt, perm, output_len) if expected else None
        reqs.append(Spec(kind, prompt, output_len, arrival, sp, exp, banned_at))
        return reqs[-1]

    # ---- stretch 1: plain only
    add(PLAIN, _random_prompt(rng, 70, vocab), 40, 0)
    add(RUN, _plant_run(_random_prompt(rng, 90, vocab), perm, 0, 12, 5), 35, 0)
    add(PAIRS, _plant_pairs(_random_prompt(rng, 75, vocab), perm), 30, 0)
    add(RUN, _plant_run(_random_prompt(rng, 100, vocab), perm, 4, 40, 3), 45, 0)      # drafts all its life: before and after swaps
    add(PLAIN, _random_prompt(rng, 170, vocab), 30, 2)                                # six chunks behind the decodes
    add(RUN, _plant_run(_random_prompt(rng, 120, vocab), perm, 2, 40, 7), 45, 4)
    add(RUN, _plant_run(_random_prompt(rng, 110, vocab), perm, 2, 40, 4), 45, 5)
    # ---- stretch 2: sampled / processed / stop-token requests and the passengers suppress speculation
    p = _random_prompt(rng, 64, vocab)
    add(PROCESSED, p, 28, S2, SamplingParams(repetition_penalty=1.01, presence_penalty=0.004, frequency_penalty=0.002,
                                             logit_bias={p[3]: 0.008}, min_p=0.05))
    p = _random_prompt(rng, 50, vocab)
    stream = closed_form(p, perm, STOP_INDEX + 1)
    assert stream[STOP_INDEX] not in stream[:STOP_INDEX] and stream.count(stream[DECOY_INDEX]) == 1
    s = add(STOP, p, 30, S2 + 1, SamplingParams(stop_token_ids=(stream[STOP_INDEX], stream[DECOY_INDEX]), min_tokens=MIN_TOKENS),
            banned_at=DECOY_INDEX)
    s.expected = stream
    add(SAMPLED, _random_prompt(rng, 60, vocab), 30, S2 + 10, SamplingParams(temperature=0.8, top_k=1, seed=11))
    add(PASSENGER, _random_prompt(rng, 45, vocab), 25, S2 + 11,
        # (its 1100 bias entries outgrow the model's entry buffer: the captured graphs are dropped mid-scenario)
        SamplingParams(temperature=0.9, top_p=0.9, seed=22, repetition_penalty=1.1, min_p=0.02,
                       logit_bias={t: -0.02 for t in range(1100)}), expected=False)
    add(PASSENGER, _random_prompt(rng, 40, vocab), 30, S2 + 16, SamplingParams(temperature=0.9, top_p=0.9, seed=21), expected=False)
    # ---- stretch 3: plain only again; short late arrivals recycle ids
    add(PLAIN, _random_prompt(rng, 30, vocab), 25, S3)
    add(RUN, _plant_run(_random_prompt(rng, 48, vocab), perm, 0, 20, 2), 25, S3 + 2)
    add(PLAIN, _random_prompt(rng, 33, vocab), 26, S3 + 8)
    return Scenario(engine, GPU_BLOCKS, reqs, vocab)


# ---- a data plane that answers the closed form ------------------------------------------------------------------------
class ClosedFormModel:
    """LlamaModel's serving surface on the CPU. It remembers every sequence's tokens and answers perm[seq[len - 1 -
    OFFSET]]; a sampled row (no closed form) draws a fixed function of (seed, position); a stop token is not picked while
    the sequence has fewer than min_tokens outputs. It holds the calls to what the real data plane requires: sequences in
    step, resident where they are used, and never more KV blocks in a pool than the pool has. It exposes no
    gpu_block_manager: the engine clips drafts by its own bookkeeping."""
    max_draft_tokens = 3

    def __init__(self, engine_config, perm, num_blocks):
        import types
        self.engine_config = engine_config
        self.model_config = types.SimpleNamespace(vocab_size=len(perm))
        self.perm = perm
        self.num_blocks = num_blocks
        self.seqs = {}          # seq id -> tokens whose K/V are stored (rejected drafts included until overwritten)
        self.prompt_lens = {}
        self.blocks = {}        # seq id -> blocks it holds (high-water mark of its stored tokens)
        self.on_host = set()

    def _answer(self, sid, sp):
        seq = self.seqs[sid]
        n = len(seq)
        if sp is not None and not sp.greedy and sp.top_k != 1:
            return (sp.seed * 1000003 + n * 7919) % len(self.perm)
        tok = self.perm[seq[n - 1 - OFFSET]] if n > OFFSET else 0
        if sp is not None and sp.stop_token_ids and n - self.prompt_lens[sid] < sp.min_tokens:
            while tok in sp.stop_token_ids:
                tok = (tok + 1) % len(self.perm)
        return tok

    def _stored(self, sid, upto, new):
        seq = self.seqs[sid]
        assert sid not in self.on_host, f"sequence {sid} is used while swapped out"
        assert len(seq) >= upto, f"sequence {sid}: {len(seq)} tokens stored, the call places it at {upto}"
        del seq[upto:]          # (what rejected drafts stored lies past the length: overwritten now)
        seq.extend(new)
        self.blocks[sid] = max(self.blocks.get(sid, 0), -(-len(seq) // BLOCK))
        assert self.blocks[sid] <= self.engine_config.max_blocks_per_seq

    def _check_pools(self):
        gpu = sum(b for s, b in self.blocks.items() if s not in self.on_host)
        cpu = sum(b for s, b in self.blocks.items() if s in self.on_host)
        assert gpu <= self.num_blocks, f"{gpu} GPU blocks in use, the pool has {self.num_blocks}"
        assert cpu <= self.engine_config.num_cpu_blocks, f"{cpu} CPU blocks in use"

    def forward(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, sampling_params=None, prefill_ctx_lens=None):
        n_pre = len(input_ids_list) - len(decoding_seq_lens_list)
        ctx = list(prefill_ctx_lens or [0] * n_pre)
        params = sampling_params or [None] * len(input_ids_list)
        assert len(set(seq_ids_list)) == len(seq_ids_list)
        ecfg = self.engine_config
        assert sum(len(x) for x in input_ids_list) <= ecfg.max_tokens_in_batch and len(input_ids_list) <= ecfg.max_batch_size
        out = []
        for i, (ids, sid, sp) in enumerate(zip(input_ids_list, seq_ids_list, params)):
            if i < n_pre:
                if ctx[i] == 0:
                    assert sid not in self.seqs, f"sequence id {sid} starts over without having been freed"
                    self.seqs[sid] = []
                    self.prompt_lens[sid] = 0
                self._stored(sid, ctx[i], ids)
                self.prompt_lens[sid] = len(self.seqs[sid])
            else:
                assert len(ids) == 1
                self._stored(sid, decoding_seq_lens_list[i - n_pre] - 1, ids)
            out.append(self._answer(sid, sp))
        self._check_pools()
        return out

    def forward_verify(self, input_ids_list, seq_ids_list, ctx_lens):
        out = []
        assert sum(len(x) for x in input_ids_list) <= self.engine_config.max_tokens_in_batch
        for ids, sid, c in zip(input_ids_list, seq_ids_list, ctx_lens):
            assert 1 <= len(ids) <= self.max_draft_tokens + 1
            self._stored(sid, c, [])
            row = []
            for t in ids:
                self.seqs[sid].append(t)
                row.append(self._answer(sid, None))
            self._stored(sid, c + len(ids), [])
            out.append(row)
        self._check_pools()
        return out

    def swap_out_seqs(self, seq_ids_list):
        for sid in seq_ids_list:
            assert sid in self.seqs and sid not in self.on_host
            self.on_host.add(sid)
        self._check_pools()

    def swap_in_seqs(self, seq_ids_list):
        for sid in seq_ids_list:
            assert sid in self.on_host
            self.on_host.discard(sid)
        self._check_pools()

    def free_seqs_resources(self, seq_ids_list):
        for sid in seq_ids_list:
            assert sid not in self.on_host
            del self.seqs[sid], self.prompt_lens[sid], self.blocks[sid]

    def is_empty(self) -> bool:
        return not (self.seqs or self.prompt_lens or self.blocks or self.on_host)


# ---- what the engine asked of the data plane --------------------------------------------------------------------------
class TraceRecorder:
    """Wraps a data plane's forward, forward_verify, swap_in_seqs, swap_out_seqs and free_seqs_resources (instance
    attributes over the methods; `detach` takes them off) and appends one dict per call to `events`:
      kind          "forward" | "verify" | "swap_out" | "swap_in" | "free"
      seq_ids, reqs the block-table rows, and the scenario indices of the requests that hold them (`resolve`)
      n_in, ctx     tokens brought and tokens resident before the call, per sequence (forward, verify)
      n_prefill     leading sequences that bring prompt tokens (forward)
      sampled, processed, any_params   some row draws / has its logits processed / has sampling params at all (forward)
      accepted, drafts  per sequence (verify)
      state         (num_prefilled, prompt_len, outputs) of each request at the call (swap_out, swap_in, free)
    On a LlamaModel (it has a `replay`, worker/decode_replay.py) also: `lookahead` (the prepared step was taken), `la_dropped` (a prepared step
    existed and this call dropped it), `graph_key` (the replayed graph), `captured` (it was captured by this call), and
    `drops` (captured graphs forgotten by replay.drop_graphs during this call). `before_free` callbacks run with the
    sequence ids before the blocks go."""
    NAMES = ("forward", "forward_verify", "swap_in_seqs", "swap_out_seqs", "free_seqs_resources")
    SPIES = ("take", "run", "drop_graphs")

    def __init__(self, model, resolve):
        self.model, self.resolve = model, resolve
        self.events = []
        self.before_free = []
        self._cur = None
        self.replay = getattr(model, "replay", None)
        self._real = self.replay is not None
        self._inner = {name: getattr(model, name) for name in self.NAMES}
        self._inner.update({name: getattr(self.replay, name) for name in (self.SPIES if self._real else ())})
        model.forward, model.forward_verify = self._forward, self._verify
        model.swap_in_seqs = functools.partial(self._move, "swap_in")
        model.swap_out_seqs = functools.partial(self._move, "swap_out")
        model.free_seqs_resources = functools.partial(self._move, "free")
        if self._real:
            self.replay.take, self.replay.run = self._spy_lookahead, self._spy_graph
            self.replay.drop_graphs = self._spy_drop

    def detach(self):
        for name in self._inner:
            delattr(self.replay if name in self.SPIES else self.model, name)

    def _open(self, kind, seq_ids, **fields):
        ev = dict(kind=kind, seq_ids=list(seq_ids), reqs=[self.resolve(s) for s in seq_ids], drops=0, **fields)
        if self._real:
            ev["la_pending"] = self.replay.prepared is not None
        self.events.append(ev)
        self._cur = ev
        return ev

    def _close(self, ev):
        if self._real and ev["kind"] != "forward":
            ev["la_dropped"] = ev.pop("la_pending")     # (swap, free and verify forget a prepared step)
        self._cur = None

    def _forward(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, **kw):
        n_pre = len(input_ids_list) - len(decoding_seq_lens_list)
        params = kw.get("sampling_params") or [None] * len(input_ids_list)
        ctx = list(kw.get("prefill_ctx_lens") or [0] * n_pre) + [n - 1 for n in decoding_seq_lens_list]
        ev = self._open("forward", seq_ids_list, n_in=[len(x) for x in input_ids_list], ctx=ctx, n_prefill=n_pre,
                        sampled=any(p is not None and not p.greedy for p in params),
                        processed=any(p is not None and p.processes_logits for p in params),
                        any_params=any(p is not None for p in params))
        ev["out"] = self._inner["forward"](input_ids_list, seq_ids_list, decoding_seq_lens_list, **kw)
        self._close(ev)
        return ev["out"]

    def _verify(self, input_ids_list, seq_ids_list, ctx_lens):
        from swiftllm_amd.server.speculative import accept
        ev = self._open("verify", seq_ids_list, n_in=[len(x) for x in input_ids_list], ctx=list(ctx_lens))
        out = self._inner["forward_verify"](input_ids_list, seq_ids_list, ctx_lens)
        ev["drafts"] = [len(x) - 1 for x in input_ids_list]
        ev["accepted"] = [accept(x[1:], t) for x, t in zip(input_ids_list, out)]
        self._close(ev)
        return out

    def _move(self, kind, seq_ids_list):
        ev = self._open(kind, seq_ids_list)
        ev["state"] = [self.resolve(s, state=True) for s in seq_ids_list]
        if kind == "free":
            for hook in self.before_free:
                hook(list(seq_ids_list))
        name = "free_seqs_resources" if kind == "free" else kind + "_seqs"
        self._inner[name](seq_ids_list)
        self._close(ev)

    def _spy_lookahead(self, *args, **kw):
        la = self._inner["take"](*args, **kw)
        ev = self._cur
        if ev is not None and "lookahead" not in ev:       # (the engine fallback runs a step twice: the first call counts)
            ev["lookahead"] = la is not None
            ev["la_dropped"] = ev.pop("la_pending") and la is None
        return la

    def _spy_graph(self, *args, **kw):
        before = self.replay.captures
        out = self._inner["run"](*args, **kw)
        if self._cur is not None:
            self._cur["graph_key"] = next(reversed(self.replay.graphs))     # (re)inserted last = the one replayed
            self._cur["captured"] = self.replay.captures > before
        return out

    def _spy_drop(self):
        if self._cur is not None:
            self._cur["drops"] += len(self.replay.graphs)
        return self._inner["drop_graphs"]()


def bucket(batch: int) -> int:
    """decode_replay.decode_batch_bucket for batches of at most 32 sequences."""
    return batch if batch <= 2 else -(-batch // 8) * 8


def coverage(events, specs) -> dict:
    """The counters of C2 (and, on a LlamaModel's trace, of the look-ahead and the graph cache) from a trace."""
    c = dict(swap_partial_prompt=0, swap_decoding=0, verify_before_and_after_swap=0, chunk_behind_context=0,
             chunks_with_decodes=0, verify_all_accepted=0, verify_rejected=0, verify_across_block=0, decode_buckets=set(),
             decode_sampled_only=0, decode_processed_only=0, decode_sampled_and_processed=0, verify_to_suppressed=0,
             suppressed_to_verify=0, ids_recycled=0, plain_after_processed=0, lookahead_hits=0, lookahead_dropped=0,
             captures=0, captures_after_drop=0, graph_keys=set(), verify_steps=0, forwards=0, swapped_out=0, swapped_in=0)
    out_state, verified, verified_before = {}, set(), set()     # request -> state at its swap-out; requests verified so far
    came_back = set()
    mode, dropped = None, False
    holder = {}             # seq id -> the last request that held it
    for ev in events:
        kind = ev["kind"]
        for sid, r in zip(ev["seq_ids"], ev["reqs"]):
            prev = holder.get(sid)
            if prev is not None and prev != r:
                c["ids_recycled"] += 1
                if specs[prev].kind == PROCESSED and specs[r].sampling_params is None:
                    c["plain_after_processed"] += 1
            holder[sid] = r
        c["lookahead_dropped"] += bool(ev.get("la_dropped"))
        dropped = dropped or ev["drops"] > 0
        if kind == "swap_out":
            c["swapped_out"] += len(ev["reqs"])
            for r, st in zip(ev["reqs"], ev["state"]):
                out_state[r] = st
                if r in verified:
                    verified_before.add(r)
        elif kind == "swap_in":
            c["swapped_in"] += len(ev["reqs"])
            for r in ev["reqs"]:
                prefilled, prompt_len, outputs = out_state.pop(r)
                came_back.add(r)
                if outputs:
                    c["swap_decoding"] += 1
                elif 0 < prefilled < prompt_len:
                    c["swap_partial_prompt"] += 1
        elif kind == "verify":
            c["verify_steps"] += 1
            for r in ev["reqs"]:
                if r in verified_before and r in came_back:
                    c["verify_before_and_after_swap"] += 1
                    verified_before.discard(r)
                verified.add(r)
            c["verify_all_accepted"] += any(d > 0 and a == d for d, a in zip(ev["drafts"], ev["accepted"]))
            c["verify_rejected"] += any(a < d for d, a in zip(ev["drafts"], ev["accepted"]))
            c["verify_across_block"] += any(n > 1 and x // BLOCK != (x + n - 1) // BLOCK for x, n in zip(ev["ctx"], ev["n_in"]))
            c["suppressed_to_verify"] += mode == "suppressed"
            mode = "verify"
        elif kind == "forward":
            c["forwards"] += 1
            n_pre, batch = ev["n_prefill"], len(ev["seq_ids"])
            c["chunk_behind_context"] += any(x > 0 for x in ev["ctx"][:n_pre])
            c["chunks_with_decodes"] += 0 < n_pre < batch
            if n_pre == 0:
                c["decode_buckets"].add(bucket(batch))
                c["decode_sampled_only"] += ev["sampled"] and not ev["processed"]
                c["decode_processed_only"] += ev["processed"] and not ev["sampled"]
                c["decode_sampled_and_processed"] += ev["sampled"] and ev["processed"]
                if ev["any_params"]:        # a live request with sampling params: the engine may not speculate
                    c["verify_to_suppressed"] += mode == "verify"
                    mode = "suppressed"
                c["lookahead_hits"] += bool(ev.get("lookahead"))
                if ev.get("captured"):
                    c["captures"] += 1
                    c["captures_after_drop"] += dropped
                if "graph_key" in ev:
                    c["graph_keys"].add(ev["graph_key"])
    return c


def assert_coverage(c: dict, real_graphs: bool = False, speculation: bool = True):
    """C2. `real_graphs`: the trace of a LlamaModel with graph replay on — the look-ahead and the graph cache too."""
    need = ["swap_partial_prompt", "swap_decoding", "chunk_behind_context", "chunks_with_decodes", "decode_sampled_only",
            "decode_processed_only", "decode_sampled_and_processed", "ids_recycled", "plain_after_processed"]
    if speculation:
        need += ["verify_before_and_after_swap", "verify_all_accepted", "verify_rejected", "verify_across_block",
                 "verify_to_suppressed", "suppressed_to_verify"]
    if real_graphs:
        need += ["lookahead_hits", "lookahead_dropped", "captures_after_drop"]
    missing = [name for name in need if c[name] < 1]
    assert not missing, f"the scenario did not reach: {missing}\n{c}"
    assert len(c["decode_buckets"]) >= 3 and c["decode_buckets"] & {1, 2}, c["decode_buckets"]
    assert c["swapped_out"] == c["swapped_in"]


def shape_of(events):
    """What the schedule was, without what the data plane answered: for comparing two runs of the scenario."""
    return [(e["kind"], tuple(e["reqs"]), tuple(e.get("n_in", ())), tuple(e.get("ctx", ()))) for e in events]


# ---- serving it -------------------------------------------------------------------------------------------------------
def serve(model, engine_config, scenario: Scenario, max_steps: int = 600, before_free=None):
    """The scenario through a new Engine on `model`, single-stepped; request i enters the scheduler before step
    `arrival`. `before_free(index, request, seq_id)` runs for every finished request while it still holds its blocks.
    Returns (engine, requests, recorder) — the recorder is detached from the model again."""
    from swiftllm_amd import Engine
    from swiftllm_amd.server import RawRequest, Request

    async def run():
        eng = Engine(engine_config, model=model, piggyback=True)
        await eng.initialize(scenario.num_gpu_blocks)
        reqs = []
        for i, s in enumerate(scenario.requests):
            r = Request(RawRequest("", s.output_len, list(s.prompt), sampling_params=s.sampling_params))
            r.churn_index = i
            assert eng.scheduler.why_unservable(r) is None
            reqs.append(r)

        def resolve(sid, state=False):
            sch = eng.scheduler
            held = [r for r in list(sch.running_q) + list(sch.swapped_q) if r.request_id == sid]
            assert len(held) == 1, f"block-table row {sid} is held by {len(held)} requests"
            r = held[0]
            return (r.num_prefilled, r.prompt_len, len(r.output_token_ids)) if state else r.churn_index
        rec = TraceRecorder(model, resolve)
        if before_free is not None:
            rec.before_free.append(lambda sids: [before_free(resolve(s), reqs[resolve(s)], s) for s in sids])
        try:
            for step in range(max_steps):
                arrived = [r for r, s in zip(reqs, scenario.requests) if s.arrival == step]
                if arrived:
                    eng.scheduler.on_requests_arrival(arrived)
                if all(r.is_finished() for r in reqs):
                    break
                did = await eng.step()
                assert did or any(s.arrival > step for s in scenario.requests), f"step {step}: nothing to do, requests left"
            else:
                raise AssertionError(f"not finished after {max_steps} steps")
        finally:
            rec.detach()
        return eng, reqs, rec
    return asyncio.run(run())


def assert_streams(scenario: Scenario, reqs):
    for i, (s, r) in enumerate(zip(scenario.requests, reqs)):
        assert r.error is None, (i, s.kind, r.error)
        if s.exact:
            why = s.mismatch(r.output_token_ids)
            assert why is None, f"request {i} ({s.kind}): {why}\n got  {r.output_token_ids}\n want {s.expected}"
        else:
            assert len(r.output_token_ids) == s.output_len, (i, len(r.output_token_ids))
            assert all(0 <= t < scenario.vocab for t in r.output_token_ids), i


def assert_scheduler_empty(eng):
    sch = eng.scheduler
    assert not sch.has_work()
    assert sorted(sch.request_id_manager._free) == list(range(sch.request_id_manager.max_id))
