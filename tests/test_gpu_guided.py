"""Guided decoding on the GPU: csrc/guided.hip against tests/_guided_ref.py bit for bit, the model's guided steps against
the reference applied to the same step's unguided logits, and the engine end to end. Every comparison is exact."""
import asyncio
import re

import numpy as np
import pytest
import torch

from oracle import synth

import _lora as L
from _guided_ref import allowed_ids, bits_of, ref_apply, ref_masks, synthetic_vocab
from _logits_ref import adjust_ref, min_p_gap

pytestmark = pytest.mark.gpu

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
FILL = -1       # 0xffffffff


def _K():
    from swiftllm_amd.worker.kernels import guided
    return guided


def _G():
    from swiftllm_amd import guided
    return guided


# ---- the build kernel -----------------------------------------------------------------------------------------------------
DATE = "[0-9]{4}-[0-9]{2}-[0-9]{2}T[0-9]{2}:[0-9]{2}(:[0-9]{2}(\\.[0-9]{1,6})?)?(Z|[-+][0-9]{2}:[0-9]{2})"
RUNS = "[0-9a-z \\-:.,\"{}\\[\\]TZ]{0,30}(é|€)?"


def _dfas():
    G = _G()
    # (one state that loops on every byte, made by hand: subset construction does not minimise `(.|\n)*` to it)
    one = G.Dfa(np.zeros((1, 256), dtype=np.int32), np.ones(1, dtype=np.bool_), np.zeros(1, dtype=np.bool_))
    return {"one_state": one, "date": G.compile_regex(DATE), "runs": G.compile_regex(RUNS),
            "choice": G.compile_choice(["yes", "no", "maybe", "café", "12-34", "yesterday"])}


def _build(dfa, vocab, end_ids, row_base, words, pool_rows):
    K = _K()
    dev = torch.device("cuda")
    pool = torch.full((pool_rows, words), FILL, dtype=torch.int32, device=dev)
    dv = K.upload_vocab(vocab, len(vocab), dev)
    ends = torch.tensor(list(end_ids), dtype=torch.int32, device=dev) if end_ids else None
    K.build_guide_masks(pool, row_base, torch.from_numpy(dfa.trans).to(dev),
                        torch.from_numpy(dfa.accepting.view(np.uint8)).to(dev), dv, ends)
    return pool.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("vocab_size,extra_words", [(1003, 0), (4096, 0), (1003, 3)])
def test_build_kernel_equals_the_reference_bit_for_bit(vocab_size, extra_words):
    end_ids = (vocab_size - 1, 700)
    vocab = synthetic_vocab(vocab_size, seed=vocab_size, end_ids=end_ids)
    assert vocab.tokens[259] is None and vocab.tokens[296] is None and any(t and len(t) >= 20 for t in vocab.tokens)
    assert b"a\xc3" in vocab.tokens and b"\x82\xac" in vocab.tokens     # tokens that split a UTF-8 character
    words = (vocab_size + 31) // 32 + extra_words
    dfas = _dfas()
    assert dfas["one_state"].num_states == 1 and 30 <= dfas["date"].num_states <= 60
    for name, dfa in dfas.items():
        want = ref_masks(dfa, vocab, end_ids, words)
        s = dfa.num_states
        for row_base in (0, 5):
            rows = row_base + s + 3
            got = _build(dfa, vocab, end_ids, row_base, words, rows)
            assert np.array_equal(got[row_base:row_base + s], want), (name, row_base)
            assert (got[:row_base] == 0xffffffff).all() and (got[row_base + s:] == 0xffffffff).all(), (name, row_base)
            assert np.array_equal(_build(dfa, vocab, end_ids, row_base, words, rows), got), (name, "two builds differ")
        # what the masks say: an end id is allowed exactly in the accepting states, an empty id never
        for st in range(s):
            allowed = set(allowed_ids(want[st], vocab_size))
            assert (end_ids[0] in allowed) == (end_ids[1] in allowed) == bool(dfa.accepting[st])
            assert 259 not in allowed and 296 not in allowed
    # without end ids: the same walk, and the ids that were end ids spell nothing
    dfa = dfas["choice"]
    got = _build(dfa, vocab, (), 2, words, dfa.num_states + 4)
    assert np.array_equal(got[2:2 + dfa.num_states], ref_masks(dfa, vocab, (), words))


# ---- the mask kernel ------------------------------------------------------------------------------------------------------
def _mask_case(dtype, n, stride, rows, offset):
    g = torch.Generator().manual_seed(n * 131 + rows * 7 + offset)
    words = (n + 31) // 32
    num_mask_rows = 6
    masks = torch.randint(-2 ** 31, 2 ** 31, (num_mask_rows, words), generator=g, dtype=torch.int64).to(torch.int32)
    masks[2] = 0            # nothing allowed
    masks[3] = -1           # everything allowed
    masks[4] = torch.where(torch.rand(words, generator=g) < 0.5, torch.tensor(-1), torch.tensor(0)).to(torch.int32)
    masks[5] &= masks[0]    # sparse
    flat = (torch.randn(offset + rows * stride + 8, generator=g) * 3).to(dtype)
    x = flat[offset:offset + rows * stride].view(rows, stride)
    # NaN and +-inf at allowed and at disallowed positions of every row (the random masks decide which is which)
    for r in range(rows):
        for j, v in zip(torch.randint(0, n, (9,), generator=g).tolist(), [float("nan")] * 3 + [float("inf")] * 3 +
                        [float("-inf")] * 3):
            x[r, j] = v
        x[r, n - 1] = float("nan")
        x[r, 0] = float("inf")
    index = [(-1, 2, 0, 6, 3, 1, 4, 5, 1000, -7)[(r * 3 + 1) % 10] for r in range(rows)]
    if rows >= 7:
        index[:7] = [0, -1, 2, 6, 3, 5, 4]
    else:
        index[0] = 0
    return flat, masks, index, words, num_mask_rows


@pytest.mark.parametrize("dtype", list(DTYPES.values()))
@pytest.mark.parametrize("n,stride", [(1003, 1011), (1024, 1024), (1001, 1008)])
@pytest.mark.parametrize("rows", [1, 7, 33])
@pytest.mark.parametrize("offset", [0, 1])
def test_mask_kernel_equals_the_reference_bit_for_bit(dtype, n, stride, rows, offset):
    _hold_mask_kernel_to_the_reference(dtype, n, stride, rows, offset)


def test_mask_kernel_equals_the_reference_at_a_qwen_vocabulary():
    _hold_mask_kernel_to_the_reference(torch.bfloat16, 151936, 151936, 7, 0)


def _hold_mask_kernel_to_the_reference(dtype, n, stride, rows, offset):
    K = _K()
    flat, masks, index, words, num_mask_rows = _mask_case(dtype, n, stride, rows, offset)
    want = flat.clone()
    view = want[offset:offset + rows * stride].view(rows, stride)
    view[:, :n] = ref_apply(flat[offset:offset + rows * stride].view(rows, stride)[:, :n], masks.numpy(), index)
    outs = []
    for _ in range(2):
        dev = flat.cuda()
        x = dev[offset:offset + rows * stride].view(rows, stride)[:, :n]
        assert (x.data_ptr() % 16 == 0) == (offset == 0)
        args = K.GuideArgs(masks.cuda(), torch.tensor(index, dtype=torch.int32, device="cuda"))
        assert K.mask_logits(x, args) is x
        outs.append(dev.cpu())
    got = outs[0]
    assert torch.equal(bits_of(got), bits_of(want))      # every element, the padding columns and the bands included
    assert torch.equal(bits_of(outs[1]), bits_of(got))   # two launches agree
    # what the reference itself says, on this case: unguided rows keep their input, the all-zero row is all -inf
    src = flat[offset:offset + rows * stride].view(rows, stride)[:, :n]
    res = got[offset:offset + rows * stride].view(rows, stride)[:, :n]
    neg_inf = 0xfc00 if dtype == torch.float16 else 0xff80
    for r, k in enumerate(index):
        if k < 0 or k >= num_mask_rows or k == 3:
            assert torch.equal(bits_of(res[r]), bits_of(src[r]))
        if k == 2:
            assert (bits_of(res[r]).to(torch.int32) & 0xffff == neg_inf).all()


# ---- the model ------------------------------------------------------------------------------------------------------------
END = (510, 511)


def _vocab(v=512):
    return synthetic_vocab(v, seed=3, end_ids=END)


def _model(tmp_path, dtype="float16", states=256, vocab=True, geometry=None, **kw):
    from swiftllm_amd import EngineConfig, LlamaModel
    cfg = synth.make_config(**(geometry or synth.SMALL64))
    path = tmp_path / f"ckpt_{dtype}_{cfg['hidden_size']}"
    if not path.exists():
        synth.write_model_dir(str(path), cfg, synth.make_state_dict(cfg, seed=9, dtype=DTYPES[dtype]))
    base = dict(model_path=str(path), use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=64,
                max_seqs_in_block_table=40, max_blocks_per_seq=16, max_batch_size=8, max_tokens_in_batch=1024, dtype=dtype)
    if states is not None:
        base["guided_max_states"] = states
    base.update(kw)
    model = LlamaModel(EngineConfig(**base))
    if vocab:
        model.set_guide_vocab(_vocab(cfg["vocab_size"]))
    model.load_weights()
    model.init_kvcache_and_swap(200)
    return model, cfg


def _sp(*a, **kw):
    from swiftllm_amd import SamplingParams
    return SamplingParams(*a, **kw)


def _prompts(vocab, sizes=(9, 30, 4)):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in sizes]


def _cursor(model, kind, spec, end_ids=()):
    G = _G()
    return G.GuideCursor(model.guide_store.acquire(G.guide_key(kind, spec, end_ids)))


def _pool_ref(model) -> np.ndarray:
    """The reference of the whole device pool: every resident guide's rows (rows of no guide: zeros, never indexed)."""
    store = model.guide_store
    pool = np.zeros((store.max_states, store.words), dtype=np.uint32)
    for g in store.resident():
        if g.dfa is None:
            pool[g.base] = g.host_mask_row(store.words).view(np.uint32)
        else:
            pool[g.base:g.base + g.num_states] = ref_masks(g.dfa, store.vocab, g.end_ids, store.words)
    return pool


def _drive(model, prompts, seqs, cursors, steps, sps=None, forced=None, lora=None):
    """Prefill + up to `steps` decode steps. `cursors`: one GuideCursor or None per sequence, advanced here with the returned
    tokens and dropped (None) once complete; None: no `guides` argument at all. `forced`: the tokens to feed instead of
    the run's own (teacher forcing: per step, per sequence). Returns (tokens, tapped logits, mask rows) per step."""
    model.post_layer.logits_tap = tap = []
    toks, logits, rows = [], [], []
    lens = [len(p) for p in prompts]
    live = list(cursors) if cursors is not None else None
    for k in range(steps + 1):
        kw = {}
        if sps is not None:
            kw["sampling_params"] = sps
        if lora is not None:
            kw["lora"] = lora
        if live is not None:
            kw["guides"] = list(live)
            rows.append([-1 if c is None else c.mask_row for c in live])
        if k == 0:
            out = model.forward(prompts, seqs, [], **kw)
        else:
            lens = [n + 1 for n in lens]
            feed = forced[k - 1] if forced is not None else toks[-1]
            out = model.forward([[t] for t in feed], seqs, lens, **kw)
        toks.append(out)
        logits.append(tap[-1][:len(seqs)].clone())
        if live is not None:
            for i, c in enumerate(live):
                if c is not None:
                    c.advance(out[i])
                    if c.complete:
                        live[i] = None
            if all(c is None for c in live) and forced is None:
                break
    model.free_seqs_resources(seqs)
    model.post_layer.logits_tap = None
    return toks, logits, rows


def _first_argmax(row: torch.Tensor) -> int:
    return int(np.argmax(row.float().cpu().numpy()))     # (first occurrence: ties go to the lowest id)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("mode", ["graph_lookahead", "graph_no_lookahead", "eager"])
def test_model_masks_the_logits_the_token_is_picked_from(tmp_path, dtype, mode):
    model, cfg = _model(tmp_path, dtype, use_hip_graph=mode != "eager")
    model.replay.lookahead = mode == "graph_lookahead"
    v = cfg["vocab_size"]
    prompts = _prompts(v)
    pattern = "[0-9]{4}-[0-9]{2}"
    cursors = [_cursor(model, "regex", pattern, END), None, _cursor(model, "choice", ["yes", "no", "maybe"])]
    toks, logits, rows = _drive(model, prompts, [0, 1, 2], cursors, steps=12)
    pool = _pool_ref(model)
    # the device pool holds the reference masks of every resident guide, bit for bit
    assert np.array_equal(model._guide_masks.cpu().numpy().view(np.uint32), pool)
    # the same contexts without guides (teacher-forced with the guided run's tokens): the raw logits of every step
    raw_toks, raw, _ = _drive(model, prompts, [3, 4, 5], None, steps=len(toks) - 1, forced=toks[:-1])
    assert len(raw) == len(logits)
    for k, (got, plain, idx) in enumerate(zip(logits, raw, rows)):
        want = ref_apply(plain.cpu(), pool, idx)
        assert torch.equal(bits_of(got.cpu()), bits_of(want)), (mode, k)
        for r in range(3):
            assert toks[k][r] == _first_argmax(got[r]), (mode, k, r)
        assert toks[k][1] == raw_toks[k][1]              # (the unguided row: the raw argmax of its own context)
    # the free-running loop ended by completion, and what it spelled matches
    assert cursors[0].complete and re.fullmatch(pattern.encode(), cursors[0].text)
    assert cursors[2].complete and cursors[2].text in (b"yes", b"no", b"maybe")
    if mode == "graph_lookahead":
        assert model.replay.captures >= 1
    for c in (cursors[0], cursors[2]):
        model.guide_store.release(c.guide)


def test_a_guided_row_is_the_same_alone_and_in_a_batch_and_leaves_its_neighbours_alone(tmp_path):
    model, cfg = _model(tmp_path, "float16", use_hip_graph=True)
    v = cfg["vocab_size"]
    prompts = _prompts(v, (9, 30, 4, 17, 5, 12, 21, 8))
    pattern = "-?[1-9][0-9]{2}(\\.[0-9]{2})?"
    steps = 9
    alone = _cursor(model, "regex", pattern, END)
    t_alone, _, _ = _drive(model, [prompts[2]], [0], [alone], steps)
    crowd = _cursor(model, "regex", pattern, END)
    cursors = [None, None, crowd] + [None] * 5
    t_crowd, _, _ = _drive(model, prompts, list(range(8)), cursors, steps)
    n = min(len(t_alone), len(t_crowd))
    assert [t[0] for t in t_alone[:n]] == [t[2] for t in t_crowd[:n]] and alone.text == crowd.text
    assert re.fullmatch(pattern.encode(), crowd.text) or not crowd.complete
    # the unguided rows: what a run without `guides` gives them
    t_plain, _, _ = _drive(model, prompts, list(range(8)), None, len(t_crowd) - 1)
    for k in range(len(t_crowd)):
        for r in (0, 1, 3, 4, 5, 6, 7):
            assert t_crowd[k][r] == t_plain[k][r], (k, r)


def test_sampled_scored_and_processed_guided_rows(tmp_path):
    model, cfg = _model(tmp_path, "bfloat16", use_hip_graph=True)
    v = cfg["vocab_size"]
    prompts = _prompts(v, (12, 7))
    pool_of = lambda: _pool_ref(model)       # noqa: E731
    # a seeded sampled row under an allowed-token guide (never complete: it runs all steps) and a scored regex row
    ids = [48, 49, 50, 65, 300, 301, 455]
    sps = [_sp(1.0, seed=7, allowed_token_ids=ids, logprobs=5), _sp(guided_regex="[a-f0-9]{20}", logprobs=5)]
    runs = []
    for _ in range(2):
        cursors = [_cursor(model, "tokens", ids), _cursor(model, "regex", "[a-f0-9]{20}")]
        scores = []
        model.post_layer.logits_tap = tap = []
        lens = [len(p) for p in prompts]
        toks = [model.forward(prompts, [0, 1], [], sampling_params=sps, guides=cursors)]
        scores.append(model.last_logprobs)
        rows = [[c.mask_row for c in cursors]]
        for k in range(6):
            for c, t in zip(cursors, toks[-1]):
                c.advance(t)
            lens = [n + 1 for n in lens]
            rows.append([c.mask_row for c in cursors])
            toks.append(model.forward([[t] for t in toks[-1]], [0, 1], lens, sampling_params=sps, guides=cursors))
            scores.append(model.last_logprobs)
        logits = [t[:2].clone() for t in tap]
        model.post_layer.logits_tap = None
        model.free_seqs_resources([0, 1])
        runs.append(toks)
        pool = pool_of()
        for k, (step, lg, idx) in enumerate(zip(scores, logits, rows)):
            assert toks[k][0] in ids                     # only ever an allowed id
            for r in range(2):
                allowed = allowed_ids(pool[idx[r]], v)
                allowed_set = set(allowed)
                s = step[r]
                assert s.token_id == toks[k][r] and s.token_id in allowed
                assert len(s.top) == 5 and all(i in allowed for i, _ in s.top), (k, r, s.top)
                # the rank counts allowed tokens only: its place among them by (value descending, id ascending)
                f = lg[r].float().cpu().numpy().astype(np.float64)
                order = [int(i) for i in np.lexsort((np.arange(v), -f)) if int(i) in allowed_set]
                assert s.rank == 1 + order.index(s.token_id) and [i for i, _ in s.top] == order[:5]
                assert np.isfinite(s.logprob)
        for c in cursors:
            model.guide_store.release(c.guide)
    assert runs[0] == runs[1] and len({t[0] for t in runs[0]}) > 1      # the same draws on replay, not a constant stream

    # min-p and a logit bias on a guided row: mask first, then the adjustment of always
    bias = {49: 3.0, 50: -2.5, 100: 4.0, 455: float("-inf")}
    sp = _sp(0.9, seed=11, min_p=0.2, logit_bias=bias, allowed_token_ids=ids)
    cur = _cursor(model, "tokens", ids)
    toks, logits, rows = _drive(model, prompts[:1], [0], [cur], 3, sps=[sp])
    _, raw, _ = _drive(model, prompts[:1], [1], None, 3, forced=toks)
    pool = pool_of()
    keys = sorted(bias)
    for got, plain, idx in zip(logits, raw, rows):
        masked = ref_apply(plain.cpu(), pool, idx)
        want = adjust_ref(masked, torch.tensor([0, len(keys)], dtype=torch.int32), torch.tensor(keys, dtype=torch.int32),
                          torch.zeros(len(keys), dtype=torch.int32), torch.tensor([bias[t] for t in keys]),
                          torch.tensor([[1.0, 0.0, 0.0, min_p_gap(0.9, 0.2)]]))
        assert torch.equal(bits_of(got.cpu()), bits_of(want))
        kept = set(np.flatnonzero(np.isfinite(got[0].float().cpu().numpy())).tolist())
        assert kept and kept <= set(ids) - {455}         # min-p took its maximum over allowed tokens only
    assert all(t[0] in ids for t in toks)
    model.guide_store.release(cur.guide)


def test_chunked_mixed_fp8_and_lora_steps(tmp_path):
    ids = list(range(40, 60))

    def compare(model, calls, seqs_a, seqs_b):
        """`calls(seqs, guides)` runs the same forwards with and without guides; every tapped step must match."""
        pool = _pool_ref(model)
        model.post_layer.logits_tap = tap = []
        rows = calls(seqs_a, True)
        got = [t.clone() for t in tap]
        del tap[:]
        calls(seqs_b, False)
        raw = [t.clone() for t in tap]
        model.post_layer.logits_tap = None
        assert len(got) == len(raw) == len(rows)
        for k, (a, b, idx) in enumerate(zip(got, raw, rows)):
            assert any(i >= 0 for i in idx)
            assert torch.equal(bits_of(a.cpu()[:len(idx)]), bits_of(ref_apply(b.cpu()[:len(idx)], pool, idx))), k
        model.free_seqs_resources(seqs_a + seqs_b)

    # FP8 KV pools; a chunked prompt (the mask applies to the token after each chunk) and a mixed step
    model, cfg = _model(tmp_path, kv_cache_dtype="fp8_e4m3", use_hip_graph=True)
    prompts = _prompts(cfg["vocab_size"], (40, 11))
    cur = _cursor(model, "tokens", ids)
    cur2 = _cursor(model, "regex", "[0-9]+", END)

    fed = {}        # the guided run's tokens: the run without guides feeds the same ones (the same contexts)

    def fp8_calls(seqs, guided):
        rows = []
        g = (lambda *c: {"guides": list(c)}) if guided else (lambda *c: {})
        # chunk 1 of sequence A alone; then chunk 2 of A with the whole prompt of B; then a mixed step: the prefill of a
        # third prompt with the first decode tokens of A and B; then a pure decode step under the graph
        model.forward([prompts[0][:16]], [seqs[0]], [], **g(cur))
        rows.append([cur.mask_row])
        t1 = model.forward([prompts[0][16:], prompts[1]], seqs[:2], [], prefill_ctx_lens=[16, 0], **g(cur, cur2))
        t1 = fed.setdefault("t1", t1)
        rows.append([cur.mask_row, cur2.mask_row])
        t2 = model.forward([prompts[1][:7], [t1[0]], [t1[1]]], [seqs[2], seqs[0], seqs[1]], [41, 12], **g(None, cur, cur2))
        t2 = fed.setdefault("t2", t2)
        rows.append([-1, cur.mask_row, cur2.mask_row])
        model.forward([[t2[1]], [t2[2]]], seqs[:2], [42, 13], **g(cur, None))
        rows.append([cur.mask_row, -1])
        return rows
    compare(model, fp8_calls, [0, 1, 2], [3, 4, 5])
    del model

    # a LoRA row
    model, cfg = _model(tmp_path, max_loras=1, use_hip_graph=True)
    model.load_lora("a", state_dict=L.random_adapter(cfg, 16, 1, std=0.2), config=L.adapter_config(16))
    cur = _cursor(model, "tokens", ids)
    cur2 = _cursor(model, "choice", ["yes", "no"])

    def lora_calls(seqs, guided):
        g = (lambda *c: {"guides": list(c)}) if guided else (lambda *c: {})
        t = fed.setdefault("lora", model.forward(prompts, seqs, [], lora=["a", None], **g(cur, cur2)))
        model.forward([[x] for x in t], seqs, [41, 12], lora=["a", None], **g(cur, cur2))
        return [[cur.mask_row, cur2.mask_row]] * 2
    compare(model, lora_calls, [0, 1], [2, 3])


# (the geometry tests/test_gpu_engine.py runs the persistent one-sequence decode step at)
ENGINE_GEOMETRY = dict(num_hidden_layers=3, hidden_size=2048, num_attention_heads=16, num_key_value_heads=8,
                       intermediate_size=2048, vocab_size=1024, max_position_embeddings=2048, rope_theta=500000.0)


@pytest.mark.parametrize("graph", [True, False])
def test_the_one_sequence_decode_engine_step_is_masked_too(tmp_path, graph):
    model, cfg = _model(tmp_path, "bfloat16", geometry=ENGINE_GEOMETRY, use_hip_graph=graph, gpu_mem_utilization=0.5,
                        max_batch_size=4, tuning=dict(decode_engine=True))
    assert model._engine is not None, "the engine must take this geometry on an MI355X"
    prompts = _prompts(cfg["vocab_size"], (21,))
    pattern = "[0-9]{3}-[a-f]{3}"
    cur = _cursor(model, "regex", pattern, END)
    toks, logits, rows = _drive(model, prompts, [0], [cur], steps=10)
    assert cur.complete and re.fullmatch(pattern.encode(), cur.text) and len(toks) >= 2
    _, raw, _ = _drive(model, prompts, [1], None, steps=len(toks) - 1, forced=toks[:-1])
    pool = _pool_ref(model)
    for k, (got, plain, idx) in enumerate(zip(logits, raw, rows)):
        assert torch.equal(bits_of(got.cpu()), bits_of(ref_apply(plain.cpu(), pool, idx))), k
        assert toks[k][0] == _first_argmax(got[0]), k
    assert model._engine is not None and model.engine_fallbacks == 0      # every decode step ran on the engine
    model.guide_store.release(cur.guide)


def test_guides_are_refused_on_the_host_where_they_cannot_run(tmp_path):
    model, cfg = _model(tmp_path, use_hip_graph=False)
    prompts = _prompts(cfg["vocab_size"], (8,))
    cur = _cursor(model, "tokens", [1, 2, 3])
    with pytest.raises(ValueError, match="ignore_kvcache"):
        model.forward(prompts, [0], [], ignore_kvcache=True, guides=[cur])
    with pytest.raises(ValueError, match="aligned"):
        model.forward(prompts, [0], [], guides=[cur, None])
    with pytest.raises(ValueError, match="no guides"):
        model.forward_verify([[1, 2]], [0], [0], guides=[cur])
    model.guide_store.release(cur.guide)
    with pytest.raises(ValueError, match="not held"):
        model.forward(prompts, [0], [], guides=[cur])                # released: nobody holds it
    assert model.gpu_block_manager.host.num_allocated(0) == 0            # nothing was allocated, nothing launched
    # a missing vocabulary with the option on is an error at start-up
    with pytest.raises(RuntimeError, match="no vocabulary"):
        _model(tmp_path, vocab=False)
    off, _ = _model(tmp_path, states=0, vocab=False)
    assert off.guide_store is None and off._guide_masks is None
    with pytest.raises(ValueError, match="guided_max_states"):
        off.forward(prompts, [0], [], guides=[cur])


def test_nothing_asked_nothing_launched(tmp_path, monkeypatch):
    from swiftllm_amd import _hip
    seen = []
    inner = _hip.call

    def spy(name, *args):
        seen.append(name)
        return inner(name, *args)
    monkeypatch.setattr(_hip, "call", spy)

    def trace(model, prompts, how):
        del seen[:]
        seqs = [0, 1, 2]
        kw = {"none": {"guides": None}, "all_none": {"guides": [None] * 3}, "absent": {}}[how]
        toks = [model.forward(prompts, seqs, [], **kw)]
        lens = [len(p) for p in prompts]
        for _ in range(3):
            lens = [n + 1 for n in lens]
            toks.append(model.forward([[t] for t in toks[-1]], seqs, lens, **kw))
        model.free_seqs_resources(seqs)
        return toks, list(seen)

    model, cfg = _model(tmp_path, use_hip_graph=False)
    prompts = _prompts(cfg["vocab_size"])
    want_toks, want = trace(model, prompts, "absent")
    assert want and "swl_logits_mask" not in want and "swl_guide_build_masks" not in want
    for how in ("none", "all_none"):
        assert trace(model, prompts, how) == (want_toks, want)
    # the option off (the configuration of before, spelled out or not): the same launches again
    for states in (0, None):
        off, _ = _model(tmp_path, states=states, vocab=False, use_hip_graph=False)
        assert trace(off, prompts, "absent") == (want_toks, want)
        assert trace(off, prompts, "all_none") == (want_toks, want)
        del off
    # under the graph: a plain run after a guided one replays the graph it captured before, entry point for entry point
    model, cfg = _model(tmp_path, use_hip_graph=True)
    trace(model, prompts, "absent")                      # (captures the plain graph)
    plain_toks, plain = trace(model, prompts, "absent")  # ... and this is what its replay launches
    captures = model.replay.captures
    cur = _cursor(model, "tokens", [5, 6, 7])
    del seen[:]
    _drive(model, prompts, [0, 1, 2], [None, cur, None], 3)
    assert seen.count("swl_guide_build_masks") == 0      # (an allowed-token guide: its row is written by the host)
    assert seen.count("swl_logits_mask") == 1 + 2        # the prefill, the warm-up run and the capture of the guided graph
    assert model.replay.captures == captures + 1
    cur2 = _cursor(model, "regex", "[0-9]+")
    del seen[:]
    _drive(model, prompts, [0, 1, 2], [cur2, None, None], 3)
    assert seen.count("swl_guide_build_masks") == 1 and seen.count("swl_logits_mask") == 1     # built once; graph replayed
    assert trace(model, prompts, "absent") == (plain_toks, plain)
    assert "swl_logits_mask" not in plain and model.replay.captures == captures + 1


# ---- the engine -----------------------------------------------------------------------------------------------------------
def test_engine_serves_guided_and_plain_requests(tmp_path):
    from swiftllm_amd import Engine, RawRequest
    model, cfg = _model(tmp_path, use_hip_graph=True)
    vocab = model.guide_store.vocab
    prompts = _prompts(cfg["vocab_size"], (11, 25, 6, 14))
    date = "[0-9]{2}:[0-9]{2}"
    sps = [_sp(guided_regex=date, stop_token_ids=END), None, _sp(guided_choice=("yes", "no", "maybe")), None]

    async def serve(raws):
        eng = Engine(model.engine_config, model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        done = await asyncio.wait_for(asyncio.gather(*(eng.add_request_and_wait(r) for r in raws)), timeout=120)
        loops.cancel()
        return done
    done = asyncio.run(serve([RawRequest("", 12, p, sampling_params=sp) for p, sp in zip(prompts, sps)]))
    texts = []
    for req, out in done:
        assert req.error is None and 1 <= len(out) <= 12
        texts.append(b"".join(vocab.token_bytes(t) or b"" for t in out))
    assert len(done[1][1]) == len(done[3][1]) == 12                      # the plain ones ran to output_len
    assert re.fullmatch(date.encode(), texts[0]) and len(done[0][1]) < 12
    assert texts[2] in (b"yes", b"no", b"maybe") and len(done[2][1]) < 12
    assert all(g.refs == 0 for g in model.guide_store.resident()) and len(model.guide_store.resident()) == 2
