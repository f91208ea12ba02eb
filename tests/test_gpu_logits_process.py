"""Logits processing on the GPU: csrc/logits_adjust.hip against the fp32 reference of its contract (tests/_logits_ref.py)
bit for bit, in the arena, run after run; its composition with the sampler; and the model and engine paths that use it."""
import asyncio
import functools
import math

import numpy as np
import pytest
import torch

from oracle import synth
from _arena import Op, run_case
from _logits_ref import adjust_ref, f32, history_entries, min_p_gap, same_bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# (n, row_stride): 16-byte rows; 16-byte rows with a scalar tail; 2-byte rows (the scalar path); the Llama-3 vocabulary
WIDTHS = [(1000, 1008), (1003, 1008), (1003, 1011), (128256, 128264), (151936, 151936), (152069, 152072)]
IN_PROMPT = -2 ** 31
INF = math.inf
PAD = 7.0       # what the padding columns hold


def _sp(*a, **kw):
    from swiftllm_amd import SamplingParams
    return SamplingParams(*a, **kw)


def _ulp(v, dtype, step):
    """The positive `dtype` value `step` ulps from v."""
    t = torch.tensor([v], dtype=dtype)
    return float((t.view(torch.int16) + step).view(dtype)[0])


@functools.lru_cache(maxsize=None)
def _case(dtype, n, seed=0):
    """Five rows: (0) every kind of entry, repetition penalty 1 (off) with the other two, min-p; (1) nothing to do; (2) min-p
    only, with elements planted at, one ulp above and one ulp below max + gap; (3) an entry for EVERY id — every kind of
    meta word and bias on positive and negative logits — under repetition penalty 1.3, whose quotients and products round;
    (4) 64 entries under repetition penalty 0.5 and a min-p gap from (T, min_p). Logits have |x| in [2^-10, 2^10]. Returns the inputs and the
    reference's output, computed once."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    rows = 5
    sign = torch.where(torch.rand(rows, n, generator=g) < 0.5, -1.0, 1.0)
    x = (sign * torch.exp2(torch.rand(rows, n, generator=g) * 20 - 10)).to(dtype)
    k2 = 100
    # row 0
    x[0, 0], x[0, n - 1], x[0, k2], x[0, k2 + 1] = 3.0, -3.0, 0.75, -0.75
    x[0, 500] = x[0, 600] = float("nan")
    e0 = [  # (id, meta, bias)
        (0, IN_PROMPT | 2, 0.0), (n - 1, 1, 0.0),                       # first and last id of the row
        (k2, IN_PROMPT, 0.0), (k2 + 1, 3, 0.0),                         # the pair (2k, 2k + 1) shares a dword
        (n + 7, 1, 5.0), (-3, 1, 5.0), (2 ** 31 - 1, 0, -INF),          # out of range: skipped
        (200, IN_PROMPT, 0.0), (201, 5, 0.0), (202, IN_PROMPT | 7, 0.0),    # prompt only, output only, both
        (300, 0, 5.0), (301, 1, -100.0), (302, IN_PROMPT, -INF),        # biases
        (400, 1000, 0.0),                                               # count 1000 under freq = 0.01
        (500, 2, 1.0),                                                  # a NaN logit stays NaN
    ]
    # row 2
    gap2 = -24.0
    x[2, 7] = 1024.0
    t = 1000.0                      # = max + gap, a value of both formats
    x[2, 11], x[2, 12], x[2, 13] = t, _ulp(t, dtype, 1), _ulp(t, dtype, -1)
    x[2, n - 2], x[2, n - 1] = t, _ulp(t, dtype, -1)         # ... and in the last vector / the scalar tail
    x[2, 20] = float("nan")
    # row 3: every id once, in a shuffled order
    ids3 = torch.randperm(n, generator=g).to(torch.int32)
    kind = torch.randint(0, 4, (n,), generator=g)
    cnt = torch.randint(1, 6, (n,), generator=g)
    meta3 = torch.where(kind == 0, 0, torch.where(kind == 1, IN_PROMPT, torch.where(kind == 2, cnt, cnt | IN_PROMPT)))
    bias3 = torch.tensor([0.0, 5.0, -100.0, -INF, 0.25])[torch.randint(0, 5, (n,), generator=g)]
    # row 4
    ids4 = torch.randperm(n, generator=g)[:64].to(torch.int32)
    meta4 = torch.randint(0, 4, (64,), generator=g) | torch.where(torch.rand(64, generator=g) < 0.5, IN_PROMPT, 0)
    bias4 = torch.where(torch.rand(64, generator=g) < 0.3, 2.5, 0.0)
    ids = torch.cat([torch.tensor([e[0] for e in e0], dtype=torch.int64).to(torch.int32), ids3, ids4])
    meta = torch.cat([torch.tensor([e[1] for e in e0], dtype=torch.int64), meta3, meta4]).to(torch.int32)
    bias = torch.cat([torch.tensor([e[2] for e in e0], dtype=torch.float32), bias3, bias4.float()])
    offsets = torch.tensor([0, len(e0), len(e0), len(e0), len(e0) + n, len(e0) + n + 64], dtype=torch.int32)
    params = torch.tensor([[1.0, 0.5, 0.01, -1000.0], [1.3, 0.5, 0.01, -INF], [1.0, 0.0, 0.0, gap2],
                           [1.3, -0.3, 0.02, -INF], [0.5, 0.7, 0.05, min_p_gap(100.0, 0.001)]], dtype=torch.float32)
    want = adjust_ref(x, offsets, ids, meta, bias, params)
    return x, offsets, ids, meta, bias, params, want


def _launch(x, stride, offsets, ids, meta, bias, params, times=1):
    """Run the kernel on x placed at `stride` in a PAD-filled buffer; returns the whole buffer(s) back on the CPU."""
    from swiftllm_amd.worker.kernels.logits_process import AdjustArgs, adjust_logits
    rows, n = x.shape
    args = AdjustArgs(offsets.cuda(), ids.cuda(), meta.cuda(), bias.cuda(), params.cuda())
    outs = []
    for _ in range(times):
        buf = torch.full((rows * stride,), PAD, dtype=x.dtype, device="cuda")
        view = buf.as_strided((rows, n), (stride, 1))
        view.copy_(x)
        adjust_logits(view, args)
        torch.cuda.synchronize()
        outs.append(buf.cpu())
    return outs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,stride", WIDTHS)
def test_kernel_equals_the_reference_bit_for_bit(dtype, n, stride):
    x, offsets, ids, meta, bias, params, want = _case(dtype, n)
    rows = x.shape[0]
    buf = _launch(x, stride, offsets, ids, meta, bias, params)[0]
    got = buf.as_strided((rows, n), (stride, 1))
    for r in range(rows):
        assert same_bits(got[r], want[r]), (r, (got[r].view(torch.int16) != want[r].view(torch.int16)).nonzero()[:8])
    pad = torch.ones(rows * stride, dtype=torch.bool)
    pad.as_strided((rows, n), (stride, 1)).fill_(False)
    assert bool((buf[pad] == PAD).all())                        # the padding columns (and the out-of-range ids' targets)
    # what no entry names keeps its bits (rows 0, 1, 4), or becomes -inf and nothing else (min-p rows)
    gi, xi = got.view(torch.int16), x.view(torch.int16)
    assert torch.equal(gi[1], xi[1])
    for r in (0, 2, 4):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        named = torch.zeros(n, dtype=torch.bool)
        rid = ids[lo:hi].long()
        named[rid[(rid >= 0) & (rid < n)]] = True
        free = ~named
        assert bool(((gi[r] == xi[r]) | (got[r] == -INF))[free].all())
    # the planted elements: at max + gap and one ulp above it kept, one ulp below it removed; NaN stays NaN
    assert got[2, 11] == 1000.0 and got[2, 12] > 1000.0 and got[2, 13] == -INF
    assert got[2, n - 2] == 1000.0 and got[2, n - 1] == -INF and got[2, 7] == 1024.0
    assert torch.isnan(got[2, 20]) and torch.isnan(got[0, 500]) and torch.isnan(got[0, 600])
    assert got[0, 302] == -INF and got[3].ne(x[3]).sum() > n // 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,stride", [(1003, 1011), (1000, 1008)])
def test_kernel_in_the_arena(dtype, n, stride):
    """logits in/out at 2-byte skew, the index and parameter arrays at 4-byte skew, in a 0xFF and a 0x00 arena: the same
    bits as on plain tensors (which take the 16-byte path when the stride allows it), nothing outside the rows touched."""
    from swiftllm_amd import _hip
    x, offsets, ids, meta, bias, params, want = _case(dtype, n)
    rows = x.shape[0]
    ops = {"logits": Op(x, skew=2, stride=stride, out=True), "offsets": Op(offsets, skew=4), "ids": Op(ids, skew=4),
           "meta": Op(meta, skew=4), "bias": Op(bias, skew=4), "params": Op(params, skew=4)}

    def call(t):
        _hip.call("swl_logits_adjust", _hip.ptr(t["logits"]), rows, n, t["logits"].stride(0), _hip.dtype_code(dtype),
                  _hip.ptr(t["offsets"]), _hip.ptr(t["ids"]), _hip.ptr(t["meta"]), _hip.ptr(t["bias"]),
                  _hip.ptr(t["params"]), _hip.stream())
    out = run_case(ops, call, "cuda", sync=torch.cuda.synchronize)
    assert same_bits(out["logits"], want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_is_deterministic(dtype):
    n, stride = 128256, 128264
    x, offsets, ids, meta, bias, params, _ = _case(dtype, n)
    outs = _launch(x, stride, offsets, ids, meta, bias, params, times=8)
    first = outs[0].view(torch.int16)
    assert all(torch.equal(o.view(torch.int16), first) for o in outs[1:])


def test_wrapper_refuses_bad_edits_and_buffers():
    from swiftllm_amd.worker.kernels.logits_process import AdjustArgs, RowEdits, adjust_logits
    x = torch.zeros(2, 64, dtype=torch.float16, device="cuda")
    row = lambda ids: RowEdits(np.array(ids, np.int32), np.zeros(len(ids), np.int32), np.ones(len(ids), np.float32))
    adjust_logits(x, [row([0, 63]), None])
    assert x[0, 0] == 1 and x[0, 63] == 1 and x[1].eq(0).all() and x[0, 1:63].eq(0).all()
    for bad in ([64], [-1], [5, 5]):
        with pytest.raises(ValueError):
            adjust_logits(x, [row(bad), None])
    with pytest.raises(ValueError):
        adjust_logits(x, [row([1])])                            # one row of edits for two rows of logits
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    zf = torch.zeros(8, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        adjust_logits(x, AdjustArgs(z[:3], z[::2], z[:4], zf[:4], zf))          # a non-contiguous buffer
    with pytest.raises(ValueError):
        adjust_logits(x.t(), AdjustArgs(z[:3], z, z, zf, zf))                   # logits without unit column stride
    with pytest.raises(ValueError):
        adjust_logits(x, AdjustArgs(z[:2], z, z, zf, zf))                       # offsets for one row only


def test_composition_with_the_sampler():
    """min_p = 0.2 at T = 1 on 64 rows of the same logits, one seed each, a -inf bias on the most likely token: every draw
    lies in the reference's kept set; a greedy row with penalties takes the argmax of the reference's output."""
    from swiftllm_amd.worker.kernels.logits_process import RowEdits, adjust_logits
    from swiftllm_amd.worker.kernels.sampling import sample_rows
    n, rows = 1000, 65
    g = torch.Generator().manual_seed(4)
    base = (torch.randn(n, generator=g) * 2).to(torch.float16)
    x = base.unsqueeze(0).repeat(rows, 1)
    top = int(base.float().argmax())
    gap = min_p_gap(1.0, 0.2)
    edit = RowEdits(np.array([top, 17], np.int32), np.array([0, 0], np.int32), np.array([-INF, 5.0], np.float32),
                    min_p_gap=gap)
    pen_ids = torch.randperm(n, generator=g)[:300].to(torch.int32)
    pen = RowEdits(pen_ids.numpy(), np.full(300, 2, np.int32), np.zeros(300, np.float32), 1.5, 0.5, 0.25)
    edits = [edit] * 64 + [pen]
    offsets = torch.tensor([2 * r for r in range(65)] + [128 + 300], dtype=torch.int32)
    ids = torch.cat([torch.tensor([top, 17] * 64, dtype=torch.int32), pen_ids])
    meta = torch.cat([torch.zeros(128, dtype=torch.int32), torch.full((300,), 2, dtype=torch.int32)])
    bias = torch.cat([torch.tensor([-INF, 5.0] * 64), torch.zeros(300)])
    params = torch.tensor([[1.0, 0.0, 0.0, gap]] * 64 + [[1.5, 0.5, 0.25, -INF]], dtype=torch.float32)
    want = adjust_ref(x, offsets, ids, meta, bias, params)
    xd = adjust_logits(x.cuda(), edits)
    assert same_bits(xd.cpu(), want)
    sps = [_sp(1.0, seed=100 + r) for r in range(64)] + [None]
    toks = sample_rows(xd, sps, list(range(50, 50 + rows))).cpu().tolist()
    kept = torch.isfinite(want[0].float())
    assert 1 < int(kept.sum()) < n and not kept[top]
    assert all(kept[t] for t in toks[:64]) and top not in toks[:64]
    assert len(set(toks[:64])) > 1
    last = want[64].float()
    assert toks[64] == int((last == last.max()).nonzero()[0])


# ---- the model ------------------------------------------------------------------------------------------------------------
LENS = (5, 16, 17, 40)
STEPS = 24
SEQS = [3, 0, 5, 1]


def _model(tmp_path, dtype, graph=False, guide_vocab=None, **kw):
    from swiftllm_amd import EngineConfig, LlamaModel
    cfg = synth.make_config()           # TINY
    path = tmp_path / f"tiny_{dtype}"
    if not path.exists():
        tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
        synth.write_model_dir(str(path), cfg, synth.make_state_dict(cfg, seed=21, dtype=tdtype))
    base = dict(model_path=str(path), use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                max_seqs_in_block_table=8, max_blocks_per_seq=8, max_batch_size=4, max_tokens_in_batch=256, dtype=dtype,
                use_hip_graph=graph)
    base.update(kw)
    model = LlamaModel(EngineConfig(**base))
    if guide_vocab is not None:
        model.set_guide_vocab(guide_vocab(cfg["vocab_size"]))
    model.load_weights()
    model.init_kvcache_and_swap(40)
    model.replay.eager_in_buckets = True      # eager steps at the replay path's batch bucket and split geometry
    return model, cfg


def _prompts(vocab):
    g = torch.Generator().manual_seed(77)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in LENS]


def _params():
    """plain; greedy with all three penalties; greedy with a bias and a banned stop token; sampled with penalties and min-p"""
    return [None,
            _sp(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.1),
            _sp(logit_bias={11: 5.0, 12: -100.0, 200: 0.02}, stop_token_ids=(13, 200), min_tokens=STEPS + 10),
            _sp(0.9, seed=1234, repetition_penalty=1.2, frequency_penalty=0.05, min_p=0.1)]


def _generate(model, prompts, sps, chunk=None, tap=False):
    """Prefill (the last prompt in chunks of `chunk` when given) + STEPS decode steps. Returns the tokens per step and, with
    `tap`, the logits each token was picked from."""
    model.post_layer.logits_tap = [] if tap else None
    if chunk is None:
        toks = model.forward(prompts, SEQS, [], sampling_params=sps)
    else:
        long = prompts[-1]
        toks = model.forward(prompts[:-1] + [long[:chunk]], SEQS, [], sampling_params=sps)
        done = chunk
        while done < len(long):
            last = model.forward([long[done:done + chunk]], SEQS[-1:], [], sampling_params=sps[-1:], prefill_ctx_lens=[done])
            done += chunk
        toks = toks[:-1] + last
    out, logits = [toks], []
    if tap:
        logits.append(model.post_layer.logits_tap[-1].cpu())
    lens = [len(p) for p in prompts]
    for _ in range(STEPS):
        lens = [n + 1 for n in lens]
        toks = model.forward([[t] for t in toks], SEQS, lens, sampling_params=sps)
        out.append(toks)
        if tap:
            logits.append(model.post_layer.logits_tap[-1].cpu())
    model.free_seqs_resources(SEQS)
    model.post_layer.logits_tap = None
    return out, logits


def _count_lookahead_hits(model):
    """Wrap the model's look-ahead lookup; returns a one-element list holding the number of hits so far."""
    hits, inner = [0], model.replay.take

    def spy(*a, **kw):
        la = inner(*a, **kw)
        hits[0] += la is not None
        return la
    model.replay.take = spy
    return hits


def _expected_entries(sp, prompt, outputs):
    """The row's entries from scratch (ids, meta, bias): history under a penalty, bias, ban — one entry per id."""
    ent = {}
    if sp.penalised:
        hid, hmeta = history_entries(prompt, outputs)
        ent = {int(t): [int(m), 0.0] for t, m in zip(hid, hmeta)}
    for t, b in sp.logit_bias or ():
        ent.setdefault(t, [0, 0.0])[1] = b
    if len(outputs) < sp.min_tokens:
        for t in sp.stop_token_ids:
            ent.setdefault(t, [0, 0.0])[1] = -INF
    return (torch.tensor(list(ent), dtype=torch.int32), torch.tensor([v[0] for v in ent.values()], dtype=torch.int32),
            torch.tensor([v[1] for v in ent.values()], dtype=torch.float32))


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_model_logits_equal_the_reference_on_a_twins_raw_logits(tmp_path, dtype):
    model, cfg = _model(tmp_path, dtype)
    twin, _ = _model(tmp_path, dtype)
    prompts, sps = _prompts(cfg["vocab_size"]), _params()
    toks, logits = _generate(model, prompts, sps, tap=True)
    assert not model._histories                 # dropped with the sequences
    # the twin: no params, fed the first model's tokens
    twin.post_layer.logits_tap = []
    twin.forward(prompts, SEQS, [])
    lens = [len(p) for p in prompts]
    for step in range(STEPS):
        lens = [n + 1 for n in lens]
        twin.forward([[t] for t in toks[step]], SEQS, lens)
    raw = [t.cpu() for t in twin.post_layer.logits_tap]
    assert len(raw) == len(logits) == STEPS + 1
    changed = 0
    for step in range(STEPS + 1):
        rows = []
        for r, sp in enumerate(sps):
            outputs = [toks[k][r] for k in range(step)]
            if sp is None:
                rows.append((torch.zeros(0, dtype=torch.int32),) * 2 + (torch.zeros(0),) + ([1.0, 0.0, 0.0, -INF],))
            else:
                rows.append(_expected_entries(sp, prompts[r], outputs)
                            + ([sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty,
                                min_p_gap(sp.temperature, sp.min_p)],))
        offsets = torch.tensor(np.cumsum([0] + [len(x[0]) for x in rows]), dtype=torch.int32)
        want = adjust_ref(raw[step], offsets, torch.cat([x[0] for x in rows]), torch.cat([x[1] for x in rows]),
                          torch.cat([x[2] for x in rows]), torch.tensor([x[3] for x in rows], dtype=torch.float32))
        got = logits[step]
        assert same_bits(got, want), step
        changed += int((got.view(torch.int16) != raw[step].view(torch.int16)).sum())
        assert torch.equal(got[0].view(torch.int16), raw[step][0].view(torch.int16))       # the plain row: raw
        for r in (0, 1, 2):                     # greedy rows: the lowest index among the maxima
            f = got[r].float()
            assert toks[step][r] == int((f == f.max()).nonzero()[0]), (step, r)
        assert torch.isfinite(got[3].float())[toks[step][3]]            # the sampled row drew inside the kept set
        assert toks[step][2] not in (13, 200) and got[2, 13] == -INF and got[2, 200] == -INF
    assert changed >= 2 * (STEPS + 1)           # at the least the two banned ids of row 2, every step


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_model_streams_are_the_same_on_every_path(tmp_path, dtype):
    model, cfg = _model(tmp_path, dtype)
    prompts, sps = _prompts(cfg["vocab_size"]), _params()
    want, _ = _generate(model, prompts, sps)
    plain, _ = _generate(model, prompts, [None] * 4)
    assert [t[0] for t in want] == [t[0] for t in plain]                # the plain row is the all-plain stream
    assert [t[1] for t in want] != [t[1] for t in plain]                # ... and the penalties change theirs
    assert _generate(model, prompts, sps, chunk=16)[0] == want          # the 40-token prompt in chunks of 16
    model.replay.lookahead = False
    assert _generate(model, prompts, sps)[0] == want
    del model
    graph, _ = _model(tmp_path, dtype, graph=True)
    hits = _count_lookahead_hits(graph)
    assert _generate(graph, prompts, sps)[0] == want                    # replay + look-ahead hits
    assert graph.replay.captures > 0
    assert hits[0] >= STEPS - 1         # every decode step but the first is the prepared one: entries uploaded on a hit
    assert _generate(graph, prompts, sps, chunk=16)[0] == want
    graph.replay.lookahead = False
    hits[0] = 0
    assert _generate(graph, prompts, sps)[0] == want                    # replay, every step planned afresh
    assert hits[0] == 0


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_entry_buffer_growth_drops_the_graphs_and_the_stream_goes_on(tmp_path, dtype):
    """The entry buffer starts at 8 entries and goes up in pieces beyond 16 words (both lowered on the instance), so the
    penalised rows outgrow it at the prefill and again in the middle of the decode steps, on a look-ahead hit: the graphs
    captured against the old buffer are dropped, the step is captured again, and the tokens are the eager stream's."""
    eager, cfg = _model(tmp_path, dtype)
    prompts, sps = _prompts(cfg["vocab_size"]), _params()
    want, _ = _generate(eager, prompts, sps)
    del eager
    graph, _ = _model(tmp_path, dtype, graph=True)
    from swiftllm_amd.worker.step_logits import StagedInts
    stage = graph._logits
    stage.min_edit_cap, stage.one_copy_words = 8, 16
    stage.edits = StagedInts(graph.replay.drop_graphs)     # (allocated at load with the class's capacity)
    stage.edit_rows = 0
    hits = _count_lookahead_hits(graph)
    log = []            # per forward: (buffer words, captures so far, look-ahead hits so far, graphs cached before the call)
    inner = graph.forward

    def spy(*a, **kw):
        cached = len(graph.replay.graphs)
        out = inner(*a, **kw)
        log.append((stage.edits.dev.numel(), graph.replay.captures, hits[0], cached))
        return out
    graph.forward = spy
    assert _generate(graph, prompts, sps)[0] == want
    assert len(log) == STEPS + 1 and log[0][0] > 16                     # beyond one copy from the first step on
    grown = [k for k in range(2, len(log)) if log[k][0] > log[k - 1][0]]
    assert grown, [w for w, _, _, _ in log]                             # the buffer grew between two decode steps
    k = grown[0]
    assert log[k][2] == log[k - 1][2] + 1                               # ... on a look-ahead hit
    assert log[k][3] >= 1 and log[k][1] == log[k - 1][1] + 1            # a graph was cached; the step was captured again


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_every_staged_buffer_can_move_under_captured_graphs(tmp_path, dtype):
    """All four logits options across one batch — a plain row, a penalised greedy row that asks for logprobs, a guided row
    and a seeded sampled row with min-p — on a replay model whose four staged buffers start over at ONE row (the edit
    buffer at 8 entries, in pieces beyond 16 words): every buffer outgrows itself under captured graphs, and the stream and
    its logprobs are the eager model's."""
    from _guided_ref import synthetic_vocab
    from swiftllm_amd.guided import GuideCursor, guide_key
    from swiftllm_amd.worker.step_logits import StagedInts
    allowed = [3, 40, 41, 97, 200, 251]
    # (the penalised row is the 5-token prompt: one entry per token it has seen, so 8 entries and then 16 are outgrown
    # within the first dozen decode steps)
    sps = [_sp(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.1, logprobs=5), None,
           _sp(allowed_token_ids=allowed), _sp(0.9, seed=1234, min_p=0.1)]

    def stream(model, watch=None):
        cur = GuideCursor(model.guide_store.acquire(guide_key("tokens", allowed, ())))
        guides, lens = [None, None, cur, None], list(LENS)
        toks = [model.forward(prompts, SEQS, [], sampling_params=sps, guides=guides)]
        scores = [model.last_logprobs]
        for _ in range(STEPS):
            cur.advance(toks[-1][2])
            lens = [n + 1 for n in lens]
            toks.append(model.forward([[t] for t in toks[-1]], SEQS, lens, sampling_params=sps, guides=guides))
            scores.append(model.last_logprobs)
            if watch is not None:
                watch()
        model.free_seqs_resources(SEQS)
        model.guide_store.release(cur.guide)
        return toks, scores

    def build(graph):
        return _model(tmp_path, dtype, graph=graph, guided_max_states=8, guide_vocab=lambda v: synthetic_vocab(v, seed=3))

    eager, cfg = build(False)
    prompts = _prompts(cfg["vocab_size"])
    want, want_scores = stream(eager)
    assert all(t[2] in allowed for t in want) and len({t[3] for t in want}) > 1
    del eager
    graph, _ = build(True)
    stage, drop = graph._logits, graph.replay.drop_graphs
    stage.min_edit_cap, stage.one_copy_words, stage.edit_rows = 8, 16, 0
    stage.sampling, stage.edits = StagedInts(drop), StagedInts(drop)
    stage.scores = StagedInts(drop, idle=-1, tail=stage.scores.tail)
    stage.guide_rows = StagedInts(drop, idle=-1)
    stage.reserve(1)
    rows = lambda: (stage.sampling.words // 5, stage.edit_rows, stage.scores.words, stage.guide_rows.words)   # noqa: E731
    assert rows() == (1, 1, 1, 1)
    hits = _count_lookahead_hits(graph)
    log = []        # per decode step: (edit buffer words, captures so far)
    got, got_scores = stream(graph, lambda: log.append((stage.edits.words, graph.replay.captures)))
    assert got == want
    for step, (a, b) in enumerate(zip(got_scores, want_scores)):
        assert [s is None for s in a] == [s is None for s in b] == [False, True, True, True], step
        a, b = a[0], b[0]
        assert (a.token_id, a.rank, [i for i, _ in a.top]) == (b.token_id, b.rank, [i for i, _ in b.top]), step
        for x, y in zip((a.logprob,) + tuple(v for _, v in a.top), (b.logprob,) + tuple(v for _, v in b.top)):
            assert abs(x - y) <= 2e-5 + 2.0 ** -22 * abs(y), (step, x, y)       # (test_gpu_logprobs._tol)
    assert all(n >= 4 for n in rows()), rows()
    grown = [k for k in range(1, len(log)) if log[k][0] > log[k - 1][0]]
    assert grown and log[grown[0]][1] > log[grown[0] - 1][1]            # a growth between decode steps: captured again
    assert hits[0] >= STEPS - 1         # every decode step but the first is the prepared one, the growing ones too


def test_model_refuses_rows_without_a_history_and_verify_on_tracked_sequences(tmp_path):
    model, cfg = _model(tmp_path, "float16")
    pen = _sp(repetition_penalty=1.2)
    t = model.forward([[1, 2, 3]], [0], [])
    with pytest.raises(ValueError):
        model.forward([t], [0], [4], sampling_params=[pen])            # processing starts at the prefill
    model.free_seqs_resources([0])
    t = model.forward([[1, 2, 3]], [0], [], sampling_params=[pen])
    with pytest.raises(ValueError):
        model.forward([t], [0], [6], sampling_params=[pen])            # out of step with the history
    assert model.max_draft_tokens > 0           # (TINY: two q-heads per kv-head, eight tokens per verify step)
    with pytest.raises(ValueError):
        model.forward_verify([t + [5]], [0], [3])
    t = model.forward([t], [0], [4], sampling_params=[pen])             # ... and the refused calls changed nothing
    assert len(model._histories[0]) == 4
    # a step that raises after the histories moved takes the move back: the same call can be made again
    inner = model._forward_step

    def failing(*args, **kw):
        raise RuntimeError("no blocks")
    model._forward_step = failing
    with pytest.raises(RuntimeError):
        model.forward([[7, 8], t], [2, 0], [5], sampling_params=[pen, pen])
    model._forward_step = inner
    assert len(model._histories[0]) == 4 and 2 not in model._histories
    model.forward([[7, 8], t], [2, 0], [5], sampling_params=[pen, pen])
    assert len(model._histories[0]) == 5 and len(model._histories[2]) == 2
    model.free_seqs_resources([2])
    with pytest.raises(ValueError):
        model.forward([[1, 2]], [1], [], sampling_params=[_sp(logit_bias={cfg["vocab_size"]: 1.0})])
    model.free_seqs_resources([0])
    assert not model._histories


# ---- the engine -----------------------------------------------------------------------------------------------------------
def test_engine_stop_tokens_and_min_tokens_on_the_decisive_checkpoint(tmp_path):
    from swiftllm_amd import Engine, RawRequest
    from test_gpu_chunked_prefill import STEPS as DSTEPS, _decisive
    model, prompts, want = _decisive(tmp_path, "bfloat16")
    # a sequence whose closed-form token at step 7 does not occur before it
    i = next(k for k in range(len(prompts)) if want[7][k] not in [want[s][k] for s in range(7)])
    stream = [want[s][i] for s in range(DSTEPS + 1)]
    t = stream[7]

    async def serve(sp):
        eng = Engine(model.engine_config, model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        req, toks = await asyncio.wait_for(eng.add_request_and_wait(RawRequest("", DSTEPS + 1, prompts[i], sampling_params=sp)),
                                           timeout=120)
        loops.cancel()
        return req, toks
    req, toks = asyncio.run(serve(_sp(stop_token_ids=(t,))))
    assert req.error is None and toks == stream[:8]
    assert model.gpu_block_manager.num_free_blocks == 40 and not model._histories
    req, toks = asyncio.run(serve(_sp(stop_token_ids=(t,), min_tokens=12)))
    assert req.error is None and toks[:7] == stream[:7] and toks[7] != t and t not in toks[:12]
    if t in toks[12:]:
        assert toks.index(t) == len(toks) - 1
    else:
        assert len(toks) == DSTEPS + 1
    assert model.gpu_block_manager.num_free_blocks == 40 and not model._histories
