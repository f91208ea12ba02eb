"""Per-token logprobs on the GPU: csrc/logprobs.hip against fp64, the model's scored steps against the tapped logits of
the same step, and the engine against the direct model run.

Reference: `log_softmax` of the row in float64 (NaN elements ignored) for the values; `np.lexsort((idx, -f))` — value
descending, id ascending, NaN last — for the ids and the rank, which are compared EXACTLY on every case.

Tolerance of a logprob: |lp - ref| <= 2e-5 + 2^-22 |ref|. The first term bounds the sum: at most 128 serial + 6 + 16 tree
additions (149 + 6 + 16 at n = 152064) over terms from a <= 2-ulp expf give about 150 * 2^-24 = 9e-6 relative on the sum,
which is absolute on its logarithm; the second covers the two roundings (m + log s, f - lse) of quantities no larger than
|lp|. Plain fp32 log_softmax stays within 1.5e-5 of fp64 on the random rows below."""
import asyncio
import math

import numpy as np
import pytest
import torch

from oracle import synth

import _lora as L

pytestmark = pytest.mark.gpu

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
CANARY_LP, CANARY_ID, BAND = 1234.5, -77, 64


def _K():
    from swiftllm_amd.worker.kernels import logprobs
    return logprobs


def _tol(ref):
    return 2e-5 + 2.0 ** -22 * abs(ref)


def _reference(row: torch.Tensor):
    """(order, lp) of one 16-bit row on the CPU: ids by (value descending, id ascending, NaN last), and the fp64
    log-softmax over the elements that are not NaN (all NaN when the row's maximum is not finite)."""
    f = row.float().numpy().astype(np.float64)
    order = np.lexsort((np.arange(f.size), -f))
    live = ~np.isnan(f)
    m = f[live].max() if live.any() else np.nan
    if not np.isfinite(m):
        return order, np.full(f.size, np.nan)
    lsm = torch.log_softmax(torch.from_numpy(np.where(live, f, -np.inf)), 0).numpy()
    return order, np.where(live, lsm, np.nan)


def _launch(x, chosen, top_n, cap=20):
    """One launch over x [rows, n] (device, any row stride) into buffers with canary bands; returns host arrays
    (lp [rows, cap + 1], ids, rank) after checking that the bands are intact."""
    K = _K()
    rows = x.shape[0]
    cols = cap + 1
    dev = x.device
    lp = torch.full((2 * BAND + rows * cols,), CANARY_LP, dtype=torch.float32, device=dev)
    ids = torch.full((2 * BAND + rows * cols,), CANARY_ID, dtype=torch.int32, device=dev)
    rank = torch.full((2 * BAND + rows,), CANARY_ID, dtype=torch.int32, device=dev)
    args = K.LogprobArgs(torch.tensor(top_n, dtype=torch.int32, device=dev), lp[BAND:BAND + rows * cols].view(rows, cols),
                         ids[BAND:BAND + rows * cols].view(rows, cols), rank[BAND:BAND + rows], cap)
    K.token_logprobs(x, torch.tensor(chosen, dtype=torch.int64, device=dev), args)
    lp, ids, rank = lp.cpu().numpy(), ids.cpu().numpy(), rank.cpu().numpy()
    for buf, canary in ((lp, CANARY_LP), (ids, CANARY_ID), (rank, CANARY_ID)):
        assert (buf[:BAND] == canary).all() and (buf[-BAND:] == canary).all(), "a canary band was written"
    return lp[BAND:-BAND].reshape(rows, cols), ids[BAND:-BAND].reshape(rows, cols), rank[BAND:-BAND]


def _check_value(got, want, what):
    if math.isnan(want):
        assert math.isnan(got), what
    elif math.isinf(want):
        assert got == want, what
    else:
        assert abs(got - want) <= _tol(want), (what, got, want)


def _check_row(ref, n, c, want_n, lp, ids, rank, cap=20, what=""):
    """One row of a launch against its reference; want_n < 0: the row did not ask and holds canaries only."""
    order, ref_lp = ref
    if want_n < 0:
        assert (lp == CANARY_LP).all() and (ids == CANARY_ID).all() and rank == CANARY_ID, what
        return
    top = min(want_n, cap)
    assert (lp[top + 1:] == CANARY_LP).all() and (ids[top + 1:] == CANARY_ID).all(), what
    if 0 <= c < n:
        assert ids[0] == c and rank == 1 + int(np.nonzero(order == c)[0][0]), (what, c, rank)
        _check_value(float(lp[0]), float(ref_lp[c]), what)
    else:
        assert ids[0] == -1 and rank == 0 and math.isnan(lp[0]), what
    have = min(top, n)
    assert ids[1:have + 1].tolist() == order[:have].tolist(), (what, ids[1:have + 1], order[:have])
    for j in range(have):
        _check_value(float(lp[1 + j]), float(ref_lp[order[j]]), (what, j))
    assert (ids[have + 1:top + 1] == -1).all() and np.isnan(lp[have + 1:top + 1]).all(), what     # a row narrower than N


def _check(x, chosen, top_n, out, cap=20, refs=None, what=""):
    xc = x.cpu()
    refs = refs or [_reference(xc[r]) for r in range(x.shape[0])]
    for r in range(x.shape[0]):
        _check_row(refs[r], x.shape[1], chosen[r], top_n[r], out[0][r], out[1][r], out[2][r], cap, (what, r))
    return refs


TOP_N = (-1, 0, 1, 5, 20, 20)


@pytest.mark.parametrize("dtype", list(DTYPES.values()))
@pytest.mark.parametrize("n", [8, 1003, 4097, 32000, 128256, 152064])
def test_parity(dtype, n):
    g = torch.Generator().manual_seed(n)
    for scale in (1.0, 4.0, 12.0):
        x = (torch.randn(6, n, generator=g) * scale).to(dtype).cuda()
        refs = None
        argmax = x.float().argmax(1).cpu().tolist()
        rand = torch.randint(0, n, (6,), generator=g).tolist()
        for mode, chosen in (("argmax", argmax), ("random", rand), ("first", [0] * 6), ("last", [n - 1] * 6)):
            refs = _check(x, chosen, TOP_N, _launch(x, chosen, TOP_N), refs=refs, what=(scale, mode))


# The kernel holds the first 131072 columns of a row in registers and re-reads the rest on every pass (csrc/logits_keys.h).
# The four tests below run at their own small width with `off` = 0 and again on a Qwen-wide row whose columns below
# `off` = 131072 are ballast that never reaches the top: the tied values, the peak, the non-finite entries and the picked
# tokens then all lie in the streamed part. (`off` = 0 leaves every input and every assertion as it was.)
HELD = 131072
WIDE = (151936, HELD)


def _cases(small_n, wide=(WIDE,)):
    """(dtype, n, off): the test's own width under the ids it always had, then the streamed widths."""
    dtypes = list(DTYPES.values())
    return [pytest.param(d, small_n, 0, id=f"dtype{i}") for i, d in enumerate(dtypes)] + \
        [pytest.param(d, n, off, id=f"{n}-{off}-dtype{i}") for n, off in wide for i, d in enumerate(dtypes)]


def _ballast(rows, off, g):
    """[rows, off] values below anything the tests put behind them (about -8 +- 2.5)."""
    return torch.randn(rows, off, generator=g) * 0.5 - 8.0


@pytest.mark.parametrize("dtype,n,off", _cases(4097))
def test_ties(dtype, n, off):
    t = n - off
    g = torch.Generator().manual_seed(1)
    levels = torch.tensor([-1.5, 0.25, 0.5, 3.0])
    quant = levels[torch.randint(0, 4, (3, t), generator=g)]
    const = torch.full((1, t), 0.75)
    zeros = torch.where(torch.rand(2, t, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    zeros[1, ::5] = -1.0
    head = _ballast(6, off, g).to(dtype)
    x = torch.cat([head, torch.cat([quant, const, zeros]).to(dtype)], 1).cuda()
    top_n = (20, 5, 1, 20, 20, 7)
    chosen = [off + c for c in (t - 1, 17, 0, 1234, 99, 4000)]
    lp, ids, rank = out = _launch(x, chosen, top_n)
    _check(x, chosen, top_n, out)
    # the constant row: every logprob is -log n (-log of the row's mass in units of one constant element, with ballast),
    # the top ids are 0 .. N-1, the rank of c is c + 1
    assert ids[3, 1:21].tolist() == list(range(off, off + 20)) and rank[3] == 1234 + 1
    log_mass = math.log(t + float(torch.exp(head[3].double() - 0.75).sum()))
    assert off or log_mass == math.log(n)
    assert np.abs(lp[3, :21] + log_mass).max() <= _tol(log_mass)
    # +0 and -0 are one value: ids ascending whatever the sign
    assert ids[4, 1:21].tolist() == list(range(off, off + 20)) and rank[4] == 100


@pytest.mark.parametrize("dtype,n,off", _cases(32000))
def test_peaked(dtype, n, off):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, n, generator=g)
    x[0, off + 777] = x[0].max() + 60.0
    x[1, n - 1] = x[1].max() + 60.0
    x = x.to(dtype).cuda()
    chosen, top_n = [off + 777, off + 5], (20, 3)
    lp, ids, rank = out = _launch(x, chosen, top_n)
    _check(x, chosen, top_n, out)
    assert rank[0] == 1 and abs(lp[0, 0]) <= 2e-5 and ids[1, 1] == n - 1 and lp[1, 0] < -50


@pytest.mark.parametrize("dtype,n,off", _cases(4097))
def test_non_finite(dtype, n, off):
    t = n - off
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, t, generator=g) * 3
    x[0] = -math.inf                            # all -inf
    x[1, 100] = math.inf                        # one +inf
    x[2, ::7] = math.nan                        # NaNs at every 7th element
    x[3, torch.randperm(t, generator=g)[:t - 9]] = -math.inf    # 9 finite elements: -inf entries reach the top 20
    x[4] = math.nan                             # all NaN
    head = _ballast(5, off, g) - 12.0           # (below every finite element of rows 1 and 2)
    head[0] = head[3] = -math.inf
    head[4] = math.nan
    x = torch.cat([head, x], 1).to(dtype).cuda()
    top_n = (5, 5, 20, 20, 3)
    finite3 = torch.isfinite(x[3].float()).nonzero().flatten().cpu().tolist()
    assert len(finite3) == 9 and finite3[0] >= off
    chosen = [off + 3, off + 100, off + 7, finite3[0], off + 2]         # (7: a NaN element of row 2)
    lp, ids, rank = out = _launch(x, chosen, top_n)
    _check(x, chosen, top_n, out)
    assert np.isnan(lp[0, :6]).all() and ids[0, 1:6].tolist() == [0, 1, 2, 3, 4] and rank[0] == off + 4
    assert np.isnan(lp[1, :6]).all() and ids[1, 1] == off + 100 and rank[1] == 1
    assert math.isnan(lp[2, 0]) and np.isfinite(lp[2, 1:21]).all() and all(i >= off and (i - off) % 7 for i in ids[2, 1:21])
    assert sorted(ids[3, 1:10].tolist()) == finite3 and np.isfinite(lp[3, 1:10]).all()
    assert (lp[3, 10:21] == -math.inf).all()    # -inf entries report -inf and never precede a finite element
    # a -inf chosen element of a healthy row
    banned = next(i for i in range(off, n) if i not in finite3)
    lp, ids, rank = _launch(x[3:4], [banned], (0,))
    assert lp[0, 0] == -math.inf and rank[0] == 9 + 1 + banned - sum(1 for i in finite3 if i < banned)


@pytest.mark.parametrize("dtype,n,off", _cases(1003, (WIDE, (HELD + 3, HELD))))
@pytest.mark.parametrize("pad", [1, 8, 5])      # (n + 5 = 1008, 131080: 16-byte loads with a partial last vector)
def test_layout(dtype, pad, n, off):
    g = torch.Generator().manual_seed(4)
    store = torch.randn(6, n + pad, generator=g) * 4
    if off:
        store[:, off:] += 12.0                  # (the streamed columns hold the top of every row)
    store = store.to(dtype).cuda()
    store[:, n:] = 100.0                        # the padding between rows would win every comparison
    x = store[:, :n]
    assert x.stride(0) == n + pad
    chosen = [off + 5 if off + 5 < n else n - 2, -1, n, off, n - 1, 2 ** 40]    # -1, n and 2^40: outside the row
    out = _launch(x, chosen, TOP_N)             # (canary bands, non-asking rows and columns past top_n[r]: _launch, _check)
    _check(x, chosen, TOP_N, out)
    # top_n[r] > n_cap is clamped to n_cap
    top_n = (9, 5, -1, 7, 0, 3)
    base = min(off, n - 7)
    chosen = [base + c for c in (1, 2, 3, 4, 5, 6)]
    _check(x, chosen, top_n, _launch(x, chosen, top_n, cap=5), cap=5)
    _check(x, chosen, top_n, _launch(x, chosen, top_n, cap=0), cap=0)
    # the list-taking form
    args = _K().token_logprobs(x, torch.tensor(chosen, device="cuda"), [3, None, 0, 20, None, 1])
    got = (args.lp.cpu().numpy(), args.ids.cpu().numpy(), args.rank.cpu().numpy())
    refs = [_reference(x[r].cpu()) for r in range(6)]
    for r, want in enumerate((3, None, 0, 20, None, 1)):
        if want is not None:
            order = refs[r][0]
            assert got[1][r, :want + 1].tolist() == [chosen[r]] + order[:want].tolist()
            _check_value(float(got[0][r, 0]), float(refs[r][1][chosen[r]]), r)
    assert args.top_n.cpu().tolist() == [3, -1, 0, 20, -1, 1]


def test_invariance():
    n = 128256
    g = torch.Generator().manual_seed(5)
    big = (torch.randn(64, n, generator=g) * 4).to(torch.bfloat16).cuda()
    row = big[37:38].clone()
    c = int(torch.randint(0, n, (1,), generator=g))
    alone20 = _launch(row, [c], (20,))
    alone3 = _launch(row, [c], (3,))
    chosen = torch.randint(0, n, (64,), generator=g).tolist()
    chosen[37] = c
    top_n = [(r * 7) % 22 - 1 for r in range(64)]
    top_n[37] = 20
    crowd = _launch(big, chosen, top_n)
    again = _launch(big, chosen, top_n)
    for a, b in zip(crowd, again):              # two launches: bit-equal (NaN-free inputs, canaries included)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for other in (alone3, (crowd[0][37:38], crowd[1][37:38], crowd[2][37:38])):
        assert other[2][0] == alone20[2][0]
        assert np.array_equal(other[0][0, :4].view(np.int32), alone20[0][0, :4].view(np.int32))
        assert np.array_equal(other[1][0, :4], alone20[1][0, :4])
    assert np.array_equal(crowd[0][37].view(np.int32), alone20[0][0].view(np.int32))
    assert np.array_equal(crowd[1][37], alone20[1][0])


# ---- the model ------------------------------------------------------------------------------------------------------------
def _model(tmp_path, dtype="float16", **kw):
    from swiftllm_amd import EngineConfig, LlamaModel
    cfg = synth.make_config(**synth.SMALL64)
    path = tmp_path / f"ckpt_{dtype}"
    if not path.exists():
        synth.write_model_dir(str(path), cfg, synth.make_state_dict(cfg, seed=9, dtype=DTYPES[dtype]))
    base = dict(model_path=str(path), use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=64,
                max_seqs_in_block_table=40, max_blocks_per_seq=16, max_batch_size=8, max_tokens_in_batch=1024, dtype=dtype)
    base.update(kw)
    model = LlamaModel(EngineConfig(**base))
    model.load_weights()
    model.init_kvcache_and_swap(200)
    return model, cfg


def _sp(*a, **kw):
    from swiftllm_amd import SamplingParams
    return SamplingParams(*a, **kw)


def _prompts(vocab, sizes=(9, 30, 4)):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in sizes]


def _check_scores(scores, sps, tokens, logits):
    """`last_logprobs` of one step against the tapped logits of that step."""
    if all(sp is None or sp.logprobs is None for sp in sps):
        assert scores is None
        return
    assert len(scores) == len(sps)
    xc = logits.cpu()
    for r, (sp, s) in enumerate(zip(sps, scores)):
        if sp is None or sp.logprobs is None:
            assert s is None
            continue
        order, ref_lp = _reference(xc[r])
        assert s.token_id == tokens[r] and s.rank == 1 + int(np.nonzero(order == tokens[r])[0][0])
        _check_value(s.logprob, float(ref_lp[tokens[r]]), r)
        assert [i for i, _ in s.top] == order[:sp.logprobs].tolist()
        for (i, v), j in zip(s.top, order):
            _check_value(v, float(ref_lp[j]), (r, i))


def _run(model, prompts, sps_of_step, steps=6, seqs=None, check=True):
    """Prefill + `steps` decode steps; sps_of_step(k) gives the params of step k (None: no sampling_params argument).
    Returns (tokens per step, tapped logits per step, last_logprobs per step)."""
    seqs = seqs or list(range(len(prompts)))
    model.post_layer.logits_tap = tap = []
    toks, logits, scores = [], [], []
    lens = [len(p) for p in prompts]
    for k in range(steps + 1):
        sps = sps_of_step(k)
        kw = {} if sps is None else {"sampling_params": sps}
        if k == 0:
            toks.append(model.forward(prompts, seqs, [], **kw))
        else:
            lens = [n + 1 for n in lens]
            toks.append(model.forward([[t] for t in toks[-1]], seqs, lens, **kw))
        logits.append(tap[-1][:len(seqs)].clone())
        scores.append(model.last_logprobs)
        if check:
            _check_scores(scores[-1], sps or [None] * len(seqs), toks[-1], logits[-1])
    model.free_seqs_resources(seqs)
    model.post_layer.logits_tap = None
    return toks, logits, scores


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("graph", [True, False])
def test_model_scores_against_the_tapped_logits(tmp_path, dtype, graph):
    model, cfg = _model(tmp_path, dtype, use_hip_graph=graph)
    prompts = _prompts(cfg["vocab_size"])
    asking = [_sp(logprobs=5), None, _sp(logprobs=0)]
    plain_toks, plain_logits, plain_scores = _run(model, prompts, lambda k: None)
    assert plain_scores == [None] * 7
    toks, logits, scores = _run(model, prompts, lambda k: asking)
    assert all(s is not None and s[1] is None and len(s[0].top) == 5 and s[2].top == () for s in scores)
    # the same tokens, from the same logits, as the run that asks for nothing
    assert toks == plain_toks
    for a, b in zip(logits, plain_logits):
        assert torch.equal(a, b)
    # N changes mid-run (a look-ahead miss on the replay path): still right, still the same tokens
    changed = [_sp(logprobs=2), _sp(logprobs=20), None]
    toks2, _, scores2 = _run(model, prompts, lambda k: asking if k < 3 else changed if k < 5 else None)
    assert toks2 == plain_toks and len(scores2[3][1].top) == 20 and scores2[3][2] is None and scores2[6] is None


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_model_scores_sampled_and_biased_rows_on_the_adjusted_logits(tmp_path, dtype):
    model, cfg = _model(tmp_path, dtype, use_hip_graph=True)
    v = cfg["vocab_size"]
    prompts = _prompts(v, (12, 7))
    keep = [3, 50, 51, 200, 201, 202, 300, 400, 500, 511]
    bias = {t: -math.inf for t in range(v) if t not in keep}
    sps = [_sp(0.8, top_k=40, seed=5, logprobs=3), _sp(logit_bias=bias, logprobs=20)]
    toks, logits, scores = _run(model, prompts, lambda k: sps)
    bare = [_sp(0.8, top_k=40, seed=5), _sp(logit_bias=bias)]
    assert _run(model, prompts, lambda k: bare)[0] == toks           # the same draws and picks without the field
    for step, tok in zip(scores, toks):
        top = step[1].top
        assert tok[1] in keep and sorted(i for i, _ in top[:10]) == keep and all(math.isfinite(x) for _, x in top[:10])
        banned = [t for t in range(v) if t not in keep][:10]
        assert [i for i, _ in top[10:]] == banned and all(x == -math.inf for _, x in top[10:])
    assert len({t[0] for t in toks}) > 1                             # (the sampled row is not a constant stream)


def test_model_scores_fp8_kv_lora_and_chunked_steps(tmp_path):
    asking = [_sp(logprobs=4), _sp(logprobs=1)]
    model, cfg = _model(tmp_path, kv_cache_dtype="fp8_e4m3", use_hip_graph=True)
    prompts = _prompts(cfg["vocab_size"], (40, 11))
    _run(model, prompts, lambda k: asking, steps=1)
    del model
    model, cfg = _model(tmp_path, max_loras=1, use_hip_graph=True)
    model.load_lora("a", state_dict=L.random_adapter(cfg, 16, 1, std=0.2), config=L.adapter_config(16))
    model.post_layer.logits_tap = tap = []
    toks = model.forward(prompts, [0, 1], [], sampling_params=asking, lora=["a", None])
    _check_scores(model.last_logprobs, asking, toks, tap[-1])
    toks = model.forward([[t] for t in toks], [0, 1], [41, 12], sampling_params=asking, lora=["a", None])
    _check_scores(model.last_logprobs, asking, toks, tap[-1])
    model.free_seqs_resources([0, 1])
    # a chunked prompt: both chunks are scored by the model (the engine keeps the last one's)
    model.forward([prompts[0][:16]], [3], [], sampling_params=asking[:1])
    assert model.last_logprobs[0] is not None
    toks = model.forward([prompts[0][16:]], [3], [], sampling_params=asking[:1], prefill_ctx_lens=[16])
    _check_scores(model.last_logprobs, asking[:1], toks, tap[-1])
    model.free_seqs_resources([3])
    model.post_layer.logits_tap = None


def test_a_run_that_asks_for_nothing_launches_what_it_launched(tmp_path, monkeypatch):
    from swiftllm_amd import _hip
    model, cfg = _model(tmp_path, use_hip_graph=True)
    prompts = _prompts(cfg["vocab_size"])
    seen = []
    inner = _hip.call

    def spy(name, *args):
        seen.append(name)
        return inner(name, *args)
    monkeypatch.setattr(_hip, "call", spy)
    quiet = [None, _sp(stop_token_ids=(1,)), _sp(0.7, seed=3)]       # params, but nobody asks
    plain_toks = _run(model, prompts, lambda k: None)[0]
    captures = model.replay.captures
    assert captures == len(model.replay.graphs) == 1 and "swl_logprobs" not in seen
    _run(model, prompts, lambda k: quiet)
    assert "swl_logprobs" not in seen
    quiet_captures = model.replay.captures
    seen.clear()
    _run(model, prompts, lambda k: [_sp(logprobs=1)] * 3)
    assert seen.count("swl_logprobs") == 1 + 2      # the prefill, the warm-up run and the capture of the scored graph
    scored_captures = model.replay.captures
    assert scored_captures == quiet_captures + 1
    # ... and afterwards: the plain run replays the graph it captured, entry point for entry point
    seen.clear()
    assert _run(model, prompts, lambda k: None)[0] == plain_toks
    assert model.replay.captures == scored_captures and "swl_logprobs" not in seen


# ---- the engine ----------------------------------------------------------------------------------------------------------
def test_engine_delivers_what_the_model_reports(tmp_path):
    from swiftllm_amd import Engine, RawRequest
    model, cfg = _model(tmp_path, use_hip_graph=True)
    prompts = _prompts(cfg["vocab_size"], (11, 25, 6))
    sps = [_sp(logprobs=5), _sp(logprobs=0), None]
    steps = 7
    toks, _, scores = _run(model, prompts, lambda k: sps, steps=steps - 1)

    async def serve(raws):
        eng = Engine(model.engine_config, model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        done = await asyncio.wait_for(asyncio.gather(*(eng.add_request_and_wait(r) for r in raws)), timeout=120)
        loops.cancel()
        return done
    done = asyncio.run(serve([RawRequest("", steps, p, sampling_params=sp) for p, sp in zip(prompts, sps)]))
    for r, (req, out) in enumerate(done):
        assert req.error is None and out == [t[r] for t in toks]
        if sps[r] is None:
            assert req.output_logprobs == []
        else:
            assert req.output_logprobs == [s[r] for s in scores]
            assert [lp.token_id for lp in req.output_logprobs] == out
    bare = asyncio.run(serve([RawRequest("", steps, p) for p in prompts]))
    assert [out for _, out in bare] == [out for _, out in done]
