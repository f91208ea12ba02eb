"""Seeded sampling on the GPU: csrc/sampling.hip against the numpy reference of its contract (tests/_sampling_ref.py),
its distribution, its determinism, and the model and engine paths that use it."""
import asyncio

import numpy as np
import pytest
import torch

from oracle import synth
from _sampling_ref import filtered_softmax, kept_set, sample_row

pytestmark = pytest.mark.gpu

VOCAB = 128256


def _sp(*a, **kw):
    from swiftllm_amd import SamplingParams
    return SamplingParams(*a, **kw)


def _sample(logits, params, pos):
    from swiftllm_amd.worker.kernels.sampling import sample_rows
    out = sample_rows(logits, params, pos)
    torch.cuda.synchronize()
    return out.cpu().tolist()


def _greedy_ref(f):
    return sample_row(f, 0.0, 0, 1.0, 0, 0)[0]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n", [VOCAB, 32000, 1000, 4097])
def test_greedy_rows_equal_argmax(dtype, n):
    from swiftllm_amd.worker.kernels.sampling import argmax_rows
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(8, n, generator=g) * 3).to(dtype)
    x[1, 5] = x[1, n - 1] = x[1].max() + 1          # tie: the lowest index wins
    x[2] = float("nan")
    x[3] = float("-inf")
    x[4, ::7] = float("nan")
    x[5] = 0.0
    x[5, n // 2] = -0.0
    x[6, :] = -1.0
    x[6, n - 1] = float("-0.0")                     # the only maximum is the last element (scalar tail when n % 8)
    xd = x.cuda()
    params = [None, _sp(0.0), None, None, None, None, None, None]
    mixed = [p if r % 2 == 0 else _sp(0.9, seed=r) for r, p in enumerate(params)]
    pos = list(range(8))
    got = _sample(xd, params, pos)
    got_mixed = _sample(xd, mixed, pos)
    want = [_greedy_ref(row) for row in x.double().numpy()]
    assert got == want
    assert [got_mixed[r] for r in range(0, 8, 2)] == [want[r] for r in range(0, 8, 2)]
    if n % 8 == 0:
        assert got == argmax_rows(xd).cpu().tolist()
    assert got_mixed[3] == 0                        # an all -inf row has nothing to draw from, sampled or not


def _rows(x, params, pos, top_p):
    """(reference token, decided?) per row."""
    out = []
    for r, f in enumerate(x.double().numpy()):
        sp = params[r]
        tok, margin = sample_row(f, sp.temperature, sp.top_k, sp.top_p, sp.seed, pos[r])
        stable = True
        if 0 < top_p < 1:
            stable = np.array_equal(kept_set(f, sp.temperature, sp.top_k, sp.top_p, -1e-4),
                                    kept_set(f, sp.temperature, sp.top_k, sp.top_p, 1e-4))
        out.append((tok, margin > 1e-3 and stable))
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
# (T, top_k, top_p, logit scale): a nucleus of thousands of near-equal weights moves with any 1e-4 of p, so the top-p
# cases use wider logits (nuclei of a few to tens of tokens) to have rows whose nucleus is decided
@pytest.mark.parametrize("mode", [(1.0, 0, 1.0, 2.5), (0.8, 50, 1.0, 2.5), (1.2, 0, 0.9, 8.0), (0.7, 100, 0.8, 6.0)])
def test_kernel_matches_reference(dtype, mode):
    temp, top_k, top_p, scale = mode
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(32, VOCAB, generator=g) * scale).to(dtype)
    params = [_sp(temp, top_k, top_p, seed=1000 + r) for r in range(32)]
    pos = [17 + 3 * r for r in range(32)]
    got = _sample(x.cuda(), params, pos)
    ref = _rows(x, params, pos, top_p)
    decided = [r for r, (_, ok) in enumerate(ref) if ok]
    assert len(decided) >= 0.9 * 32, len(decided)
    assert [got[r] for r in decided] == [ref[r][0] for r in decided]
    for r, f in enumerate(x.double().numpy()):
        assert kept_set(f, temp, top_k, 1.0)[got[r]]                        # inside the top-k set, exactly
        assert kept_set(f, temp, top_k, top_p, 1e-4)[got[r]]                # inside the nucleus of p + 1e-4


def _chi2_ok(counts, probs):
    from scipy.stats import chi2
    n = counts.sum()
    exp = probs * n
    big = exp >= 5
    obs_b = np.append(counts[big], counts[~big].sum())
    exp_b = np.append(exp[big], exp[~big].sum())
    keep = exp_b > 0
    assert obs_b[~keep].sum() == 0          # nothing drawn outside the filtered support
    obs_b, exp_b = obs_b[keep], exp_b[keep]
    stat = ((obs_b - exp_b) ** 2 / exp_b).sum()
    return stat, chi2.ppf(0.999, max(1, obs_b.size - 1))


@pytest.mark.parametrize("shape", ["v1024", "peaked"])
@pytest.mark.parametrize("temp", [0.7, 1.3])
@pytest.mark.parametrize("filt", [(0, 1.0), (50, 1.0), (0, 0.9)])
def test_distribution_matches_filtered_softmax(shape, temp, filt):
    top_k, top_p = filt
    g = torch.Generator().manual_seed(3)
    if shape == "v1024":
        row = (torch.randn(1024, generator=g) * 1.5).to(torch.bfloat16)
    else:
        row = torch.randn(VOCAB, generator=g).to(torch.bfloat16)
        row[torch.randint(0, VOCAB, (24,), generator=g)] = torch.linspace(6, 9, 24).to(torch.bfloat16)
    rows = 16384
    x = row.cuda().unsqueeze(0).expand(rows, -1).contiguous()
    from swiftllm_amd.worker.kernels.sampling import SampleArgs, sample_rows
    dev = x.device
    seeds = torch.stack((torch.arange(rows, dtype=torch.int32), torch.zeros(rows, dtype=torch.int32)), 1)
    args = SampleArgs(torch.full((rows,), temp, device=dev), torch.full((rows,), top_k, dtype=torch.int32, device=dev),
                      torch.full((rows,), top_p, device=dev), seeds.to(dev).contiguous(),
                      torch.full((rows,), 5, dtype=torch.int32, device=dev))
    toks = sample_rows(x, args, None).cpu().numpy()
    probs = filtered_softmax(row.double().numpy(), temp, top_k, top_p)
    stat, limit = _chi2_ok(np.bincount(toks, minlength=row.numel()).astype(np.float64), probs)
    assert stat < limit, (stat, limit)


def test_determinism_and_row_independence():
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(32, VOCAB, generator=g) * 2).to(torch.bfloat16).cuda()
    params = [_sp(1.0, 40 if r % 3 == 0 else 0, 0.9 if r % 2 else 1.0, seed=77 + r) for r in range(32)]
    pos = [100 + r for r in range(32)]
    a, b = _sample(x, params, pos), _sample(x, params, pos)
    assert a == b
    # row 17's draw alone (row 0 of a batch of 1) and moved to another row of a batch of 32
    assert _sample(x[17:18].clone(), params[17:18], pos[17:18]) == [a[17]]
    perm = list(range(32))
    perm[3], perm[17] = perm[17], perm[3]
    y = x[perm].contiguous()
    c = _sample(y, [params[i] for i in perm], [pos[i] for i in perm])
    assert c[3] == a[17] and c[17] == a[3]
    assert len(set(a)) > 16                     # different seeds, different draws


# ---- the model ------------------------------------------------------------------------------------------------------------
def _model(tmp_path, **kw):
    from swiftllm_amd import EngineConfig, LlamaModel
    cfg = synth.make_config(**synth.SMALL64)
    path = tmp_path / "ckpt"
    if not path.exists():
        synth.write_model_dir(str(path), cfg, synth.make_state_dict(cfg, seed=9))
    base = dict(model_path=str(path), use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=64,
                max_seqs_in_block_table=40, max_blocks_per_seq=16, max_batch_size=32, max_tokens_in_batch=1024)
    base.update(kw)
    model = LlamaModel(EngineConfig(**base))
    model.load_weights()
    model.init_kvcache_and_swap(200)
    return model, cfg


def _stream(model, prompt, sp, steps=16, sid=3, others=0, swap_at=None, piggy_at=None, vocab=None):
    """The 16 tokens the sequence `sid` draws, with `others` further sequences in its batch."""
    g = torch.Generator().manual_seed(99)
    other_prompts = [torch.randint(0, vocab, (int(n),), generator=g).tolist()
                     for n in torch.randint(3, 40, (others,), generator=g)]
    at = others // 2
    ids = other_prompts[:at] + [prompt] + other_prompts[at:]
    seqs = list(range(10, 10 + at)) + [sid] + list(range(10 + at, 10 + others))
    sps = [_sp(0.9, seed=500 + i) if i % 2 else None for i in range(others)]
    sps = sps[:at] + [sp] + sps[at:]
    toks = model.forward(ids, seqs, [], sampling_params=sps)
    lens = [len(p) for p in ids]
    out = [toks[at]]
    for step in range(1, steps):
        if step == swap_at:
            model.swap_out_seqs([sid])
            model.swap_in_seqs([sid])
        lens = [n + 1 for n in lens]
        if step == piggy_at:
            extra = torch.randint(0, vocab, (21,), generator=g).tolist()
            toks = model.forward([extra] + [[t] for t in toks], [30] + seqs, lens,
                                 sampling_params=[_sp(1.1, seed=5)] + sps)[1:]
            model.free_seqs_resources([30])
        else:
            toks = model.forward([[t] for t in toks], seqs, lens, sampling_params=sps)
        out.append(toks[at])
    model.free_seqs_resources(seqs)
    return out


def test_model_seeded_stream_is_the_same_everywhere(tmp_path):
    eager, cfg = _model(tmp_path, use_hip_graph=False)
    v = cfg["vocab_size"]
    prompt = list(range(5, 40, 3))
    sp = _sp(0.8, top_p=0.95, seed=2024)
    want = _stream(eager, prompt, sp, vocab=v)
    assert len(set(want)) > 1
    assert _stream(eager, prompt, sp, others=23, vocab=v) == want
    assert _stream(eager, prompt, sp, swap_at=8, vocab=v) == want
    assert _stream(eager, prompt, sp, others=5, piggy_at=6, vocab=v) == want
    del eager
    graph, _ = _model(tmp_path, use_hip_graph=True)
    assert _stream(graph, prompt, sp, vocab=v) == want
    assert _stream(graph, prompt, sp, others=23, vocab=v) == want
    assert _stream(graph, prompt, sp, others=23, swap_at=9, vocab=v) == want
    graph.replay.lookahead = False
    assert _stream(graph, prompt, sp, others=7, vocab=v) == want


def test_model_mixed_batch_greedy_rows_and_prefill_position(tmp_path):
    from swiftllm_amd.worker.kernels.sampling import sample_rows
    model, cfg = _model(tmp_path, use_hip_graph=True)
    v = cfg["vocab_size"]
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, v, (n,), generator=g).tolist() for n in (9, 30, 4, 17)]
    seqs = [0, 1, 2, 3]

    def run(sps):
        model.post_layer.logits_tap = []
        toks = [model.forward(prompts, seqs, [], sampling_params=sps)]
        logits0 = model.post_layer.logits_tap[0].clone()
        lens = [len(p) for p in prompts]
        for _ in range(6):
            lens = [n + 1 for n in lens]
            toks.append(model.forward([[t] for t in toks[-1]], seqs, lens, sampling_params=sps))
        model.free_seqs_resources(seqs)
        model.post_layer.logits_tap = None
        return toks, logits0
    greedy, _ = run(None)
    sps = [None, _sp(1.0, seed=8), _sp(0.0), _sp(0.6, top_k=20, seed=9)]
    mixed, logits0 = run(sps)
    for r in (0, 2):                            # greedy rows bit-equal to the all-greedy forward
        assert [t[r] for t in mixed] == [t[r] for t in greedy]
    # the prefill row drew at pos = prompt length
    again = sample_rows(logits0, sps, [len(p) for p in prompts]).cpu().tolist()
    assert again == mixed[0]


def test_engine_seeded_requests(tmp_path):
    from swiftllm_amd import Engine, RawRequest
    model, cfg = _model(tmp_path, use_hip_graph=True, max_batch_size=8)
    v = cfg["vocab_size"]
    g = torch.Generator().manual_seed(12)
    prompts = [torch.randint(0, v, (n,), generator=g).tolist() for n in (11, 25, 6, 40, 3)]
    seeded = _sp(0.9, top_k=64, top_p=0.95, seed=31337)

    async def serve(raws):
        eng = Engine(model.engine_config, model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        done = await asyncio.wait_for(asyncio.gather(*(eng.add_request_and_wait(r) for r in raws)), timeout=120)
        loops.cancel()
        return [toks for _, toks in done]
    alone = asyncio.run(serve([RawRequest("", 12, prompts[0], sampling_params=seeded)]))[0]
    crowd = asyncio.run(serve([RawRequest("", 9, p) for p in prompts[1:3]]
                              + [RawRequest("", 12, prompts[0], sampling_params=seeded)]
                              + [RawRequest("", 14, p, sampling_params=_sp(1.0)) for p in prompts[3:]]))
    assert crowd[2] == alone
    greedy = asyncio.run(serve([RawRequest("", 8, p) for p in prompts[:3]]))
    zero_t = asyncio.run(serve([RawRequest("", 8, p, sampling_params=_sp(0.0, top_k=3)) for p in prompts[:3]]))
    assert zero_t == greedy
    unseeded = asyncio.run(serve([RawRequest("", 12, prompts[1], sampling_params=_sp(1.0)) for _ in range(3)]))
    assert len({tuple(t) for t in unseeded}) == 3
