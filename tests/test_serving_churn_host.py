"""The churned serving scenario (tests/_churn.py) is what it claims — on the CPU, through the real Engine and scheduler.

C2 (coverage): the scenario, replayed on the closed-form data plane, reaches every interaction the GPU test
(tests/test_gpu_serving_churn.py) is there for. These are conditions on the scenario, not measurements of the product:
arrivals and the pool size were tuned until they held.
C1 (the options do not move the decision): along the expected streams of the processed, the stop-token and the top_k=1
request, the CPU oracle's raw top-2 gap is at least 4 times the largest change the chosen penalties and bias apply to any
one logit (tests/_logits_ref.py), so "the closed form" is a fair expectation for requests whose logits are edited.
"""
import pytest
import torch

import _churn
from _logits_ref import adjust_ref, history_entries, min_p_gap
from oracle.ref_model import RefLlamaModel


def _replay():
    from swiftllm_amd import EngineConfig
    _, _, perm = _churn.decisive("float16")
    sc = _churn.build_scenario(perm)
    ecfg = EngineConfig(model_path="", **sc.engine)
    model = _churn.ClosedFormModel(ecfg, perm, sc.num_gpu_blocks)
    eng, reqs, rec = _churn.serve(model, ecfg, sc)
    return sc, model, eng, reqs, rec


def test_the_scenario_is_the_one_the_issue_describes():
    _, _, perm = _churn.decisive("float16")
    assert perm == _churn.decisive("bfloat16")[2]           # one closed form for both dtypes
    sc = _churn.build_scenario(perm)
    kinds = [s.kind for s in sc.requests]
    assert 12 <= len(kinds) <= 16
    for kind in (_churn.PLAIN, _churn.RUN, _churn.PAIRS, _churn.SAMPLED, _churn.PROCESSED, _churn.STOP, _churn.PASSENGER):
        assert kind in kinds
    e = sc.engine
    assert (e["block_size"], e["max_prefill_chunk"], e["max_batch_size"], e["speculative_ngram"]) == (16, 32, 8, 3)
    assert e["max_tokens_in_batch"] == 96 and e["num_cpu_blocks"] > 0
    for s in sc.requests:
        assert _churn.OFFSET < len(s.prompt) <= 190 and 25 <= s.output_len <= 45 and len(s.prompt) + s.output_len <= 256
        assert s.exact == (s.kind != _churn.PASSENGER)
    # the pool cannot hold the plain stretch: the scheduler must swap
    first = [s for s in sc.requests if s.arrival < _churn.S2]
    assert sum(-(-(len(s.prompt) + s.output_len) // 16) for s in first) > sc.num_gpu_blocks
    sp = next(s for s in sc.requests if s.kind == _churn.SAMPLED).sampling_params
    assert sp.top_k == 1 and sp.temperature == 0.8
    sp = next(s for s in sc.requests if s.kind == _churn.PROCESSED).sampling_params
    assert sp.greedy and sp.penalised and sp.logit_bias and sp.min_p > 0
    stop = next(s for s in sc.requests if s.kind == _churn.STOP)
    sp = stop.sampling_params
    assert sp.min_tokens == 5 and len(stop.expected) == 12 and stop.expected[11] in sp.stop_token_ids
    assert stop.expected[stop.banned_at] in sp.stop_token_ids and stop.banned_at < sp.min_tokens
    assert build_is_seeded(perm)


def build_is_seeded(perm):
    a, b = _churn.build_scenario(perm), _churn.build_scenario(perm)
    return [s.prompt for s in a.requests] == [s.prompt for s in b.requests]


def test_host_replay_gives_every_stream_and_reaches_every_interaction():
    """Streams, accounting back to empty, and C2. The counters are printed."""
    sc, model, eng, reqs, rec = _replay()
    _churn.assert_streams(sc, reqs)
    _churn.assert_scheduler_empty(eng)
    assert model.is_empty()
    c = _churn.coverage(rec.events, sc.requests)
    print("\n[churn, host replay] " + ", ".join(f"{k} {sorted(v) if isinstance(v, set) else v}" for k, v in c.items()))
    _churn.assert_coverage(c)
    assert (eng.num_swapped_out, eng.num_swapped_in) == (c["swapped_out"], c["swapped_in"])
    assert eng.num_verify_steps == c["verify_steps"] and eng.num_forwards == c["verify_steps"] + c["forwards"]
    assert 0 < eng.num_accepted_tokens < eng.num_draft_tokens
    # no step passed the budgets the options set
    for ev in rec.events:
        if ev["kind"] == "forward":
            assert sum(ev["n_in"][:ev["n_prefill"]]) <= 32 and sum(ev["n_in"]) <= 96 and len(ev["seq_ids"]) <= 8


def test_host_replay_is_reproducible():
    a, b = _replay(), _replay()
    assert _churn.shape_of(a[4].events) == _churn.shape_of(b[4].events)
    assert [r.output_token_ids for r in a[3]] == [r.output_token_ids for r in b[3]]


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_c1_the_options_do_not_move_the_decision(dtype):
    """The oracle, teacher-forced along the expected streams of the processed, stop-token and top_k=1 requests. At every
    output position the raw argmax is the expected token with a unique maximum; for the processed request the raw top-2
    gap is >= 4 x the largest |change| its penalties and bias make to any logit there, the adjusted argmax is the same
    token, and min_p keeps it. The stop request: its decoy is the closed-form token at an index below min_tokens (where the
    data plane bans it), its stop token first occurs at index 11."""
    from swiftllm_amd import EngineConfig, LlamaModelConfig
    cfg, sd, perm = _churn.decisive(dtype)
    tdtype = getattr(torch, dtype)
    sc = _churn.build_scenario(perm)
    picks = [next(s for s in sc.requests if s.kind == k) for k in (_churn.PROCESSED, _churn.STOP, _churn.SAMPLED)]
    steps = max(s.output_len for s in picks)
    streams = [_churn.closed_form(s.prompt, perm, steps) for s in picks]
    ecfg = EngineConfig(model_path="", use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=0,
                        max_seqs_in_block_table=4, max_blocks_per_seq=16, max_batch_size=4, max_tokens_in_batch=1024)
    ref = RefLlamaModel(LlamaModelConfig(cfg), ecfg, sd, tdtype)
    ref.init_kvcache_and_swap(3 * 16)
    ids = [0, 1, 2]
    rows = []           # per output position: raw logits [3, vocab] in the storage dtype
    toks = ref.forward([s.prompt for s in picks], ids, [])
    rows.append(ref.last_logits.to(tdtype))
    lens = [len(s.prompt) for s in picks]
    for i in range(steps - 1):
        assert toks == [st[i] for st in streams], i
        lens = [n + 1 for n in lens]
        toks = ref.forward([[st[i]] for st in streams], ids, list(lens))
        rows.append(ref.last_logits.to(tdtype))
    worst_ratio, min_gap = 0.0, float("inf")
    proc, stop, samp = picks
    sp = proc.sampling_params
    for i in range(proc.output_len):
        x = rows[i][0:1]
        top = x.float().topk(2).values[0]
        gap = float(top[0] - top[1])
        assert int(x.float().argmax()) == proc.expected[i]
        e_ids, e_meta = history_entries(proc.prompt, proc.expected[:i])
        bias = torch.zeros(len(e_ids), dtype=torch.float32)
        for tok, b in sp.logit_bias:
            assert tok in e_ids.tolist()
            bias[e_ids.tolist().index(tok)] = b
        params = torch.tensor([[sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, float("-inf")]],
                              dtype=torch.float32)
        offsets = torch.tensor([0, len(e_ids)], dtype=torch.int32)
        y = adjust_ref(x, offsets, e_ids, e_meta, bias, params)
        change = float((y.float() - x.float()).abs().max())
        assert change > 0                                   # the options really edit this row
        assert gap >= 4 * change, (i, gap, change)
        assert int(y.float().argmax()) == proc.expected[i]
        params[0, 3] = min_p_gap(1.0, sp.min_p)             # (a greedy row's min_p is inert; at T = 1 it keeps the winner too)
        kept = adjust_ref(x, offsets, e_ids, e_meta, bias, params)
        assert torch.isfinite(kept[0, proc.expected[i]].float())
        worst_ratio, min_gap = max(worst_ratio, change / gap), min(min_gap, gap)
    print(f"\n[C1 {dtype}] processed request: smallest raw top-2 gap {min_gap:.4f}, largest change / gap {worst_ratio:.4f} "
          f"(bound 0.25)")
    for which, spec in ((1, stop), (2, samp)):
        for i in range(len(spec.expected)):
            x = rows[i][which].float()
            top = x.topk(2).values
            assert int(x.argmax()) == streams[which][i] and float(top[0] - top[1]) > 0, (spec.kind, i)
    full = streams[1]
    stops = stop.sampling_params.stop_token_ids
    assert full[_churn.DECOY_INDEX] in stops and _churn.DECOY_INDEX < stop.sampling_params.min_tokens
    assert [i for i, t in enumerate(full[:_churn.STOP_INDEX + 1]) if t in stops] == [_churn.DECOY_INDEX, _churn.STOP_INDEX]
    assert stop.expected == full[:_churn.STOP_INDEX + 1]
    assert samp.expected == streams[2][:samp.output_len]
