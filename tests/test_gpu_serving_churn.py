"""One churned scenario with every option on, served by the real Engine on a real LlamaModel, held to the closed form.

Chunked prefill, piggybacking, prompt-lookup speculation, swapping, seeded sampling, logits processing, stop tokens and
graph replay each have their own tests, one option at a time. Here they run through each other (tests/_churn.py: 15
requests arriving over ~100 steps on a pool that overflows), on the decisive checkpoint, whose greedy streams are known
in advance whatever the schedule does. Per case:
  * streams: every request with an expectation has error None and exactly its expected stream (the stop-token request
    holds one position — where its second stop token is banned — to "not that token"; every other position is exact);
  * coverage: the conditions C2 of tests/test_serving_churn_host.py hold for the trace of the REAL run, and with graph
    replay on also: a look-ahead hit, a prepared look-ahead dropped, a capture after replay.drop_graphs();
  * KV audit: when a request finishes, and before its blocks go, K and V of every (layer, position, kv-head) of its
    prompt + outputs[:-1] are read through the allocator's host mirror and compared with the pools of the CPU oracle after
    ONE whole-prompt forward of the same tokens: max|d| <= TAU * max|row|, TAU = 1/8. A stale, misplaced or unwritten
    row is unrelated data and differs by the row's own magnitude; rounding differs by a few units of 2^-8 (bfloat16) or
    2^-11 (float16). This reads what the copy head (position p - 19 of layer 0 only) never does: the slots rejected drafts
    wrote and decode steps overwrote, slots that went to the host and came back, slots stored by chunks;
  * end state: both pools free on the host mirror and on the device, no surplus marks, no token histories, the
    engine's swap counters equal to the trace's;
  * a second serving on the same model object (graph cache populated, buffers grown): the same streams, the same audit,
    the same schedule, and every free sampled passenger draws exactly its first-run stream.

Measured on MI355X, worst audit ratio max|d| / max|row| over all rows of the 13 audited requests: float16 0.00162
(3.3 x 2^-11), bfloat16 0.0137 (3.5 x 2^-8) — the same figure in the calm control, in both churned servings, with graph
replay and without (anything above 1/32 would be a finding to explain, not a reason to widen TAU). Coverage of the real
run, all four cases: 2 swaps (one partly fed prompt, one decoding and speculated request), 30 verify steps (23 with a
whole draft accepted, 12 with a rejection, 6 across a block), buckets 1 / 2 / 8, 7 sampled, 6 processed and 19
sampled-and-processed decode steps, 10 recycled ids; with graphs 38 look-ahead hits, 20 prepared steps dropped, 10
captures (6 after a drop), 4 in the second serving; no divergence from the host dry run; passengers identical 2 / 2.
A case takes 0.3 s (eager) to 1.7 s (graphs).
FP8 pools: no case. Decided on the CPU with the fake-quant oracle of tests/test_gpu_kv_fp8.py (K and V stored as
dequant(quant(.)), every prompt token past the first 32-token chunk fed as a decode step so that it attends to the
quantised pool, as an FP8 chunk does), teacher-forced along all 13 expected streams, 416 output positions: the closed form
holds at every one of them, but the rule for adding the case — top-2 gap >= 4 x the fake-quant oracle's logit distance
to the 16-bit oracle — fails at 2 positions in float16 and 1 in bfloat16 (worst distance / gap 0.269 and 0.292 against
0.25; the gap is ~0.48 there, the distance 0.13 - 0.14). The checkpoint does not survive the quantisation with the margin
an exact-id assertion needs, so the case is left out.
"""
import pytest
import torch

import _churn
from oracle import synth
from oracle.ref_model import RefLlamaModel

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
TAU = 1.0 / 8


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """One checkpoint directory per dtype for the whole module."""
    made = {}

    def get(dtype):
        if dtype not in made:
            cfg, sd, _ = _churn.decisive(dtype)
            made[dtype] = synth.write_model_dir(str(tmp_path_factory.mktemp("churn_" + dtype)), cfg, sd)
        return made[dtype]
    return get


def _model(path, dtype, sc, **kw):
    from swiftllm_amd import EngineConfig, LlamaModel
    opts = dict(sc.engine)
    opts.update(kw)
    model = LlamaModel(EngineConfig(model_path=path, dtype=dtype, **opts))
    model.load_weights()
    model.init_kvcache_and_swap(sc.num_gpu_blocks)
    return model


# ---- the KV audit -----------------------------------------------------------------------------------------------------
_ORACLES, _REF_KV = {}, {}


def _reference_kv(dtype, tokens):
    """K and V [L, tokens, KVH, D] (fp32) the CPU oracle stores for one whole-prompt forward of `tokens`; computed once
    per (dtype, tokens) and shared by every case."""
    key = (dtype, tuple(tokens))
    if key not in _REF_KV:
        from swiftllm_amd import EngineConfig, LlamaModelConfig
        if dtype not in _ORACLES:
            cfg, sd, _ = _churn.decisive(dtype)
            ecfg = EngineConfig(model_path="", use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=0,
                                max_seqs_in_block_table=2, max_blocks_per_seq=16, max_batch_size=2, max_tokens_in_batch=1024)
            ref = RefLlamaModel(LlamaModelConfig(cfg), ecfg, sd, getattr(torch, dtype))
            ref.init_kvcache_and_swap(16)
            _ORACLES[dtype] = ref
        ref = _ORACLES[dtype]
        ref.forward([list(tokens)], [0], [])
        nb = -(-len(tokens) // 16)
        blocks = ref.gpu_block_manager.block_table[0, :nb].long()
        _REF_KV[key] = tuple(_rows(pool[blocks], len(tokens)) for pool in (ref.k_cache, ref.v_cache))
        ref.free_seqs_resources([0])
    return _REF_KV[key]


def _rows(blocks, n):
    """[nb, L, KVH, 16, D] -> [L, n, KVH, D] fp32 on the CPU."""
    nb, L, KVH, bs, D = blocks.shape
    return blocks.permute(1, 0, 3, 2, 4).reshape(L, nb * bs, KVH, D)[:, :n].float().cpu()


def _audit(model, dtype, req, sid):
    """Worst max|d| / max|row| over the K and V rows of one finishing sequence; asserts every row inside TAU."""
    tokens = list(req.prompt_token_ids) + list(req.output_token_ids[:-1])
    n = len(tokens)
    blocks = model.gpu_block_manager.get_block_ids_host(sid)
    nb = -(-n // 16)
    assert len(blocks) >= nb, f"sequence {sid}: {len(blocks)} blocks for {n} resident tokens"
    idx = torch.tensor(blocks[:nb], dtype=torch.long, device="cuda")
    worst = 0.0
    for name, pool, want in zip("KV", (model.k_cache, model.v_cache), _reference_kv(dtype, tokens)):
        got = _rows(pool[idx], n)
        ratio = (got - want).abs().amax(-1) / want.abs().amax(-1)          # [L, n, KVH]
        assert torch.isfinite(ratio).all()
        top = float(ratio.max())
        if top > TAU:
            layer, pos, head = (int(x) for x in torch.unravel_index(ratio.argmax(), ratio.shape))
            raise AssertionError(f"{name} of sequence {sid} (prompt {req.prompt_len} + {len(req.output_token_ids)} outputs): "
                                 f"layer {layer} position {pos} kv-head {head} differs from a plain forward's by {top:.3f} "
                                 f"of the row's magnitude (TAU {TAU}); rows over TAU: {int((ratio > TAU).sum())}")
        worst = max(worst, top)
    return worst


def _assert_end_state(model, eng, c):
    for mgr in (model.gpu_block_manager, model.cpu_block_manager):
        assert mgr.num_free_blocks == mgr.num_blocks, mgr.device_name
        assert not any(mgr.host.seq_blocks.values()), (mgr.device_name, mgr.host.seq_blocks)
        assert not mgr.host.surplus_ok, (mgr.device_name, mgr.host.surplus_ok)
        assert bool(mgr.host.is_free.all())
        assert bool(mgr.is_block_free.all()) and int(mgr.num_seq_allocated_blocks.sum()) == 0, mgr.device_name
    assert not model._histories
    assert (eng.num_swapped_out, eng.num_swapped_in) == (c["swapped_out"], c["swapped_in"])
    _churn.assert_scheduler_empty(eng)


def _show(c):
    return ", ".join(f"{k} {sorted(v, key=str) if isinstance(v, set) else v}" for k, v in c.items() if k != "graph_keys")


def _serve_and_hold(model, dtype, sc, tag, audit=True):
    worst = [0.0, 0]

    def before_free(index, req, sid):
        if audit and sc.requests[index].exact:
            worst[0] = max(worst[0], _audit(model, dtype, req, sid))
            worst[1] += 1
    captures = model.replay.captures
    eng, reqs, rec = _churn.serve(model, model.engine_config, sc, before_free=before_free)
    c = _churn.coverage(rec.events, sc.requests)
    print(f"\n[churn {tag}] {_show(c)}; graph keys {len(c['graph_keys'])}, captures {model.replay.captures - captures}; "
          f"drafts accepted {eng.num_accepted_tokens} / {eng.num_draft_tokens}; "
          f"KV audit: worst ratio {worst[0]:.5f} over {worst[1]} sequences (TAU {TAU})")
    _churn.assert_streams(sc, reqs)
    assert not audit or worst[1] == sum(s.exact for s in sc.requests)
    _assert_end_state(model, eng, c)
    return eng, reqs, rec, c


def _host_shape(sc, perm):
    from swiftllm_amd import EngineConfig
    ecfg = EngineConfig(model_path="", **sc.engine)
    return _churn.shape_of(_churn.serve(_churn.ClosedFormModel(ecfg, perm, sc.num_gpu_blocks), ecfg, sc)[2].events)


@pytest.mark.parametrize("use_hip_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_churned_scenario_gives_the_closed_form_and_leaves_nothing_behind(checkpoint, dtype, use_hip_graph):
    _, _, perm = _churn.decisive(dtype)
    sc = _churn.build_scenario(perm, use_hip_graph=use_hip_graph)
    model = _model(checkpoint(dtype), dtype, sc)
    tag = f"{dtype} {'graph' if use_hip_graph else 'eager'}"
    eng, reqs, rec, c = _serve_and_hold(model, dtype, sc, tag + ", first serving")
    _churn.assert_coverage(c, real_graphs=use_hip_graph)
    # (a diagnostic, not an assertion: the allocator-backed draft clipping may legitimately differ from the bookkeeping)
    real, host = _churn.shape_of(rec.events), _host_shape(sc, perm)
    at = next((i for i, (a, b) in enumerate(zip(real, host)) if a != b), None if len(real) == len(host) else min(len(real), len(host)))
    print(f"[churn {tag}] divergence from the host dry run: " + ("none" if at is None else f"at call {at}: {real[at:at + 1]} "
                                                                                          f"against {host[at:at + 1]}"))
    # ---- the same scenario again on the same model object: graphs warm, buffers grown
    eng2, reqs2, rec2, c2 = _serve_and_hold(model, dtype, sc, tag + ", second serving")
    assert _churn.shape_of(rec2.events) == real
    same = 0
    for s, a, b in zip(sc.requests, reqs, reqs2):
        if not s.exact:
            assert a.output_token_ids == b.output_token_ids, "a passenger's second stream differs from its first"
            same += 1
    print(f"[churn {tag}] passengers with identical first and second streams: {same} / {same}")
    assert same == sum(not s.exact for s in sc.requests) > 0


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_calm_control_of_the_kv_audit(checkpoint, dtype):
    """Every request with an expectation served ALONE: one whole-prompt prefill, then decode steps. Its stream and the
    same audit: the ratio the churned runs are read against."""
    _, _, perm = _churn.decisive(dtype)
    sc = _churn.build_scenario(perm)
    model = _model(checkpoint(dtype), dtype, sc, max_prefill_chunk=0, speculative_ngram=0, max_tokens_in_batch=256)
    from swiftllm_amd.server import RawRequest, Request
    worst = 0.0
    for s in sc.requests:
        if not s.exact:
            continue
        req = Request(RawRequest("", s.output_len, list(s.prompt), sampling_params=s.sampling_params))
        kw = dict(sampling_params=[req.sampling_params]) if req.sampling_params is not None else {}
        req.output_token_ids.append(model.forward([req.prompt_token_ids], [0], [], **kw)[0])
        while not req.is_finished():
            req.output_token_ids.append(model.forward([[req.output_token_ids[-1]]], [0], [req.num_tokens()], **kw)[0])
        assert s.mismatch(req.output_token_ids) is None, (s.kind, s.mismatch(req.output_token_ids))
        worst = max(worst, _audit(model, dtype, req, 0))
        model.free_seqs_resources([0])
    print(f"\n[churn {dtype}, calm control] KV audit: worst ratio {worst:.5f} (TAU {TAU})")
    assert model.gpu_block_manager.num_free_blocks == sc.num_gpu_blocks and not model._histories
