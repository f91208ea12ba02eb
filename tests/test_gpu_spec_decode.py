"""Prompt-lookup speculative decoding on the GPU: swl_paged_attn_verify against fp64 on designed score profiles (held to the
decode kernel's own bounds, garbage in every slot it must not read), causality, determinism; LlamaModel.forward_verify
against the oracle decoding the same tokens teacher-forced; exact ids on the decisive checkpoint, with rejected drafts
left in the pool; the Engine with the option on.

Bounds of the kernel test are those tests/test_gpu_attention_extremes.py derives for paged decode (the same arithmetic:
fp32 scores and sums, P as a hi + lo pair, one output rounding): general |o - o64| <= (2 u + 2 * 2^-22 log2(e) S) vmax,
a 30-nat needle EXACTLY its key's v, an exact tie within 1 ulp of (v_a + v_b) / 2."""
import asyncio
import types

import pytest
import torch

from _attn_cases import attn64, make_kv, make_q, scores64
from oracle import synth
from oracle.ref_model import RefLlamaModel
from test_gpu_attention_extremes import PAGED_SPECS, _check_rows
from test_gpu_chunked_prefill import DECISIVE, LAYER, NUM_LAYERS, OFFSET, _engine_config, _fill_pools, _make_model

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace
DTYPES = [torch.float16, torch.bfloat16]
# H, KVH, D, split width
CASES = [(32, 8, 128, 64), (32, 8, 128, 4096), (8, 8, 128, 512), (8, 4, 64, 128), (16, 2, 32, 1024)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _verify():
    from swiftllm_amd.worker.kernels.paged_attn import paged_attention_verify
    return paged_attention_verify


# ---- building a launch -----------------------------------------------------------------------------------------------
def _contexts(sbs):
    return [0, 1, 13, 15, 16, 17, 63, 64, 300, 1499, sbs - 2, sbs - 1]


def _new_lens(tmax):
    """n per context of _contexts: 0 .. 16 / G mixed in one launch; the full width where the rows straddle a block
    (c = 15, 63) or a split (c = sbs - 2, sbs - 1)."""
    half = max(1, tmax // 2)
    return [tmax, 1, 0, tmax, half, max(1, tmax - 1), tmax, 1, half, tmax, tmax, tmax]


def _make_seq(c, n, H, KVH, D, sbs, dtype, g, salt):
    """K/V of all c + n keys with needles at the context edge, block / split edges, first and last key; q of the n rows,
    a profile per head (PAGED_SPECS), rising ramps anchored at the last key."""
    L = c + n
    cand = [c - 1, c, 0, L - 1, 15, 16, sbs - 1, sbs, c // 2, c + n // 2, L - 2]
    needles = [[min(max(cand[(h * 3 + salt) % len(cand)], 0), L - 1) for h in range(KVH)], [0] * KVH]
    ties = [[(min(3 + h, L - 1), L - 1 - h) if L > 2 * KVH + 4 else None for h in range(KVH)]]
    k_, v_, F = make_kv(L, KVH, D, dtype, g, needles=needles, ties=ties)
    # _check_rows holds a tie row to 1 ulp of (v_a + v_b) / 2. Where 16-bit values cancel (v_a = -v_b happens now and then)
    # that target is ~0, its ulp the subnormal spacing, and the EXACT answer is already ~1e-10 away from it (what the
    # other keys add at e^-30 each): no kernel can meet it. The pairs that can tie — the planted ones, and keys 0 and 1
    # of a two-key flat row — therefore never cancel in these inputs.
    pairs = [(ab, h) for h, ab in enumerate(ties[0]) if ab is not None] + [((0, 1), h) for h in range(KVH) if L > 1]
    for (a, b), h in pairs:
        small = (v_[a, h].float() + v_[b, h].float()).abs() < 2.0 ** -16
        v_[a, h] = torch.where(small, torch.ones_like(v_[a, h]), v_[a, h])
        v_[b, h] = torch.where(small, torch.ones_like(v_[b, h]), v_[b, h])
    specs = [PAGED_SPECS[h % len(PAGED_SPECS)] for h in range(H)]
    sp = [dict(x, shift=x.get("shift", 0.0) - x["slope"] * (L - 1)) if x["kind"] == "ramp" and x["slope"] > 0 else x
          for x in specs]
    q_ = make_q(n, H, D, F, dtype, g, sp, D ** -0.5) if n else torch.zeros(0, H, D, dtype=dtype)
    return q_, k_, v_


def _state(ctxs, lens, D, sbs, seq_ids):
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0)
    total = max(c + n for c, n in zip(ctxs, lens))
    row_lens = torch.cat([c + 1 + torch.arange(n) for c, n in zip(ctxs, lens)]).to(torch.int32)
    return NS(num_prefill_seqs=len(lens), max_prefill_len=max(lens), softmax_scale=D ** -0.5,
              prefill_seq_start_locs_with_end=cu.cuda(), num_prefill_tokens=sum(lens),
              prefill_ctx_lens=torch.tensor(ctxs, dtype=torch.int32).cuda(), max_prefill_total_len=total,
              seq_ids=seq_ids.cuda(), seq_block_size=sbs, num_seq_blocks=-(-total // sbs),
              verify_row_lens=row_lens.cuda())


def _launch(seqs, ctxs, H, KVH, D, sbs, dtype, fill=0.0, pad_rows=0, only=None, repeat=1):
    """One launch over the sequences. `only`: that sequence alone, its q and o being its rows of the whole batch's
    buffers — the other sequences' rows of o must stay NaN. Returns the whole o."""
    lens = [q.shape[0] for q, _, _ in seqs]
    mbps = max(-(-(c + n) // 16) for c, n in zip(ctxs, lens)) + 3
    kc, vc, bt, seq_ids = _fill_pools(seqs, ctxs, KVH, D, dtype, fill, mbps)
    q = torch.cat([s[0] for s in seqs]).cuda()
    mc = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=NUM_LAYERS)
    lo, hi = 0, q.shape[0]
    if only is None:
        st = _state(ctxs, lens, D, sbs, seq_ids)
    else:
        lo = sum(lens[:only])
        hi = lo + lens[only]
        st = _state(ctxs[only:only + 1], lens[only:only + 1], D, sbs, seq_ids[only:only + 1])
    kcd, vcd, btd = kc.cuda(), vc.cuda(), bt.cuda()
    outs = []
    for _ in range(repeat):
        o = torch.full((q.shape[0] + pad_rows, H, D), float("nan"), dtype=dtype, device="cuda")
        _verify()(q[lo:hi], kcd, vcd, btd, o[lo:hi], mc, NS(block_size=16), st, LAYER)
        outs.append(o)
    torch.cuda.synchronize()
    return outs[0] if repeat == 1 else outs


def _reference(q_, k_, v_, D):
    n, L = q_.shape[0], k_.shape[0]
    ref = attn64(q_, k_, v_, D ** -0.5, causal=True)
    s = scores64(q_, k_, D ** -0.5)
    vis = torch.arange(L)[None, :] <= torch.arange(n)[:, None] + (L - n)
    return ref, s.masked_fill(~vis[:, None, :], float("-inf"))


# ---- 1. the kernel against fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D,sbs", CASES)
def test_verify_attention_extreme_scores_and_garbage(dtype, H, KVH, D, sbs):
    """Twelve sequences in one launch: contexts 0 .. 1499 and both sides of a split edge, n from 0 to 16 / G mixed,
    cur_layer 1 of 2, scattered block ids, reversed table rows. Three passes over the same inputs: every slot the kernel
    must not read (slots >= c + n, blocks outside the tables, the other layer) holds 0, then NaN, then +Inf; the outputs
    must be finite and inside the decode kernel's bounds each time (c_round = 2, needles exact, ties within 1 ulp).
    The measured fractions of the bounds are printed; on MI355X, the same in all three passes: the general bound at
    <= 0.42 of it (0.27 .. 0.41 over the ten cases), the needles exact, the ties at 0.5 ulp."""
    g = gen(H * 13 + D + sbs + (dtype == torch.bfloat16))
    tmax = 16 // (H // KVH)
    ctxs, lens = _contexts(sbs), _new_lens(16 // (H // KVH))
    assert max(lens) == tmax and min(lens) == 0
    seqs = [_make_seq(c, n, H, KVH, D, sbs, dtype, g, i) for i, (c, n) in enumerate(zip(ctxs, lens))]
    refs = [_reference(*sq, D) if sq[0].shape[0] else None for sq in seqs]
    for name, fill in (("zero", 0.0), ("nan", float("nan")), ("inf", float("inf"))):
        o = _launch(seqs, ctxs, H, KVH, D, sbs, dtype, fill).cpu()
        assert torch.isfinite(o.float()).all(), f"fill={name}: non-finite output"
        worst, off = [0.0, 0.0, 0.0], 0
        for (q_, k_, v_), c, n, ref in zip(seqs, ctxs, lens, refs):
            if n:
                fr = _check_rows(o[off:off + n], ref[0], ref[1], k_, v_, dtype, 2, True, 1.0,
                                 f"verify c={c} n={n} fill={name}")
                worst = [max(a, b) for a, b in zip(worst, fr)]
            off += n
        print(f"\n[verify extremes {dtype} {H}/{KVH}/{D} sbs {sbs} fill={name}] bound fractions: general {worst[0]:.3f} "
              f"tie {worst[2]:.3f}")


# ---- 2. causality, untouched rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D,sbs", [(32, 8, 128, 64), (8, 8, 128, 512), (16, 2, 32, 1024)])
def test_verify_rows_do_not_depend_on_later_keys_and_touch_nothing_else(dtype, H, KVH, D, sbs):
    """New K/V at every position > c + i leaves rows <= i bit-identical (and moves the later ones). A launch of ONE
    sequence leaves its neighbours' rows of o and the rows behind the batch as the NaN they were filled with."""
    g = gen(7 + D)
    tmax = 16 // (H // KVH)
    ctxs, lens = [13, sbs - 2, 300], [tmax, tmax, max(1, tmax - 1)]
    seqs = [_make_seq(c, n, H, KVH, D, sbs, dtype, g, i) for i, (c, n) in enumerate(zip(ctxs, lens))]
    o1 = _launch(seqs, ctxs, H, KVH, D, sbs, dtype, pad_rows=3)
    assert torch.isnan(o1[sum(lens):].float()).all() and torch.isfinite(o1[:sum(lens)].float()).all()
    for i in range(tmax - 1):
        changed = []
        for (q_, k_, v_), c, n in zip(seqs, ctxs, lens):
            k2, v2 = k_.clone(), v_.clone()
            m = max(0, n - i - 1)
            if m:
                k2[c + i + 1:] = (torch.randn(m, KVH, D, generator=g) * 3).to(dtype)
                v2[c + i + 1:] = (torch.randn(m, KVH, D, generator=g) * 3).to(dtype)
            changed.append((q_, k2, v2))
        o2 = _launch(changed, ctxs, H, KVH, D, sbs, dtype, pad_rows=3)
        off = 0
        for n in lens:
            keep = min(i + 1, n)
            assert torch.equal(o1[off:off + keep].view(torch.int16), o2[off:off + keep].view(torch.int16)), (i, off)
            if n > keep:
                assert not torch.equal(o1[off + keep:off + n].view(torch.int16), o2[off + keep:off + n].view(torch.int16))
            off += n
    alone = _launch(seqs, ctxs, H, KVH, D, sbs, dtype, pad_rows=3, only=1)
    a, b = lens[0], lens[0] + lens[1]
    assert torch.equal(alone[a:b].view(torch.int16), o1[a:b].view(torch.int16))
    assert torch.isnan(alone[:a].float()).all() and torch.isnan(alone[b:].float()).all()


# ---- 3. determinism --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_verify_attention_is_deterministic(dtype):
    """Twelve launches of one case with phase 2 (24 splits for the longest sequence): bit-equal."""
    H, KVH, D, sbs = 32, 8, 128, 64
    g = gen(3)
    ctxs, lens = [1499, 62, 17, 300], [4, 4, 2, 3]
    seqs = [_make_seq(c, n, H, KVH, D, sbs, dtype, g, i) for i, (c, n) in enumerate(zip(ctxs, lens))]
    outs = _launch(seqs, ctxs, H, KVH, D, sbs, dtype, repeat=12)
    assert torch.isfinite(outs[0].float()).all()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))


# ---- 3b. one new token per sequence is the decode step ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sbs,lengths", [(64, [1, 17, 100]), (512, [600])])
@pytest.mark.parametrize("H,KVH,D", [(4, 2, 64), (32, 8, 128), (16, 2, 32)])
def test_verify_of_one_token_is_the_decode_step_bit_for_bit(dtype, H, KVH, D, sbs, lengths):
    """n = 1, ctx = len - 1: swl_paged_attn_verify and swl_paged_attn_decode run the same attend_block_mfma with the same
    mask limit, the same ring, wave merge and phase 2 over the same finite pools, so their outputs are the same bits —
    with one split (lengths 1 and 17) and with two (100 at 64, 600 at 512). G >= 2 only: decode's G = 1 is the VALU path."""
    from swiftllm_amd.worker.kernels.paged_attn import paged_attention
    assert H // KVH >= 2
    g = gen(D + sbs)
    mc, ec = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=NUM_LAYERS), NS(block_size=16)
    for length in lengths:
        ctxs = [length - 1, length - 1]
        seqs = [_make_seq(c, 1, H, KVH, D, sbs, dtype, g, i) for i, c in enumerate(ctxs)]
        kc, vc, bt, seq_ids = _fill_pools(seqs, ctxs, KVH, D, dtype, 0.0, -(-length // 16) + 3)
        kc, vc, bt = kc.cuda(), vc.cuda(), bt.cuda()
        q = torch.cat([s[0] for s in seqs]).cuda()
        o_verify, o_decode = torch.full_like(q, float("nan")), torch.full_like(q, float("nan"))
        st = _state(ctxs, [1, 1], D, sbs, seq_ids)
        _verify()(q, kc, vc, bt, o_verify, mc, ec, st, LAYER)
        dec = NS(num_decoding_seqs=2, num_prefill_seqs=0, seq_block_size=sbs, num_seq_blocks=st.num_seq_blocks,
                 softmax_scale=st.softmax_scale, seq_ids=st.seq_ids, paged_attn_scratch=None,
                 decoding_seq_lens=torch.tensor([length, length], dtype=torch.int32).cuda())
        paged_attention(q, kc, vc, bt, mc, ec, dec, LAYER, o_decode)
        torch.cuda.synchronize()
        assert torch.isfinite(o_decode.float()).all(), length
        assert torch.equal(o_verify.view(torch.int16), o_decode.view(torch.int16)), length


# ---- 4. the model: logits against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["TINY", "SMALL128"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_forward_verify_logits_match_the_oracle_teacher_forced(tmp_path, shape, dtype):
    """Sequences of different lengths, verify steps with k = 0, 1, max and a mixed one; the oracle decodes the same
    tokens one at a time. Every row's logits inside the chunked-prefill budget |d| <= atol + rtol |logit|. Logits only:
    no id assertion, so nothing is left out. The K/V a verify step stores are what the next step attends to.
    Measured on MI355X, excess over rtol |logit| against atol: TINY 3.1e-4 / SMALL128 1.4e-3 of 2e-3 (float16),
    2.6e-3 / 1.0e-2 of 1.6e-2 (bfloat16)."""
    from swiftllm_amd import LlamaModelConfig
    cfg = synth.make_config(**getattr(synth, shape))
    tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
    sd = synth.make_state_dict(cfg, seed=5, dtype=tdtype)
    ecfg = dict(max_blocks_per_seq=32, max_tokens_in_batch=1024, dtype=dtype)
    model = _make_model(tmp_path, cfg, sd, 64, **ecfg)
    ref = RefLlamaModel(LlamaModelConfig(cfg), _engine_config("", **ecfg), sd, tdtype)
    ref.init_kvcache_and_swap(64)
    kmax = model.max_draft_tokens
    assert kmax == 16 // (cfg["num_attention_heads"] // cfg["num_key_value_heads"]) - 1
    g = gen(2)
    prompts = [torch.randint(0, cfg["vocab_size"], (n,), generator=g).tolist() for n in (5, 16, 17, 40)]
    ids = list(range(4))
    atol, rtol = (2e-3, 2e-3) if dtype == "float16" else (1.6e-2, 1.6e-2)
    last = model.forward(prompts, ids, [])
    ref.forward(prompts, ids, [])
    lens = [len(p) for p in prompts]            # tokens resident
    worst = 0.0
    for ks in ([0] * 4, [1] * 4, [kmax] * 4, [0, 1, kmax, kmax - 1], [kmax] * 4):
        inputs = [[last[i]] + torch.randint(0, cfg["vocab_size"], (k,), generator=g).tolist() for i, k in enumerate(ks)]
        del model.post_layer.logits_tap[:]
        out = model.forward_verify(inputs, ids, list(lens))
        ours = model.post_layer.logits_tap[-1].float().cpu()
        assert [len(o) for o in out] == [k + 1 for k in ks] and ours.shape[0] == sum(ks) + 4
        starts = [sum(k + 1 for k in ks[:i]) for i in range(4)]
        for j in range(max(ks) + 1):
            live = [i for i in ids if j <= ks[i]]
            ref.forward([[inputs[i][j]] for i in live], live, [lens[i] + j + 1 for i in live])
            theirs = ref.last_logits
            rows = ours[[starts[i] + j for i in live]]
            worst = max(worst, ((rows - theirs).abs() - rtol * theirs.abs()).max().item())
            assert [out[i][j] for i in live] == rows.argmax(-1).tolist()
        lens = [n + k + 1 for n, k in zip(lens, ks)]
        last = [o[-1] for o in out]
    print(f"\n[forward_verify {shape} {dtype}] logit excess over rtol|logit|: {worst:.2e} (atol {atol})")
    assert worst <= atol


def test_forward_verify_refuses_bad_calls_on_the_host(tmp_path):
    cfg = synth.make_config(**synth.TINY)
    model = _make_model(tmp_path, cfg, synth.make_state_dict(cfg, seed=5), 16)
    model.forward([[1] * 20], [0], [])
    free = model.gpu_block_manager.num_free_blocks
    with pytest.raises(ValueError, match="at most"):
        model.forward_verify([[1] * (model.max_draft_tokens + 2)], [0], [20])
    with pytest.raises(ValueError, match="empty"):
        model.forward_verify([[]], [0], [20])
    with pytest.raises(ValueError, match="allocated KV blocks"):
        model.forward_verify([[1, 2]], [0], [33])
    with pytest.raises(ValueError, match=">= 0"):
        model.forward_verify([[1, 2]], [0], [-1])
    with pytest.raises(ValueError, match="one sequence id"):
        model.forward_verify([[1, 2]], [0], [20, 20])
    assert model.gpu_block_manager.num_free_blocks == free
    assert model.forward_verify([], [], []) == []
    assert len(model.forward_verify([[3, 4]], [0], [20])[0]) == 2


# ---- 5. exact ids on the decisive checkpoint -------------------------------------------------------------------------
STEPS = 26


def _decisive_model(tmp_path, dtype, identity=False, prompts=None, steps=STEPS, **kw):
    """The geometry and prompts of test_gpu_chunked_prefill._decisive. `identity`: lm_head rows permuted so that the token
    after position p IS the token at p - OFFSET (a periodic stream prompt lookup predicts)."""
    cfg = synth.make_config(**DECISIVE)
    tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
    sd, perm, _ = synth.make_decisive_state_dict(cfg, seed=5, dtype=tdtype, offset=OFFSET, max_context=300)
    if identity:
        sd["lm_head.weight"] = sd["lm_head.weight"][perm]
        perm = torch.arange(cfg["vocab_size"])
    if prompts is None:
        g = gen(1)
        prompts = [torch.randint(0, cfg["vocab_size"], (60 + 7 * i,), generator=g).tolist() for i in range(4)]
    elif callable(prompts):
        prompts = prompts(cfg, perm)
    want = synth.decisive_expected_tokens(prompts, perm, OFFSET, steps)
    base = dict(max_seqs_in_block_table=8, max_blocks_per_seq=16, max_batch_size=4, max_tokens_in_batch=1024, dtype=dtype)
    base.update(kw)
    model = _make_model(tmp_path, cfg, sd, 40, **base)
    model.post_layer.logits_tap = None
    return model, prompts, want, cfg


def _stream(want, i):
    return [step[i] for step in want]


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_decisive_verify_steps_return_the_closed_form(tmp_path, dtype):
    """(a) the drafts ARE the closed form: every returned row equals it, six steps of four rows per sequence, contexts
    60 .. 101 (rows cross the 16-token boundaries at 64, 80 and 96 on the way)."""
    model, prompts, want, _ = _decisive_model(tmp_path, dtype)
    ids = list(range(4))
    assert model.max_draft_tokens == 3
    assert model.forward(prompts, ids, []) == want[0]
    crossed = 0
    for t in range(0, STEPS - 3, 4):
        ctx = [len(p) + t for p in prompts]
        crossed += sum(c // 16 != (c + 3) // 16 for c in ctx)
        out = model.forward_verify([[want[t + j][i] for j in range(4)] for i in ids], ids, ctx)
        assert out == [[want[t + 1 + j][i] for j in range(4)] for i in ids], t
    assert crossed >= 4


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_decisive_verify_step_across_a_block_boundary(tmp_path, dtype):
    """(c) one sequence, context 62: the rows sit at positions 62 .. 65, the step takes the sequence's fifth block."""
    model, prompts, want, _ = _decisive_model(tmp_path, dtype)
    p, s = prompts[0], _stream(want, 0)
    assert len(p) == 60
    assert model.forward([p], [0], []) == [s[0]]
    assert model.forward([[s[0]]], [0], [61]) == [s[1]]
    assert model.forward([[s[1]]], [0], [62]) == [s[2]]
    assert model.gpu_block_manager.host.num_allocated(0) == 4
    assert model.forward_verify([s[2:6]], [0], [62]) == [s[3:7]]
    assert model.gpu_block_manager.host.num_allocated(0) == 5


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_decisive_rejected_drafts_leave_nothing_behind(tmp_path, dtype):
    """(b) sequence i gets a wrong token at draft 1 + i % 3: accept() keeps exactly the drafts before it. Plain decode
    steps continue from the accepted point for 22 steps — past OFFSET = 19, so the copy head reads the slots the rejected
    drafts wrote (and the decode steps overwrote) — and every stream is the closed form."""
    from swiftllm_amd.server.speculative import accept
    model, prompts, want, cfg = _decisive_model(tmp_path, dtype)
    ids = list(range(4))
    streams = [[t] for t in model.forward(prompts, ids, [])]
    assert [s[0] for s in streams] == want[0]
    drafts = []
    for i in ids:
        d = [want[1 + j][i] for j in range(3)]
        d[i % 3] = (d[i % 3] + 1) % cfg["vocab_size"]
        drafts.append(d)
    out = model.forward_verify([[streams[i][0]] + drafts[i] for i in ids], ids, [len(p) for p in prompts])
    for i in ids:
        a = accept(drafts[i], out[i])
        assert a == i % 3
        assert out[i][:a + 1] == _stream(want, i)[1:a + 2]
        streams[i] += out[i][:a + 1]
    for _ in range(22):
        lens = [len(p) + len(s) for p, s in zip(prompts, streams)]
        nxt = model.forward([[s[-1]] for s in streams], ids, lens)
        for s, t in zip(streams, nxt):
            s.append(t)
    for i in ids:
        assert streams[i] == _stream(want, i)[:len(streams[i])], i
        assert len(streams[i]) >= 24
    model.free_seqs_resources(ids)
    assert model.gpu_block_manager.num_free_blocks == 40


# ---- 6. the engine ---------------------------------------------------------------------------------------------------
def _serve(model, prompts, output_len):
    from swiftllm_amd import Engine, RawRequest

    async def serve():
        eng = Engine(model.engine_config, model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        jobs = [asyncio.ensure_future(eng.add_request_and_wait(RawRequest("", output_len, p))) for p in prompts]
        done = await asyncio.wait_for(asyncio.gather(*jobs), timeout=300)
        loops.cancel()
        return eng, [(r.error, toks) for r, toks in done]
    return asyncio.run(serve())


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_engine_accepts_drafts_on_a_periodic_stream(tmp_path, dtype):
    """(i) the identity-permutation checkpoint: the stream repeats the prompt's tail, prompt lookup predicts it."""
    steps = 45
    model, prompts, want, _ = _decisive_model(tmp_path, dtype, identity=True, steps=steps, speculative_ngram=3)
    eng, got = _serve(model, prompts, steps + 1)
    for i, (err, toks) in enumerate(got):
        assert err is None and toks == _stream(want, i), i
    print(f"\n[engine, periodic stream, {dtype}] forwards {eng.num_forwards}, verify steps {eng.num_verify_steps}, "
          f"drafts accepted {eng.num_accepted_tokens} / {eng.num_draft_tokens}")
    assert eng.speculative_k == 3 and eng.num_verify_steps > 0
    assert eng.num_accepted_tokens > 0
    assert eng.num_forwards < steps + 1
    assert model.gpu_block_manager.num_free_blocks == 40


def _planted_prompts(cfg, perm):
    """Prompts of 60 .. 81 tokens whose first outputs t_s = perm[p[len - 20 + s]] appear in the prompt as the pairs
    (t_s, t_s+1), s = 0, 2, .., 10, at positions 3j, 3j + 1: a 1-gram match proposes the right next token, then junk."""
    g = gen(1)
    out = []
    for i in range(4):
        p = torch.randint(0, cfg["vocab_size"], (60 + 7 * i,), generator=g).tolist()
        n = len(p)
        for j, s in enumerate(range(0, 12, 2)):
            p[3 * j] = int(perm[p[n - 20 + s]])
            p[3 * j + 1] = int(perm[p[n - 20 + s + 1]])
        out.append(p)
    return out


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_engine_rejects_wrong_drafts_and_keeps_the_stream(tmp_path, dtype):
    """(ii) the random-permutation checkpoint with planted pairs: drafts are proposed, most are rejected, the streams are
    the closed form and every block returns to the pool."""
    steps = 29
    model, prompts, want, _ = _decisive_model(tmp_path, dtype, prompts=_planted_prompts, steps=steps,
                                              speculative_ngram=3)
    eng, got = _serve(model, prompts, steps + 1)
    for i, (err, toks) in enumerate(got):
        assert err is None and toks == _stream(want, i), i
    print(f"\n[engine, planted pairs, {dtype}] forwards {eng.num_forwards}, verify steps {eng.num_verify_steps}, "
          f"drafts accepted {eng.num_accepted_tokens} / {eng.num_draft_tokens}")
    assert eng.num_verify_steps > 0 and 0 < eng.num_accepted_tokens < eng.num_draft_tokens
    assert model.gpu_block_manager.num_free_blocks == 40
