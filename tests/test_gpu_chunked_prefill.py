"""Chunked prefill on the GPU: swl_prefill_attn_paged against fp64 on designed score profiles (contexts x chunk lengths,
scattered block ids, garbage in every slot the kernel must not read), causality, the c = 0 case against the fresh-K/V
kernel, the stores at an offset, and the whole path — model against the oracle on whole prompts, the decisive
checkpoint, one mixed step, the Engine with chunking on.

Bounds of the kernel tests are those tests/test_gpu_attention_extremes.py derives for prefill (same arithmetic):
general |o - o64| <= (3 u + 2 * 2^-22 log2(e) S) vmax, a 30-nat needle within 1 ulp of its v, a tie within 1.5 ulp.
The reference (tests/_attn_cases.py: attn64, unchanged) is evaluated in fp64 on the device: the largest case holds
1024 x 32 x 4024 scores. Measured fractions of the bounds are printed by every test; see the docstrings."""
import asyncio
import math
import types

import pytest
import torch

from _attn_cases import LOG2E, attn64, make_kv, make_q, scores64, ulp, unit_roundoff
from oracle import synth
from oracle.ref_model import RefLlamaModel
from test_gpu_attention_extremes import MARGIN, PREFILL_SPECS, _top2

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace
DTYPES = [torch.float16, torch.bfloat16]
CONTEXTS = [0, 1, 15, 16, 17, 63, 64, 65, 1000, 3000]
CHUNKS = [1, 63, 64, 65, 128, 200, 1024]
SHAPES = [(32, 8, 128), (8, 8, 128), (8, 2, 64), (10, 10, 32)]
NUM_LAYERS, LAYER = 2, 1


def gen(seed):
    return torch.Generator().manual_seed(seed)


def K():
    from swiftllm_amd.worker import kernels
    return kernels


def _paged_attn():
    from swiftllm_amd.worker.kernels.prefill_attn import prefill_attention_paged
    return prefill_attention_paged


# ---- building a launch -----------------------------------------------------------------------------------------------
def _needles(c, n, KVH, salt):
    """One needle per kv head: inside the context, inside the chunk, on both sides of the context boundary and of 16-
    and 64-key edges, first / last key; feature 1 is the sink (key 0)."""
    L = c + n
    cand = [c - 1, c, 0, L - 1, 15, 16, 63, 64, c // 2, c + n // 2, c - 16, c + 15, L - 2, 130, 700]
    pos = [cand[(h + salt) % len(cand)] for h in range(KVH)]
    return [[min(max(p, 0), L - 1) for p in pos], [0] * KVH]


def _make_seq(c, n, H, KVH, D, dtype, g, salt):
    L = c + n
    specs = [PREFILL_SPECS[h % len(PREFILL_SPECS)] for h in range(H)]
    ties = [[(min(5, L - 1), min(70 + 13 * h, L - 1)) if L > 70 else None for h in range(KVH)]]
    k_, v_, F = make_kv(L, KVH, D, dtype, g, needles=_needles(c, n, KVH, salt), ties=ties)
    q_ = make_q(n, H, D, F, dtype, g, specs, D ** -0.5)
    return q_, k_, v_


def _block_ids(total_blocks):
    """A permutation of the pool's blocks, scattered and mostly descending."""
    nb = total_blocks + 5
    while math.gcd(nb, 7) != 1:
        nb += 1
    return nb, [nb - 1 - (i * 7) % nb for i in range(nb)]


def _fill_pools(seqs, ctxs, KVH, D, dtype, fill, mbps):
    """seqs: [(q, K, V)] with K/V of all c + n keys. Pools [NB, L, KVH, 16, D] pre-filled with `fill` in EVERY slot of
    every layer; only keys < c + n of the sequences' own blocks are written. Table rows in reverse order, entries past a
    sequence's blocks point at a block nobody owns."""
    need = [-(-k.shape[0] // 16) for _, k, _ in seqs]
    nb, ids = _block_ids(sum(need))
    kc = torch.full((nb, NUM_LAYERS, KVH, 16, D), fill, dtype=dtype)
    vc = torch.full((nb, NUM_LAYERS, KVH, 16, D), fill, dtype=dtype)
    rows = len(seqs) + 2
    bt = torch.full((rows, mbps), ids[-1], dtype=torch.int32)
    seq_ids, off = [], 0
    for i, ((_, k_, v_), nblk) in enumerate(zip(seqs, need)):
        row = rows - 1 - i
        mine = torch.tensor(ids[off:off + nblk], dtype=torch.int64)
        off += nblk
        bt[row, :nblk] = mine.to(torch.int32)
        pos = torch.arange(k_.shape[0])
        kc[mine[pos // 16], LAYER, :, pos % 16] = k_
        vc[mine[pos // 16], LAYER, :, pos % 16] = v_
        seq_ids.append(row)
    return kc, vc, bt, torch.tensor(seq_ids, dtype=torch.int32)


def _state(ctxs, lens, D, seq_ids):
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0)
    return NS(num_prefill_seqs=len(lens), max_prefill_len=max(lens), softmax_scale=D ** -0.5,
              prefill_seq_start_locs_with_end=cu.cuda(), prefill_seq_start_locs=cu[:-1].cuda(),
              prefill_seq_lens=torch.tensor(lens, dtype=torch.int32).cuda(), num_prefill_tokens=sum(lens),
              prefill_ctx_lens=torch.tensor(ctxs, dtype=torch.int32).cuda(),
              max_prefill_total_len=max(c + n for c, n in zip(ctxs, lens)), seq_ids=seq_ids.cuda(),
              num_decoding_seqs=0, decoding_seq_lens=torch.zeros(0, dtype=torch.int32).cuda(), ignore_kvcache=False)


def _launch(seqs, ctxs, H, KVH, D, dtype, fill=0.0):
    lens = [q.shape[0] for q, _, _ in seqs]
    mbps = max(-(-(c + n) // 16) for c, n in zip(ctxs, lens)) + 3
    kc, vc, bt, seq_ids = _fill_pools(seqs, ctxs, KVH, D, dtype, fill, mbps)
    q = torch.cat([s[0] for s in seqs]).cuda()
    o = torch.full_like(q, float("nan"))
    mc = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=NUM_LAYERS)
    _paged_attn()(q, kc.cuda(), vc.cuda(), bt.cuda(), o, mc, NS(block_size=16), _state(ctxs, lens, D, seq_ids), LAYER)
    torch.cuda.synchronize()
    return o


def _reference(q_, k_, v_, D):
    """attn64 and the masked fp64 scores, on the device."""
    n, L = q_.shape[0], k_.shape[0]
    with torch.device("cuda"):
        qd, kd, vd = q_.cuda(), k_.cuda(), v_.cuda()
        ref = attn64(qd, kd, vd, D ** -0.5, causal=True)
        s = scores64(qd, kd, D ** -0.5)
        vis = torch.arange(L)[None, :] <= torch.arange(n)[:, None] + (L - n)
        s = s.masked_fill(~vis[:, None, :], float("-inf"))
    return ref, s, vd


def _check(o, ref, s, V, dtype, what):
    """o [T, H, D] from the kernel, everything on the device. Returns the measured fractions (general, needle, tie)."""
    T, H, D = o.shape
    G = H // V.shape[1]
    assert torch.isfinite(o.float()).all(), f"{what}: non-finite output"
    u = unit_roundoff(dtype)
    Vr = V.double().repeat_interleave(G, dim=1)                     # [n, H, D]
    vm = Vr.abs().amax(-1).t()                                      # [H, n]
    vmax = (vm[None] * torch.isfinite(s)).amax(-1)                  # [T, H]: the largest |v| the row can see
    bound = (3 * u + 2 * 2.0 ** -22 * LOG2E * ref["smag"]) * vmax
    err = (o.double() - ref["o"]).abs().amax(-1)
    frac = (err / bound).max().item()
    assert (err <= bound).all(), f"{what}: |o - o64| {err.max().item():.3e} > bound (worst {frac:.2f} of it)"
    top, lead, second, lead3 = _top2(s)
    hh = torch.arange(H, device=o.device)[None, :].expand(T, H)
    nfrac = tfrac = 0.0
    sel = lead >= MARGIN
    if sel.any():
        want = Vr[top[sel], hh[sel]].to(dtype)
        d = (o[sel].double() - want.double()).abs() / ulp(want, dtype)
        nfrac = d.max().item()
        assert nfrac <= 1, f"{what}: a needle row is {nfrac} ulp from its key's v"
    sel = (lead == 0) & (lead3 >= MARGIN)
    if sel.any():
        a, b, h = top[sel], second[sel], hh[sel]
        want = (Vr[a, h] + Vr[b, h]) / 2
        # (v_a + v_b) / 2 is the output only up to what the OTHER keys add: o = want (1 - sum_j p_j) + sum_j p_j v_j over
        # the keys j outside the tie, each p_j <= e^-30. That is ~1e-10 vmax, far below an ulp of `want` — except where
        # v_a = -v_b cancels to (near) zero, which 16-bit values do exactly now and then: the spacing there is the
        # subnormal one and "1.5 ulp of want" alone would hold the kernel to 1e-40 on a quantity of 1e-17 that it computes
        # from P rounded to 8 or 11 bits. The size of that remainder, t = sum_j p_j (|v_j| + |want|) from the fp64
        # softmax of the reference (never from the kernel's output), is granted on top, twice: once because it is in
        # the exact answer, once because the kernel may get each of its terms wrong by less than its own size (the
        # rounding of P and the fp32 score error are relative errors far below 1).
        slack = torch.zeros_like(want)
        rows_t, rows_h = sel.nonzero(as_tuple=True)
        for head in rows_h.unique().tolist():
            m = rows_h == head
            pr = torch.softmax(s[rows_t[m], head], dim=-1)                       # [R, n] fp64, masked keys exactly 0
            pr = pr.scatter(1, a[m][:, None], 0.0).scatter(1, b[m][:, None], 0.0)
            slack[m] = pr @ Vr[:, head].abs() + pr.sum(-1, keepdim=True) * want[m].abs()
        d = ((o[sel].double() - want).abs() - 2 * slack).clamp(min=0) / ulp(want, dtype)
        tfrac = d.max().item() / 1.5
        assert tfrac <= 1, f"{what}: a tie row is {d.max().item()} ulp from (v_a + v_b) / 2"
    return frac, nfrac, tfrac


# ---- the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D", SHAPES)
def test_paged_prefill_attention_extreme_scores_and_garbage(dtype, H, KVH, D):
    """Every context x every chunk length (one launch per chunk length: ten sequences), cur_layer 1 of 2, block ids
    scattered and descending, table rows reversed. Three passes over the same inputs: every slot the kernel must not
    read (slots past c + n, blocks outside the tables, the other layer) holds 0, then NaN, then +Inf — the outputs must
    be finite and inside the same bounds each time.
    Measured on MI355X (the same in all three passes): the general bound at <= 0.33 of it, the needles at 0 ulp
    (bound 1), the ties at <= 0.34 of their bound."""
    g = gen(H * 11 + D + (dtype == torch.bfloat16))
    worst = {}
    for n in CHUNKS:
        ctxs = [c for c in CONTEXTS if c + n <= 4096]
        assert len(ctxs) == len(CONTEXTS)
        seqs = [_make_seq(c, n, H, KVH, D, dtype, g, i) for i, c in enumerate(ctxs)]
        refs = [_reference(*sq, D) for sq in seqs]
        for name, fill in (("zero", 0.0), ("nan", float("nan")), ("inf", float("inf"))):
            o = _launch(seqs, ctxs, H, KVH, D, dtype, fill)
            off = 0
            w = worst.setdefault(name, [0.0, 0.0, 0.0])
            for c, (ref, s, vd) in zip(ctxs, refs):
                fr = _check(o[off:off + n], ref, s, vd, dtype, f"paged prefill c={c} n={n} fill={name}")
                worst[name] = w = [max(a, b) for a, b in zip(w, fr)]
                off += n
        del refs
    for name, w in worst.items():
        print(f"\n[paged prefill extremes {dtype} {H}/{KVH}/{D} fill={name}] bound fractions: general {w[0]:.3f} "
              f"needle {w[1]:.3f} tie {w[2]:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D", [(8, 2, 128), (4, 2, 64), (4, 4, 32)])
def test_paged_prefill_rows_do_not_depend_on_later_keys(dtype, H, KVH, D):
    """Causality, bit for bit: new K/V at every position > c + i leaves rows <= i as they were."""
    g = gen(5)
    c, n, i = 100, 200, 77
    q_, k_, v_ = _make_seq(c, n, H, KVH, D, dtype, g, 0)
    o1 = _launch([(q_, k_, v_)], [c], H, KVH, D, dtype)
    k2, v2 = k_.clone(), v_.clone()
    k2[c + i + 1:] = (torch.randn(n - i - 1, KVH, D, generator=g) * 3).to(dtype)
    v2[c + i + 1:] = (torch.randn(n - i - 1, KVH, D, generator=g) * 3).to(dtype)
    o2 = _launch([(q_, k2, v2)], [c], H, KVH, D, dtype)
    assert torch.equal(o1[:i + 1].view(torch.int16), o2[:i + 1].view(torch.int16))
    assert not torch.equal(o1[i + 1:].view(torch.int16), o2[i + 1:].view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D", SHAPES)
def test_paged_prefill_without_context_against_the_fresh_kv_kernel(dtype, H, KVH, D):
    """c = 0 is a plain causal prefill: the paged kernel and swl_prefill_attn_varlen on the same data are each inside
    the general bound against fp64 (measured on MI355X: both at <= 0.29 of it). With c = 0 the 64-key tiles start
    where the fresh-K/V kernels' tiles start and a row's arithmetic depends on its own scores only, so the outputs are
    also bit-identical — at D = 128 too, where the fresh-K/V kernel pairs heads per workgroup: asserted."""
    g = gen(H + D)
    lens = [1, 17, 64, 129, 700]
    seqs = [_make_seq(0, n, H, KVH, D, dtype, g, i) for i, n in enumerate(lens)]
    o = _launch(seqs, [0] * len(lens), H, KVH, D, dtype)
    q = torch.cat([s[0] for s in seqs]).cuda()
    k = torch.cat([s[1] for s in seqs]).cuda()
    v = torch.cat([s[2] for s in seqs]).cuda()
    o_fresh = torch.full_like(q, float("nan"))
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0)
    st = NS(num_prefill_seqs=len(lens), max_prefill_len=max(lens), softmax_scale=D ** -0.5,
            prefill_seq_start_locs_with_end=cu.cuda(), num_prefill_tokens=sum(lens))
    K().prefill_attention(q, k, v, o_fresh, NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D), None, st)
    torch.cuda.synchronize()
    off, worst = 0, [0.0, 0.0]
    for (q_, k_, v_), n in zip(seqs, lens):
        ref, s, vd = _reference(q_, k_, v_, D)
        worst[0] = max(worst[0], _check(o[off:off + n], ref, s, vd, dtype, f"paged c=0 n={n}")[0])
        worst[1] = max(worst[1], _check(o_fresh[off:off + n], ref, s, vd, dtype, f"fresh n={n}")[0])
        off += n
    same = torch.equal(o.view(torch.int16), o_fresh.view(torch.int16))
    print(f"\n[paged vs fresh, c = 0, {dtype} {H}/{KVH}/{D}] general bound fractions: paged {worst[0]:.3f} fresh "
          f"{worst[1]:.3f}; bit-identical: {same}")
    assert same


# ---- stores at an offset ---------------------------------------------------------------------------------------------
def _store_state(ctxs, lens, seq_ids, D, rope_rows, dtype, g):
    st = _state(ctxs, lens, D, torch.tensor(seq_ids, dtype=torch.int32))
    pos = torch.cat([c + torch.arange(n) for c, n in zip(ctxs, lens)]).to(torch.int32)
    ang = torch.rand(rope_rows, D // 2, generator=g) * 6.28
    st.position_cos, st.position_sin = torch.cos(ang).to(dtype).cuda(), torch.sin(ang).to(dtype).cuda()
    st.position_indices = pos.cuda()
    return st


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D", [(8, 2, 128), (4, 2, 64), (4, 4, 32)])
def test_store_at_an_offset_is_bit_exact_and_touches_nothing_else(dtype, H, KVH, D):
    g = gen(D)
    ctxs, lens = [0, 5, 16, 27, 33, 15], [1, 11, 16, 40, 3, 2]      # chunks that start and end inside blocks
    seq_ids = [4, 0, 6, 2, 1, 5]
    mbps, nb = 8, 40
    bt = torch.full((8, mbps), nb - 1, dtype=torch.int32)
    ids = _block_ids(30)[1]
    off = 0
    for sid, c, n in zip(seq_ids, ctxs, lens):
        need = -(-(c + n) // 16)
        bt[sid, :need] = torch.tensor(ids[off:off + need], dtype=torch.int32)
        off += need
    P = sum(lens)
    k = torch.randn(P, KVH, D, generator=g).to(dtype)
    v = torch.randn(P, KVH, D, generator=g).to(dtype)
    q = torch.randn(P, H, D, generator=g).to(dtype)
    sentinel = 7.0
    shape = (nb, NUM_LAYERS, KVH, 16, D)
    mc, ec = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=NUM_LAYERS), NS(block_size=16)
    st = _store_state(ctxs, lens, seq_ids, D, 128, dtype, g)

    def expected(kk, vv):
        ek, ev = torch.full(shape, sentinel, dtype=dtype), torch.full(shape, sentinel, dtype=dtype)
        t0 = 0
        for sid, c, n in zip(seq_ids, ctxs, lens):
            pos = c + torch.arange(n)
            blk = bt[sid].long()[pos // 16]
            ek[blk, LAYER, :, pos % 16] = kk[t0:t0 + n]
            ev[blk, LAYER, :, pos % 16] = vv[t0:t0 + n]
            t0 += n
        return ek, ev

    def bits(t):
        return t.cpu().view(torch.int16)
    # plain store
    kc, vc = torch.full(shape, sentinel, dtype=dtype).cuda(), torch.full(shape, sentinel, dtype=dtype).cuda()
    K().store_kvcache(k.cuda(), v.cuda(), kc, vc, bt.cuda(), mc, ec, st, LAYER)
    ek, ev = expected(k, v)
    assert torch.equal(bits(kc), bits(ek)) and torch.equal(bits(vc), bits(ev))     # the sentinels included
    # rotary + store in one pass == rotary, then the plain store at the offset
    q1, k1 = q.clone().cuda(), k.clone().cuda()
    K().rotary_embedding_inplace(q1, k1, st)
    kc1, vc1 = torch.full(shape, sentinel, dtype=dtype).cuda(), torch.full(shape, sentinel, dtype=dtype).cuda()
    K().store_kvcache(k1, v.cuda(), kc1, vc1, bt.cuda(), mc, ec, st, LAYER)
    from swiftllm_amd.worker.kernels.rotary_emb import rotary_embedding_and_store_kvcache_prefill as fused
    q2, k2 = q.clone().cuda(), k.clone().cuda()
    kc2, vc2 = torch.full(shape, sentinel, dtype=dtype).cuda(), torch.full(shape, sentinel, dtype=dtype).cuda()
    fused(q2, k2, v.cuda(), kc2, vc2, bt.cuda(), mc, ec, st, LAYER)
    assert torch.equal(bits(q1), bits(q2)) and torch.equal(bits(k1), bits(k2))
    assert torch.equal(bits(kc1), bits(kc2)) and torch.equal(bits(vc1), bits(vc2))
    ek, ev = expected(k1.cpu(), v)
    assert torch.equal(bits(kc2), bits(ek)) and torch.equal(bits(vc2), bits(ev))
    # all contexts zero: the bits of the existing entries
    zero = _store_state([0] * len(lens), lens, seq_ids, D, 128, dtype, g)
    plain = _store_state([0] * len(lens), lens, seq_ids, D, 128, dtype, g)
    plain.position_cos, plain.position_sin = zero.position_cos, zero.position_sin
    plain.prefill_ctx_lens = None
    pools = []
    for s_ in (zero, plain):
        ka, va = torch.full(shape, sentinel, dtype=dtype).cuda(), torch.full(shape, sentinel, dtype=dtype).cuda()
        K().store_kvcache(k.cuda(), v.cuda(), ka, va, bt.cuda(), mc, ec, s_, LAYER)
        qb, kb = q.clone().cuda(), k.clone().cuda()
        kb_, vb_ = torch.full(shape, sentinel, dtype=dtype).cuda(), torch.full(shape, sentinel, dtype=dtype).cuda()
        fused(qb, kb, v.cuda(), kb_, vb_, bt.cuda(), mc, ec, s_, LAYER)
        pools.append([bits(t) for t in (ka, va, kb_, vb_, qb, kb)])
    assert all(torch.equal(a, b) for a, b in zip(*pools))


# ---- the model -------------------------------------------------------------------------------------------------------
def _engine_config(path, **kw):
    from swiftllm_amd import EngineConfig
    base = dict(model_path=path, use_dummy=False, block_size=16, gpu_mem_utilization=0.9,
                num_cpu_blocks=8, max_seqs_in_block_table=16, max_blocks_per_seq=32, max_batch_size=8,
                max_tokens_in_batch=256)
    base.update(kw)
    return EngineConfig(**base)


def _make_model(tmp_path, cfg, sd, num_blocks=24, **kw):
    from swiftllm_amd import LlamaModel
    synth.write_model_dir(str(tmp_path), cfg, sd)
    model = LlamaModel(_engine_config(str(tmp_path), **kw))
    model.load_weights()
    model.init_kvcache_and_swap(num_blocks)
    model.post_layer.logits_tap = []
    return model


def _chunked_prefill(model, prompts, seq_ids, chunk):
    """Feed the prompts `chunk` tokens at a time (None: whole), all unfinished sequences in every step. Returns the
    token after each prompt and (if the model taps them) the logits of each sequence's last chunk."""
    done = [0] * len(prompts)
    toks, logits = [None] * len(prompts), [None] * len(prompts)
    while any(d < len(p) for d, p in zip(done, prompts)):
        idx = [i for i, p in enumerate(prompts) if done[i] < len(p)]
        take = [len(prompts[i]) - done[i] if chunk is None else min(chunk, len(prompts[i]) - done[i]) for i in idx]
        out = model.forward([prompts[i][done[i]:done[i] + t] for i, t in zip(idx, take)], [seq_ids[i] for i in idx], [],
                            prefill_ctx_lens=[done[i] for i in idx])
        tap = model.post_layer.logits_tap
        for row, (i, t) in enumerate(zip(idx, take)):
            done[i] += t
            if done[i] == len(prompts[i]):
                toks[i] = out[row]
                if tap:
                    logits[i] = tap[-1][row].float().cpu()
    return toks, logits


@pytest.mark.parametrize("shape", ["TINY", "SMALL64", "SMALL128"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_chunked_forward_matches_oracle_on_whole_prompts(tmp_path, shape, dtype):
    """The inputs of test_gpu_model.py::test_forward_matches_oracle_model, the prompts fed in chunks of 1, 7, 16, 64 and
    whole (sequences finish at different steps: steps mix first, middle and last chunks), then 8 decode steps
    teacher-forced with our tokens. Logits against the oracle run on the WHOLE prompts, |d| <= atol + rtol |logit|;
    ids equal the oracle's wherever its top-2 gap exceeds 2 (atol + rtol |top|); positions left out are capped at 20 %
    (float16) / 55 % (bfloat16) of the 45."""
    cfg = synth.make_config(**getattr(synth, shape))
    tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
    sd = synth.make_state_dict(cfg, seed=5, dtype=tdtype)
    from swiftllm_amd import LlamaModelConfig
    ecfg = dict(max_blocks_per_seq=32, max_tokens_in_batch=1024, dtype=dtype)
    model = _make_model(tmp_path, cfg, sd, 64, **ecfg)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, cfg["vocab_size"], (n,), generator=g).tolist() for n in (1, 16, 17, 130, 65)]
    atol, rtol = (2e-3, 2e-3) if dtype == "float16" else (1.6e-2, 1.6e-2)
    cap = 0.20 if dtype == "float16" else 0.55
    ids5 = list(range(5))
    for chunk in (1, 7, 16, 64, None):
        ref = RefLlamaModel(LlamaModelConfig(cfg), _engine_config("", **ecfg), sd, tdtype)
        ref.init_kvcache_and_swap(64)
        worst, left_out, positions = 0.0, 0, 0

        def hold(ours, ours_ids, theirs_ids):
            nonlocal worst, left_out, positions
            theirs = ref.last_logits
            worst = max(worst, ((ours - theirs).abs() - rtol * theirs.abs()).max().item())
            top2 = theirs.topk(2).values
            decided = (top2[:, 0] - top2[:, 1]) > 2 * (atol + rtol * top2[:, 0].abs())
            for i in range(len(ours_ids)):
                positions += 1
                if decided[i]:
                    assert ours_ids[i] == theirs_ids[i], (chunk, i, ours_ids[i], theirs_ids[i])
                else:
                    left_out += 1
        toks, logits = _chunked_prefill(model, prompts, ids5, chunk)
        want = ref.forward(prompts, ids5, [])
        hold(torch.stack(logits), toks, want)
        lens = [len(p) for p in prompts]
        for _ in range(8):
            lens = [n + 1 for n in lens]
            nxt = model.forward([[t] for t in toks], ids5, list(lens))
            want = ref.forward([[t] for t in toks], ids5, list(lens))     # teacher-forced with OUR tokens
            hold(model.post_layer.logits_tap[-1].float().cpu(), nxt, want)
            toks = nxt
        print(f"\n[chunked forward {shape} {dtype} chunk={chunk}] logit excess over rtol|logit|: {worst:.2e} (atol {atol}); "
              f"positions left out {left_out} / {positions}")
        assert worst <= atol, (chunk, worst)
        assert positions == 45 and left_out <= cap * positions, (chunk, left_out)
        model.free_seqs_resources(ids5)
        del model.post_layer.logits_tap[:]


def test_forward_refuses_bad_contexts_on_the_host(tmp_path):
    cfg = synth.make_config(**synth.TINY)
    model = _make_model(tmp_path, cfg, synth.make_state_dict(cfg, seed=5), 16)
    with pytest.raises(ValueError, match="ignore_kvcache"):
        model.forward([[1, 2]], [0], [], ignore_kvcache=True, prefill_ctx_lens=[4])
    with pytest.raises(ValueError, match=">= 0"):
        model.forward([[1, 2]], [0], [], prefill_ctx_lens=[-1])
    with pytest.raises(ValueError, match="one entry"):
        model.forward([[1, 2]], [0], [], prefill_ctx_lens=[0, 0])
    with pytest.raises(ValueError, match="allocated KV blocks"):
        model.forward([[1, 2]], [0], [], prefill_ctx_lens=[4])              # nothing resident yet
    model.forward([[1] * 20], [0], [])                                       # 2 blocks = 32 slots
    with pytest.raises(ValueError, match="allocated KV blocks"):
        model.forward([[1, 2]], [0], [], prefill_ctx_lens=[33])
    with pytest.raises(RuntimeError, match="rotary table"):
        model.forward([[1] * 700], [0], [], prefill_ctx_lens=[20])
    assert model.gpu_block_manager.num_free_blocks == 14                     # nothing was allocated by the refusals
    assert len(model.forward([[3, 4]], [0], [], prefill_ctx_lens=[20])) == 1


DECISIVE = dict(num_hidden_layers=3, hidden_size=1024, num_attention_heads=16, num_key_value_heads=4,
                intermediate_size=2048, vocab_size=2048, max_position_embeddings=2048, rope_theta=500000.0)
OFFSET, STEPS = 19, 26


def _decisive(tmp_path, dtype, num_blocks=40, **kw):
    cfg = synth.make_config(**DECISIVE)
    tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
    sd, perm, _ = synth.make_decisive_state_dict(cfg, seed=5, dtype=tdtype, offset=OFFSET, max_context=300)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg["vocab_size"], (60 + 7 * i,), generator=g).tolist() for i in range(4)]
    want = synth.decisive_expected_tokens(prompts, perm, OFFSET, STEPS)
    base = dict(max_seqs_in_block_table=8, max_blocks_per_seq=16, max_batch_size=4, max_tokens_in_batch=1024, dtype=dtype)
    base.update(kw)
    model = _make_model(tmp_path, cfg, sd, num_blocks, **base)
    model.post_layer.logits_tap = None
    return model, prompts, want


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("chunk", [16, 50])
def test_decisive_checkpoint_chunked_prefill_walks_the_closed_form(tmp_path, dtype, chunk):
    """Top-2 gap ~0.2 (400 float16 / 50 bfloat16 ulps): exact ids at every position, nothing left out."""
    model, prompts, want = _decisive(tmp_path, dtype)
    ids = list(range(4))
    toks, _ = _chunked_prefill(model, prompts, ids, chunk)
    got, lens = [toks], [len(p) for p in prompts]
    for _ in range(STEPS):
        lens = [n + 1 for n in lens]
        got.append(model.forward([[t] for t in got[-1]], ids, list(lens)))
    assert got == want


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_one_mixed_step_equals_the_same_work_in_separate_forwards(tmp_path, dtype):
    """The second chunk of A, the first chunk of B and two decodes in ONE forward against four separate forwards on
    other block-table rows: logits within the oracle test's budget, same tokens on this decisive checkpoint."""
    model, prompts, _ = _decisive(tmp_path, dtype, num_blocks=64, max_batch_size=8)
    model.post_layer.logits_tap = []
    a, b, c, d = prompts
    atol, rtol = (2e-3, 2e-3) if dtype == "float16" else (1.6e-2, 1.6e-2)

    def prepare(base):
        model.forward([a[:25]], [base], [])
        tc, td = model.forward([c, d], [base + 2, base + 3], [])
        return tc, td
    tc, td = prepare(0)
    mixed = model.forward([a[25:], b[:40], [tc], [td]], [0, 1, 2, 3], [len(c) + 1, len(d) + 1], prefill_ctx_lens=[25, 0])
    mixed_logits = model.post_layer.logits_tap[-1].float().cpu()
    tc2, td2 = prepare(4)
    assert (tc2, td2) == (tc, td)
    sep, sep_logits = [], []
    for args, kw in ((([a[25:]], [4], []), dict(prefill_ctx_lens=[25])), (([b[:40]], [5], []), {}),
                     (([[tc]], [6], [len(c) + 1]), {}), (([[td]], [7], [len(d) + 1]), {})):
        sep += model.forward(*args, **kw)
        sep_logits.append(model.post_layer.logits_tap[-1].float().cpu())
    sep_logits = torch.cat(sep_logits)
    excess = ((mixed_logits - sep_logits).abs() - rtol * sep_logits.abs()).max().item()
    print(f"\n[mixed step {dtype}] logit excess over rtol|logit|: {excess:.2e} (atol {atol})")
    assert excess <= atol
    assert mixed == sep


# ---- the engine ------------------------------------------------------------------------------------------------------
def _per_sequence(want, i):
    return [step[i] for step in want]


@pytest.mark.parametrize("piggyback", [True, False])
def test_engine_with_chunked_prefill_gives_the_closed_form(tmp_path, piggyback):
    """max_prefill_chunk 32 under max_tokens_in_batch 64: three of the four prompts (60, 67, 74, 81 tokens) are longer
    than a batch may be and are served; no forward carries more than 32 prompt tokens or 64 tokens."""
    from swiftllm_amd import Engine, RawRequest
    model, prompts, want = _decisive(tmp_path, "bfloat16", max_tokens_in_batch=64, max_prefill_chunk=32)
    seen = []
    inner = model.forward

    def spy(input_ids, seq_ids, dec_lens, **kw):
        n_prefill = len(input_ids) - len(dec_lens)
        seen.append((sum(len(x) for x in input_ids[:n_prefill]), len(dec_lens), kw.get("prefill_ctx_lens")))
        return inner(input_ids, seq_ids, dec_lens, **kw)
    model.forward = spy

    async def serve():
        eng = Engine(model.engine_config, model=model, piggyback=piggyback)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        jobs = [asyncio.ensure_future(eng.add_request_and_wait(RawRequest("", STEPS + 1, p))) for p in prompts]
        done = await asyncio.wait_for(asyncio.gather(*jobs), timeout=300)
        loops.cancel()
        return [(r.error, toks) for r, toks in done]
    got = asyncio.run(serve())
    for i, (err, toks) in enumerate(got):
        assert err is None and toks == _per_sequence(want, i), i
    assert all(p <= 32 and p + d <= 64 for p, d, _ in seen)
    assert any(ctx and any(ctx) for _, _, ctx in seen)                   # chunks behind a resident context happened
    assert any(p and d for p, d, _ in seen) == piggyback                 # decodes rode along with chunks (or never)
    assert model.gpu_block_manager.num_free_blocks == 40


def test_engine_swaps_a_partly_prefilled_request_and_still_gives_the_closed_form(tmp_path):
    """Pool of 10 blocks = request A (60 tokens, 4 blocks until it holds 65) + request D (81 tokens, 6 blocks). D arrives
    when A holds 63 tokens; A rides with D's first two chunks and outgrows the pool: D is swapped out with 64 of its 81
    prompt tokens resident, waits for A to finish, swaps in and continues at 64."""
    from swiftllm_amd import Engine
    from swiftllm_amd.server import RawRequest, Request
    model, prompts, want = _decisive(tmp_path, "float16", num_blocks=10, max_prefill_chunk=32)
    swapped = []

    async def run():
        eng = Engine(model.engine_config, model=model, piggyback=True)
        await eng.initialize()
        a, d = Request(RawRequest("", STEPS + 1, prompts[0])), Request(RawRequest("", STEPS + 1, prompts[3]))
        out = model.swap_out_seqs

        def spy(ids):
            swapped.append((list(ids), d.request_id, d.num_prefilled))
            return out(ids)
        model.swap_out_seqs = spy
        eng.scheduler.on_requests_arrival([a])
        while a.num_tokens() < 63:
            assert await eng.step()
        eng.scheduler.on_requests_arrival([d])
        for _ in range(200):
            if a.is_finished() and d.is_finished():
                break
            assert await eng.step()
        return eng, a, d
    eng, a, d = asyncio.run(run())
    assert a.output_token_ids == _per_sequence(want, 0) and d.output_token_ids == _per_sequence(want, 3)
    assert eng.num_swapped_out == 1 and eng.num_swapped_in == 1
    assert swapped == [([d.request_id], d.request_id, 64)]               # hit with 64 of 81 prompt tokens resident
    assert model.gpu_block_manager.num_free_blocks == 10
