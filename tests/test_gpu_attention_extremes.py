"""Every shipped attention entry point against an fp64 softmax on peaked and extreme scores (tests/_attn_cases.py).

The rest of the suite draws q and K from torch.randn: scores ~N(0, 1) nats, a nearly flat softmax whose running
maximum settles on the first tile. Here heads of one launch (and of one matrix-core wave) carry sinks, needles at
block / split / wave / tile boundaries, rising ramps (the maximum moves on every tile; prefill's masked future keys
hold the largest scores), falling ramps (whole blocks, waves and splits underflow), exact ties, flat rows and rows
shifted by +-600 nats.

Checks. The first assertion of every test: no non-finite output. Then, with u the unit roundoff of the storage dtype
(2^-11 float16, 2^-8 bfloat16) and vmax the largest |v| the row can see:
  * a row whose top key beats every other visible key by >= 30 nats gets that key's v. The other keys weigh
    < n e^-30 < 2^-31 together (n <= 4096). Paged decode: P is fp32 (or a hi + lo pair of storage-dtype halves,
    2^-16 relative or better), the accumulators are fp32 and the output is rounded once, so
    o = v (1 + O(2^-16)) rounds to v itself: EXACT bits. Prefill rounds P to the storage dtype before the PV product
    while the row sum stays fp32 (up to 2^kLazyMax = 16 because of the lazy maximum), so o = v (1 + d), |d| <= u
    < 1 ulp(v), before the output rounding: within 1 ulp of v.
  * an exact tie (two bit-identical K rows on top by >= 30 nats): (v_a + v_b) / 2. Paged: one rounding, <= 1 ulp.
    Prefill: the same relative error u before that rounding, <= 1.5 ulp.
  * everything else: |o - o64| <= c u vmax + 2 * 2^-22 log2(e) S vmax. The first term is the output rounding (paged,
    c = 2: the rounding plus fp32 accumulation over <= 4096 keys) or that plus the rounding of P (prefill, c = 3);
    the second is the fp32 error of scores of magnitude S = scale * max sum_d |q_d k_d| over the keys within 30 nats
    of the row maximum (each p relative ~2^-22 S log2 e; numerator and denominator: twice). The measured maximum of
    every bound, as a fraction of it, is noted beside it (MI355X).
The existing 2e-3 / 1.6e-2 bars of tests/test_gpu_kernels.py stay as they are; these are additional.
"""
import types

import pytest
import torch

from _attn_cases import LOG2E, attn64, make_kv, make_q, scores64, ulp, unit_roundoff

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace
DTYPES = [torch.float16, torch.bfloat16]
MARGIN = 30.0               # nats: a top key this far ahead owns the output


def gen(seed):
    return torch.Generator().manual_seed(seed)


def K():
    from swiftllm_amd.worker import kernels
    return kernels


def _top2(s):
    """Per row of nats [..., n] (masked = -inf): index of the maximum, its lead over the runner-up, the runner-up's
    index, and the lead of the maximum over the third key."""
    v, i = torch.topk(s, min(3, s.shape[-1]), dim=-1)
    lead = v[..., 0] - (v[..., 1] if v.shape[-1] > 1 else torch.full_like(v[..., 0], float("-inf")))
    third = v[..., 2] if v.shape[-1] > 2 else torch.full_like(v[..., 0], float("-inf"))
    return i[..., 0], lead, (i[..., 1] if v.shape[-1] > 1 else i[..., 0]), v[..., 0] - third


def _check_rows(o, ref, s, Kt, V, dtype, c_round, needle_exact, tie_ulps, what):
    """o [T, H, D] (storage dtype, from the kernel), ref = attn64(...), s = masked fp64 scores [T, H, n]. Returns the
    largest measured fraction of each bound: (general, needle, tie)."""
    T, H, D = o.shape
    G = H // Kt.shape[1]
    assert torch.isfinite(o.float()).all(), f"{what}: non-finite output"
    u = unit_roundoff(dtype)
    Vr = V.double().repeat_interleave(G, dim=1)                     # [n, H, D]
    vm = Vr.abs().amax(-1).t()                                      # [H, n]
    vmax = torch.where(torch.isfinite(s), vm[None], torch.zeros(())).amax(-1)          # [T, H]
    bound = (c_round * u + 2 * 2.0 ** -22 * LOG2E * ref["smag"]) * vmax
    err = (o.double() - ref["o"]).abs().amax(-1)
    frac = (err / bound).max().item()
    assert (err <= bound).all(), f"{what}: |o - o64| {err.max().item():.3e} > bound (worst {frac:.2f} of it)"
    top, lead, second, lead3 = _top2(s)
    hh = torch.arange(H)[None, :].expand(T, H)
    nfrac = tfrac = 0.0
    # needles: one key ahead of every other visible key by >= MARGIN
    sel = lead >= MARGIN
    if sel.any():
        want = Vr[top[sel], hh[sel]].to(dtype)                       # [rows, D]
        got = o[sel]
        if needle_exact:
            bad = (got != want).any(-1)
            assert not bad.any(), f"{what}: {int(bad.sum())} needle rows are not exactly their key's v"
        else:
            d = (got.double() - want.double()).abs() / ulp(want, dtype)
            nfrac = d.max().item()
            assert nfrac <= 1, f"{what}: a needle row is {nfrac} ulp from its key's v"
    # ties: two top keys with the same score (bit-identical K rows, or a flat row of two keys), ahead of the rest by
    # >= MARGIN
    sel = (lead == 0) & (lead3 >= MARGIN)
    if sel.any():
        a, b, h = top[sel], second[sel], hh[sel]
        want = (Vr[a, h] + Vr[b, h]) / 2
        d = (o[sel].double() - want).abs() / ulp(want, dtype)
        tfrac = d.max().item() / tie_ulps
        assert tfrac <= 1, f"{what}: a tie row is {d.max().item()} ulp from (v_a + v_b) / 2"
    return frac, nfrac, tfrac


# ---- prefill ---------------------------------------------------------------------------------------------------------
PREFILL_SPECS = [
    {"kind": "needle", "i": 0, "delta": 40.0},
    {"kind": "ramp", "slope": 7.5 / (64 * LOG2E)},          # +7.5 log2 units per 64-key tile: a lazy raise on every tile
    {"kind": "needle", "i": 1, "delta": 12.0},              # sink (key 0), below the exact-needle margin
    {"kind": "tie", "i": 2, "delta": 40.0},
    {"kind": "ramp", "slope": -2.0},                        # falling: later tiles underflow to p = 0
    {"kind": "flat"},
    {"kind": "needle", "i": 0, "delta": 12.0},              # 17.3 log2 units: a raise past kLazyMax, p <= 2^4 after it
    {"kind": "flat", "shift": 600.0},
    {"kind": "needle", "i": 0, "delta": 40.0, "shift": -600.0},
    {"kind": "needle", "i": 1, "delta": 40.0},
]


def _prefill_needles(L, KVH, salt):
    """Needle positions (one per kv head) for a sequence of L tokens: first / last token, both sides of a 16-key block
    and of a 64-key tile, keys in tiles >= 2; feature 1 is the sink (key 0)."""
    cand = [0, L - 1, 15, 16, 63, 64, 130, 200, 700, L // 2, L - 2]
    pos = [cand[(h + salt) % len(cand)] for h in range(KVH)]
    return [[min(p, L - 1) for p in pos], [0] * KVH]


def _prefill_state(lens, D, device):
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0)
    return NS(num_prefill_seqs=len(lens), max_prefill_len=max(lens), softmax_scale=D ** -0.5,
              prefill_seq_start_locs_with_end=cu.to(device), num_prefill_tokens=sum(lens))


@pytest.mark.parametrize("dtype", DTYPES)
# LDS-DMA kernel at D = 128 with two heads per workgroup (GQA 4) and one (MHA); the register kernel at D = 64 and 32
@pytest.mark.parametrize("H,KVH,D", [(32, 8, 128), (8, 8, 128), (8, 2, 64), (10, 10, 32)])
def test_prefill_attention_extreme_scores(dtype, H, KVH, D):
    """Varlen causal prefill, one launch, a different profile per head. Measured on MI355X: the general bound at
    <= 0.28 of it, the needles at 0 ulp (bound 1), the ties at <= 0.51 ulp (bound 1.5)."""
    g = gen(H * 7 + D + (dtype == torch.bfloat16))
    lens = [1, 63, 64, 65, 200, 1024]
    scale = D ** -0.5
    specs = [PREFILL_SPECS[h % len(PREFILL_SPECS)] for h in range(H)]
    qs, ks, vs, seqs = [], [], [], []
    for i, L in enumerate(lens):
        ties = [[(min(5, L - 1), min(70 + 13 * h, L - 1)) if L > 70 else None for h in range(KVH)]]
        k_, v_, F = make_kv(L, KVH, D, dtype, g, needles=_prefill_needles(L, KVH, i), ties=ties)
        q_ = make_q(L, H, D, F, dtype, g, specs, scale)
        qs.append(q_)
        ks.append(k_)
        vs.append(v_)
        seqs.append((q_, k_, v_))
    q, k, v = torch.cat(qs), torch.cat(ks), torch.cat(vs)
    mc = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D)
    o = torch.full_like(q, float("nan")).cuda()
    K().prefill_attention(q.cuda(), k.cuda(), v.cuda(), o, mc, None, _prefill_state(lens, D, "cuda"))
    o = o.cpu()
    assert torch.isfinite(o.float()).all()
    worst = [0.0, 0.0, 0.0]
    off = 0
    for (q_, k_, v_), L in zip(seqs, lens):
        ref = attn64(q_, k_, v_, scale, causal=True)
        s = scores64(q_, k_, scale)
        s = s.masked_fill(~(torch.arange(L)[None, :] <= torch.arange(L)[:, None])[:, None, :], float("-inf"))
        fr = _check_rows(o[off:off + L], ref, s, k_, v_, dtype, 3, False, 1.5, f"prefill L={L}")
        worst = [max(a, b) for a, b in zip(worst, fr)]
        off += L
    print(f"\n[prefill extremes {dtype} {H}/{KVH}/{D}] bound fractions: general {worst[0]:.3f} needle {worst[1]:.3f} "
          f"tie {worst[2]:.3f}")


# ---- paged decode ----------------------------------------------------------------------------------------------------
def _paged_setup(lens, KVH, D, L, layer, dtype, g, sbs, specs, nw):
    """Cache, block table and q for decode sequences of `lens`: the blocks of each sequence scattered over the pool,
    every kv head of every sequence with its own needle position. Needle candidates: first / last (the new token)
    key, both sides of a 16-key block and of a split, one key inside each wave's share of the workgroup (wave w
    attends blocks w, w + NW, ...). Rising ramps are anchored per sequence so their top sits near 0 nats."""
    seq_ids = list(range(1, 1 + len(lens)))
    nblk = sum(-(-n // 16) for n in lens) + 2
    kc = (torch.randn(nblk, L, KVH, 16, D, generator=g) * 3).to(dtype)     # other layers / blocks: junk
    vc = torch.randn(nblk, L, KVH, 16, D, generator=g).to(dtype)
    perm = torch.randperm(nblk, generator=g).tolist()
    bt = torch.zeros(len(lens) + 2, max(-(-max(lens) // 16), 1) + 1, dtype=torch.int32)
    qs, seqs = [], []
    for i, (sid, n) in enumerate(zip(seq_ids, lens)):
        cand = [0, n - 1, 15, 16, sbs - 1, sbs, 2 * sbs - 1] + [16 * w + 5 for w in range(nw)] + [n // 2, n - 17]
        needles = [[max(0, min(cand[(h * 3 + i) % len(cand)], n - 1)) for h in range(KVH)], [0] * KVH]
        ties = [[(min(3 + h, n - 1), n - 1 - h) if n > 2 * KVH + 4 else None for h in range(KVH)]]
        k_, v_, F = make_kv(n, KVH, D, dtype, g, needles=needles, ties=ties)
        sp = [dict(x, shift=x.get("shift", 0.0) - x["slope"] * (n - 1)) if x["kind"] == "ramp" and x["slope"] > 0
              else x for x in specs]
        q_ = make_q(1, len(specs), D, F, dtype, g, sp, D ** -0.5)
        for j in range(-(-n // 16)):
            blk = perm.pop()
            bt[sid, j] = blk
            t0, t1 = 16 * j, min(16 * j + 16, n)
            kc[blk, layer, :, :t1 - t0] = k_[t0:t1].transpose(0, 1)
            vc[blk, layer, :, :t1 - t0] = v_[t0:t1].transpose(0, 1)
        qs.append(q_[0])
        seqs.append((q_, k_, v_))
    return torch.stack(qs), kc, vc, bt, seq_ids, seqs


PAGED_SPECS = [
    {"kind": "needle", "i": 0, "delta": 40.0},
    {"kind": "ramp", "slope": 0.5},                         # rising: alpha = e^-8 on every block
    {"kind": "needle", "i": 1, "delta": 12.0},              # sink
    {"kind": "ramp", "slope": -2.0},                        # falling: later blocks, waves and splits hold no mass
    {"kind": "tie", "i": 2, "delta": 40.0},
    {"kind": "flat"},
    {"kind": "needle", "i": 0, "delta": 12.0, "shift": 600.0},
    {"kind": "needle", "i": 1, "delta": 40.0, "shift": -600.0},
    {"kind": "flat", "shift": -600.0},
]


def _paged_state(lens, seq_ids, sbs, D, device):
    return NS(num_decoding_seqs=len(lens), num_prefill_seqs=0, seq_block_size=sbs,
              num_seq_blocks=-(-max(lens) // sbs), softmax_scale=D ** -0.5,
              decoding_seq_lens=torch.tensor(lens, dtype=torch.int32, device=device),
              seq_ids=torch.tensor(seq_ids, dtype=torch.int32, device=device))


PAGED_CASES = [
    # H, KVH, D, sbs, lens
    (32, 8, 128, 64, [1, 17, 65, 300, 1500]),       # G = 4 matrix core, 4-wave workgroups, phase 2
    (32, 8, 128, 4096, [1, 33, 700, 4096]),         # G = 4, 8-wave, one split (direct store), flat up to 4k keys
    (8, 8, 128, 512, [2, 513, 1100]),               # G = 1 (VALU attend_block), 8-wave, phase 2
    (8, 4, 64, 128, [5, 129, 640]),                 # G = 2, 4-wave
    (16, 2, 32, 1024, [16, 1024, 2049]),            # G = 8, D = 32, 8-wave
    (9, 9, 64, 16, [2080, 31]),                     # G = 1, 130 splits: phase 2 past 64 partials from phase 1
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D,sbs,lens", PAGED_CASES)
def test_paged_attention_extreme_scores(dtype, H, KVH, D, sbs, lens):
    """swl_paged_attn_decode on every kernel variant the dispatch picks. Measured on MI355X: the general bound at
    <= 0.29 of it, the needles exact, the ties at 0.5 ulp (bound 1)."""
    g = gen(H * 5 + D + sbs + (dtype == torch.bfloat16))
    L, layer = 2, 1
    specs = [PAGED_SPECS[h % len(PAGED_SPECS)] for h in range(H)]
    nw = 8 if sbs >= 512 else 4
    q, kc, vc, bt, seq_ids, seqs = _paged_setup(lens, KVH, D, L, layer, dtype, g, sbs, specs, nw)
    o = torch.full_like(q, float("nan")).cuda()
    K().paged_attention(q.cuda(), kc.cuda(), vc.cuda(), bt.cuda(),
                        NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16),
                        _paged_state(lens, seq_ids, sbs, D, "cuda"), layer, o)
    o = o.cpu()
    assert torch.isfinite(o.float()).all()
    worst = [0.0, 0.0, 0.0]
    for i, (q_, k_, v_) in enumerate(seqs):
        ref = attn64(q_, k_, v_, D ** -0.5)
        fr = _check_rows(o[i:i + 1], ref, scores64(q_, k_, D ** -0.5), k_, v_, dtype, 2, True, 1.0,
                         f"decode seq {i} (len {lens[i]})")
        worst = [max(a, b) for a, b in zip(worst, fr)]
    print(f"\n[paged extremes {dtype} {H}/{KVH}/{D} sbs {sbs}] bound fractions: general {worst[0]:.3f} "
          f"tie {worst[2]:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D,sbs,lens", [(32, 8, 128, 64, [1, 17, 65, 300, 1500]),
                                              (8, 8, 64, 64, [640, 2, 129])])
def test_paged_phase1_partials_extreme_scores(dtype, H, KVH, D, sbs, lens):
    """swl_paged_attn_phase1: mid_o and mid_lse of every split against the fp64 per-split softmax, splits that hold
    no mass (falling ramp: LSE > 150 log2 units below the row's) included. mid_o is fp32 (P exact to 2^-16 or
    better, fp32 sums of <= 64 keys): |mid_o - o64| <= (2^-15 + 2 * 2^-22 log2(e) S) vmax, measured <= 0.06 of it;
    mid_lse: fp32 log2 of the split sum plus the scores' error, |lse - lse64| <= 2^-20 + 2 * 2^-22 log2(e) S (a few
    fp32 ulps of the score magnitude), measured <= 0.47 of it. Splits past a sequence are not written: they keep the
    -inf they were filled with."""
    from swiftllm_amd import _hip
    g = gen(H + D + sbs + 3 * (dtype == torch.bfloat16))
    L, layer = 1, 0
    specs = [PAGED_SPECS[h % len(PAGED_SPECS)] for h in range(H)]
    q, kc, vc, bt, seq_ids, seqs = _paged_setup(lens, KVH, D, L, layer, dtype, g, sbs, specs, 4)
    nd, nsb = len(lens), -(-max(lens) // sbs)
    mid_o = torch.full((nd, H, nsb, D), float("nan"), dtype=torch.float32, device="cuda")
    mid_lse = torch.full((nd, H, nsb), float("-inf"), dtype=torch.float32, device="cuda")
    st = _paged_state(lens, seq_ids, sbs, D, "cuda")
    qd, kd, vd, btd = q.cuda(), kc.cuda(), vc.cuda(), bt.cuda()
    _hip.call("swl_paged_attn_phase1", 0, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), btd.data_ptr(),
              st.seq_ids.data_ptr(), st.decoding_seq_lens.data_ptr(), mid_o.data_ptr(), mid_lse.data_ptr(),
              st.softmax_scale, nd, H, KVH, D, L, 16, layer, bt.shape[1], sbs, nsb, H * D, H * D,
              _hip.dtype_code(dtype), _hip.stream())
    mid_o, mid_lse = mid_o.cpu(), mid_lse.cpu()
    fo = fl = 0.0
    saw_empty = False
    for i, (q_, k_, v_) in enumerate(seqs):
        n = lens[i]
        ns = -(-n // sbs)
        assert torch.isfinite(mid_o[i, :, :ns]).all() and torch.isfinite(mid_lse[i, :, :ns]).all()
        assert torch.equal(mid_lse[i, :, ns:], torch.full((H, nsb - ns), float("-inf")))
        ref = attn64(q_, k_, v_, D ** -0.5, split=sbs)
        o64, l64, smag = ref["o_s"][0], ref["lse2_s"][0], ref["smag_s"][0]          # [H, ns, D], [H, ns], [H, ns]
        G = H // KVH
        Vr = v_.double().repeat_interleave(G, dim=1).abs()                          # [n, H, D]
        vmax = torch.stack([Vr[k0:k0 + sbs].amax(dim=(0, 2)) for k0 in range(0, n, sbs)], 1)   # [H, ns]
        b_o = (2.0 ** -15 + 2 * 2.0 ** -22 * LOG2E * smag) * vmax
        e_o = (mid_o[i, :, :ns].double() - o64).abs().amax(-1)
        assert (e_o <= b_o).all(), f"seq {i}: mid_o off by {(e_o / b_o).max().item():.2f} of the bound"
        b_l = 2.0 ** -20 + 2 * 2.0 ** -22 * LOG2E * smag
        e_l = (mid_lse[i, :, :ns].double() - l64).abs()
        assert (e_l <= b_l).all(), f"seq {i}: mid_lse off by {(e_l / b_l).max().item():.2f} of the bound"
        fo, fl = max(fo, (e_o / b_o).max().item()), max(fl, (e_l / b_l).max().item())
        saw_empty |= bool((l64.amax(-1, keepdim=True) - l64 > 150).any())
    assert saw_empty, "no split without mass: the falling ramp did not reach its regime"
    print(f"\n[phase 1 extremes {dtype} {H}/{KVH}/{D}] bound fractions: mid_o {fo:.3f} mid_lse {fl:.3f}")


# ---- flash-decoding merges: phase 2 and the tiny-batch o_proj ----------------------------------------------------------
def _wide_lse(g, H, n, nsb):
    """mid_lse [H, nsb] patterns per head (entries >= n are junk the merge must not read): the maximum after partial
    64 (and after partial 16) and > 128 above all before it; the maximum first with the rest 200 below; uniform in
    [-200, 200]; all equal; ~N(0, 9)."""
    lse = torch.full((H, nsb), float("nan"))
    for h in range(H):
        kind = h % 5
        x = torch.rand(n, generator=g) * 400 - 200
        if kind == 0:
            x = torch.rand(n, generator=g) * 40 - 200
            x[n - 1 if n > 64 else min(n - 1, 20)] = 150.0
        elif kind == 1:
            x = torch.full((n,), -200.0) + torch.rand(n, generator=g)
            x[0] = 0.0
        elif kind == 3:
            x = torch.full((n,), 7.25)
        elif kind == 4:
            x = torch.randn(n, generator=g) * 3
        lse[h, :n] = x
    return lse


def _merge64(mid_o, mid_lse, n):
    """fp64 LSE-weighted merge of the first n partials: mid_o [H, nsb, D], mid_lse [H, nsb] -> [H, D]."""
    l = mid_lse[:, :n].double()
    w = torch.exp2(l - l.amax(-1, keepdim=True))
    return (w[..., None] * mid_o[:, :n].double()).sum(1) / w.sum(-1, keepdim=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [128, 64, 32])
def test_paged_phase2_wide_lse_spreads(dtype, D):
    """swl_paged_attn_phase2 on synthetic partials, n in {1, 16, 17, 64, 65, 130}, LSEs over +-200 with the maximum past
    partial 64: |o - o64| <= 2 u vmax (the output rounding and fp32 sums) + 2^-22 (1 + max|lse|) vmax (the fp32
    difference lse - M before the exp2), measured <= 0.37 of it."""
    from swiftllm_amd import _hip
    g = gen(D + 11 * (dtype == torch.bfloat16))
    H, sbs, nsb = 5, 16, 130
    ns = [1, 16, 17, 64, 65, 130]
    mid_o = torch.randn(len(ns), H, nsb, D, generator=g)
    mid_lse = torch.stack([_wide_lse(g, H, n, nsb) for n in ns])
    lens = torch.tensor([16 * n - (n % 7) for n in ns], dtype=torch.int32)
    assert [-(-int(x) // sbs) for x in lens] == ns
    o = torch.full((len(ns), H, D), float("nan"), dtype=dtype, device="cuda")
    mo, ml, ld = mid_o.cuda(), mid_lse.cuda(), lens.cuda()
    _hip.call("swl_paged_attn_phase2", o.data_ptr(), mo.data_ptr(), ml.data_ptr(), ld.data_ptr(), len(ns), H, D, sbs,
              nsb, H * D, _hip.dtype_code(dtype), _hip.stream())
    o = o.cpu()
    assert torch.isfinite(o.float()).all()
    u = unit_roundoff(dtype)
    worst = 0.0
    for i, n in enumerate(ns):
        want = _merge64(mid_o[i], mid_lse[i], n)
        vmax = mid_o[i, :, :n].abs().amax(dim=(1, 2)).double()
        lmax = mid_lse[i, :, :n].abs().amax(-1).double()
        bound = ((2 * u + 2.0 ** -22 * (1 + lmax)) * vmax)[:, None]
        err = (o[i].double() - want).abs()
        assert (err <= bound).all(), f"n={n}: {(err / bound).max().item():.2f} of the bound"
        worst = max(worst, (err / bound).max().item())
    print(f"\n[phase 2 wide LSE {dtype} D={D}] bound fraction {worst:.3f}")


def _tiny_case(dtype, ns, g, H=8, D=128, N=256, nsb=130, sbs=16):
    import importlib
    Lm = importlib.import_module("swiftllm_amd.worker.kernels.linear")
    hid = H * D
    w = (torch.randn(N, hid, generator=g) * hid ** -0.5).to(dtype).cuda()
    Lm.pack_weight(w)
    M = len(ns)
    mid_o = torch.randn(M, H, nsb, D, generator=g)
    mid_lse = torch.stack([_wide_lse(g, H, max(n, 1), nsb) for n in ns])
    lens = [16 * n - (n % 5) if n > 0 else 0 for n in ns]
    return Lm, w, mid_o, mid_lse, lens


def _tiny_run(Lm, w, mid_o, mid_lse, lens, H, D, nsb, sbs, dtype):
    M = len(lens)
    scratch = torch.cat([mid_o.reshape(-1), mid_lse.reshape(-1)]).cuda()
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    assert Lm.attn_partials_ok(M, H, D, w)
    r = Lm.linear_splitk_from_attn_partials(scratch, sl, M, H, D, sbs, nsb, w, dtype)
    # (the slabs live in the shared split-K workspace: keep a private copy)
    slabs = r.slabs[:r.k_splits * M * w.shape[0]].clone().view(r.k_splits, M, w.shape[0])
    return r, slabs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ns", [[33], [128], [16, 17], [2, 17, 33, 128]])
def test_tiny_o_proj_merge_wide_lse_spreads(dtype, ns):
    """swl_gemm_tiny_partial_from_attn with n <= 16 and n > 16 partials (rows with different n in one launch,
    num_seq_blocks = 130 larger than every row's n, the graph-bucket stride), LSE spreads over +-200 with the largest
    after partial 16 and > 128 above the first 16: against an fp64 merge rounded to the storage dtype, then the product,
    to 4 eps of the output scale as tests/test_gpu_kernels.py's merge test (the merged row may sit one rounding away
    from the fp64 one), measured <= 0.001 of it."""
    g = gen(sum(ns) + 3 * (dtype == torch.bfloat16))
    H, D, nsb, sbs = 8, 128, 130, 16
    Lm, w, mid_o, mid_lse, lens = _tiny_case(dtype, ns, g)
    _, slabs = _tiny_run(Lm, w, mid_o, mid_lse, lens, H, D, nsb, sbs, dtype)
    out = slabs.sum(0).double().cpu()
    assert torch.isfinite(out).all()
    x64 = torch.stack([_merge64(mid_o[m], mid_lse[m], n).reshape(-1) for m, n in enumerate(ns)])
    out64 = x64.to(dtype).double() @ w.double().cpu().t()
    eps = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    bound = 4 * eps * max(1.0, float(out64.abs().max()))
    err = (out - out64).abs().max().item()
    assert err <= bound, f"{err:.3e} > {bound:.3e}"
    print(f"\n[tiny o_proj wide LSE {dtype} n={ns}] bound fraction {err / bound:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inert", [0, 1, 3])
def test_tiny_o_proj_length0_row_is_inert(dtype, inert):
    """A length-0 row (a padded decode slot) in swl_gemm_tiny_partial_from_attn: its slab rows are exactly 0, it reads
    no partial (its scratch is NaN here), and the other rows are bit-identical to a launch without it."""
    g = gen(inert + 7 * (dtype == torch.bfloat16))
    H, D, nsb, sbs = 8, 128, 40, 16
    ns = [3, 17, 40]
    ns_full = ns[:inert] + [0] + ns[inert:]
    Lm, w, mid_o, mid_lse, lens = _tiny_case(dtype, ns_full, g, nsb=nsb)
    mid_o[inert], mid_lse[inert] = float("nan"), float("nan")
    _, slabs = _tiny_run(Lm, w, mid_o, mid_lse, lens, H, D, nsb, sbs, dtype)
    keep = [m for m in range(4) if m != inert]
    _, ref = _tiny_run(Lm, w, mid_o[keep], mid_lse[keep], [lens[m] for m in keep], H, D, nsb, sbs, dtype)
    assert torch.isfinite(slabs).all()
    assert torch.equal(slabs[:, inert], torch.zeros_like(slabs[:, inert]))
    assert torch.equal(slabs[:, keep], ref)


# ---- slab-fed attention (rotary + KV store in the prologue) -----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sbs", [64, 1024])
@pytest.mark.parametrize("H,KVH,D,hid", [(32, 8, 128, 4096), (8, 8, 128, 512), (4, 2, 32, 128)])
def test_slab_fed_attention_peaked_cache_equals_three_kernels(dtype, sbs, H, KVH, D, hid):
    """paged_attention_from_qkv_splitk with the cache holding large-norm keys (|k| ~ 30 sqrt(D)) at block, split and
    wave boundaries, so that the attention is peaked whatever rotary does to q: the plain slab-fed kernel == rotary /
    store + paged attention, bit for bit; the deferred-norm form (_rs) == its phase-1-only form (_rs_partials) followed
    by phase 2, bit for bit (outputs and pools)."""
    from swiftllm_amd import _hip
    from swiftllm_amd.worker.kernels.linear import linear_splitk, SplitKPartials
    from swiftllm_amd.worker.kernels.paged_attn import paged_attention_from_qkv_splitk
    from swiftllm_amd.worker.kernels.rmsnorm import RowScalePending
    from swiftllm_amd.worker.kernels.rotary_emb import rotary_embedding_and_store_kvcache_decode_from_splitk
    g = gen(H * 3 + D + hid + sbs + (dtype == torch.bfloat16))
    L, layer = 2, 1
    lens = [1, 17, 65, 300, 1100]
    nd = len(lens)
    seq_ids = list(range(1, 1 + nd))
    nblk = sum(-(-n // 16) for n in lens) + 3
    kc = torch.randn(nblk, L, KVH, 16, D, generator=g)
    vc = torch.randn(nblk, L, KVH, 16, D, generator=g)
    perm = torch.randperm(nblk, generator=g).tolist()
    bt = torch.zeros(nd + 2, -(-max(lens) // 16) + 1, dtype=torch.int32)
    for sid, n in zip(seq_ids, lens):
        for j in range(-(-n // 16)):
            bt[sid, j] = perm.pop()
        for pos in {0, 15, 16, sbs - 1, sbs, 16 * 3 + 2, n // 2, n - 2}:
            if 0 <= pos < n - 1:
                blk = int(bt[sid, pos // 16])
                kc[blk, layer, :, pos % 16] *= 30.0
    kc, vc = kc.to(dtype), vc.to(dtype)
    n_qkv = (H + 2 * KVH) * D
    x = torch.randn(nd, hid, generator=g).to(dtype).cuda()
    wqkv = (torch.randn(n_qkv, hid, generator=g) * (hid ** -0.5)).to(dtype).cuda()
    ang = torch.rand(2048, D // 2, generator=g) * 6.28
    st = _paged_state(lens, seq_ids, sbs, D, "cuda")
    st.position_cos, st.position_sin = torch.cos(ang).to(dtype).cuda(), torch.sin(ang).to(dtype).cuda()
    st.position_indices = torch.tensor([v - 1 for v in lens], dtype=torch.int32, device="cuda")
    mc, ec = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16)
    part = linear_splitk(x, wqkv, always=True)
    assert isinstance(part, SplitKPartials) and part.k_splits in (1, 2, 4)
    part = SplitKPartials(part.slabs[:part.k_splits * nd * n_qkv].clone(), part.k_splits, nd, n_qkv, part.dtype)
    btc = bt.cuda()
    # plain: three kernels vs one
    kc1, vc1 = kc.cuda(), vc.cuda()
    q1, _, _ = rotary_embedding_and_store_kvcache_decode_from_splitk(part, kc1, vc1, btc, mc, ec, st, layer)
    o1 = torch.zeros(nd, H, D, dtype=dtype, device="cuda")
    K().paged_attention(q1, kc1, vc1, btc, mc, ec, st, layer, o1)
    kc2, vc2 = kc.cuda(), vc.cuda()
    o2 = torch.zeros(nd, H * D, dtype=dtype, device="cuda")
    paged_attention_from_qkv_splitk(part, kc2, vc2, btc, mc, ec, st, layer, o2)
    assert torch.isfinite(o1.float()).all() and torch.isfinite(o2.float()).all()
    assert torch.equal(o2.view(nd, H, D), o1)
    assert torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
    # deferred norm: merged in one launch vs phase 1 only + phase 2
    ssq = (torch.rand(1, nd, generator=g) * hid + hid / 4).float().cuda()
    rs = RowScalePending(None, ssq, 1, 1e-5, hid)
    kc3, vc3 = kc.cuda(), vc.cuda()
    o3 = torch.zeros(nd, H * D, dtype=dtype, device="cuda")
    paged_attention_from_qkv_splitk(part, kc3, vc3, btc, mc, ec, st, layer, o3, row_scale=rs)
    kc4, vc4 = kc.cuda(), vc.cuda()
    o4 = torch.zeros(nd, H * D, dtype=dtype, device="cuda")
    scratch = paged_attention_from_qkv_splitk(part, kc4, vc4, btc, mc, ec, st, layer, None if st.num_seq_blocks > 1
                                              else o4, row_scale=rs, merge=False)
    if st.num_seq_blocks > 1:
        nsb = st.num_seq_blocks
        mo = scratch[: nd * H * nsb * D]
        ml = scratch[nd * H * nsb * D: nd * H * nsb * (D + 1)]
        _hip.call("swl_paged_attn_phase2", o4.data_ptr(), mo.data_ptr(), ml.data_ptr(),
                  st.decoding_seq_lens.data_ptr(), nd, H, D, sbs, nsb, H * D, _hip.dtype_code(dtype), _hip.stream())
    assert torch.isfinite(o3.float()).all()
    assert torch.equal(o4, o3)
    assert torch.equal(kc4, kc3) and torch.equal(vc4, vc3)
