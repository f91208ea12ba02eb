"""FP8 (e4m3fn) KV cache on the GPU: quantising stores (bit-exact against tests/_fp8_ref.py), FP8 decode and chunked-
prefill attention against fp64 on the STORED values (code * scale — the conversion to the activation dtype is exact, so
the bounds are those of the 16-bit kernels: tests/test_gpu_attention_extremes.py, tests/test_gpu_chunked_prefill.py),
and the model end to end.

Scales. The kernels fold k_scale into the exp2 factor: c = fp32(fp32(scale * log2 e) * k_scale), one fp32 rounding more
than the 16-bit kernel's c — a relative 2^-24 on every exponent, against the 2 * 2^-22 log2(e) S the score term of the
bounds already grants for the fp32 dot products, the fma and c itself (S is computed on the stored values, k_scale
included). The term is not widened. v_scale multiplies the normalised fp32 output before its one rounding; the scales
used here have <= 5 significant bits, so code * v_scale is exact in fp32 and a needle row must be EXACTLY
round(v_scale * v8), as the 16-bit kernel's is exactly v.

Zeros. The needle and tie rules of the 16-bit tests are RELATIVE arguments — "o = v (1 + d) rounds to v", "within 1 ulp
of (v_a + v_b) / 2" — and their data (randn rounded to 16 bits) never holds an exact zero nor an exact v_a = -v_b. e4m3
does both all the time: |x| < 2^-10 * scale quantises to the code 0, and two of 254 values cancel often. There the exact
answer is not 0 but what the OTHER keys add, t = sum_j p_j v_j over the keys outside the needle / tie (each p_j <= e^-30),
which bfloat16 — whose exponent range is fp32's — represents, while float16 flushes it. _check_stored therefore keeps
the rules of tests/test_gpu_attention_extremes.py and tests/test_gpu_chunked_prefill.py bit for bit wherever they mean
something and replaces them only where the wanted value is (next to) zero:
  * needle element with round(v_scale * v8) != 0: as before (exact bits for decode, <= 1 ulp for prefill);
    == 0: |o| <= 2 t_abs, t_abs = sum_j p_j |v_j| from the fp64 softmax of the reference (never from the kernel) — once
    because it is in the exact answer, once because the kernel gets each term wrong by less than its own size (the
    argument tests/test_gpu_chunked_prefill.py makes for its ties);
  * tie element: |o - (v_a + v_b) / 2| <= max(tie_ulps * ulp(want), p_abs * max(|v_a|, |v_b|) + 2 t_abs). The second
    arm only matters under cancellation (|want| << |v_a|): p_abs is the absolute precision of one P v term relative to |v|
    — decode feeds P as hi + lo halves, 2^-16 relative per term, two terms: 2^-15; prefill rounds P to the storage dtype,
    u / 2 per term at p = 1/2, two terms: u. Without cancellation ulp(want) >= u |want| is the larger arm and the rule
    is the old one.
"""
import types

import pytest
import torch

import _fp8_ref as R
from _attn_cases import LOG2E, attn64, scores64

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace
DTYPES = [torch.float16, torch.bfloat16]
FP8 = torch.float8_e4m3fn
NAN_CODE = 0x7f


def _ext():
    import test_gpu_attention_extremes as m
    return m


def _chk():
    import test_gpu_chunked_prefill as m
    return m


def _scales(L, KVH, unit=False):
    """[2, L, KVH] fp32, short mantissas (see the module docstring); no two heads alike."""
    if unit:
        return torch.ones(2, L, KVH)
    vals = torch.tensor([0.75, 1.5, 0.4375, 1.25, 0.625, 2.0, 0.875, 1.0, 1.75, 0.5])
    idx = torch.arange(2 * L * KVH)
    return vals[(idx * 3 + 1) % len(vals)].reshape(2, L, KVH).contiguous()


def _check_stored(o, ref, s, V, dtype, c_round, needle_exact, tie_ulps, p_abs, what):
    """o [T, H, D] from the kernel, ref = attn64(...) on the stored values, s the masked fp64 scores [T, H, n], V the
    stored values [n, KVH, D] (fp64), all on one device. The general bound of the 16-bit tests, and their needle / tie
    rules with the zero cases of the module docstring. Returns the measured fractions (general, needle, tie)."""
    from _attn_cases import ulp, unit_roundoff
    E = _ext()
    T, H, D = o.shape
    G = H // V.shape[1]
    dev = o.device
    assert torch.isfinite(o.float()).all(), f"{what}: non-finite output"
    u = unit_roundoff(dtype)
    Vr = V.double().repeat_interleave(G, dim=1)                     # [n, H, D]
    vm = Vr.abs().amax(-1).t()                                      # [H, n]
    vmax = (vm[None] * torch.isfinite(s)).amax(-1)                  # [T, H]
    bound = (c_round * u + 2 * 2.0 ** -22 * LOG2E * ref["smag"]) * vmax
    err = (o.double() - ref["o"]).abs().amax(-1)
    frac = (err / bound).max().item()
    assert (err <= bound).all(), f"{what}: |o - o64| {err.max().item():.3e} > bound (worst {frac:.2f} of it)"
    top, lead, second, lead3 = E._top2(s)
    hh = torch.arange(H, device=dev)[None, :].expand(T, H)
    nfrac = tfrac = 0.0

    def others(sel, drop):
        """t_abs [rows, D] and the other keys' total weight [rows, 1] for the selected rows, the keys in `drop` removed."""
        rows_t, rows_h = sel.nonzero(as_tuple=True)
        t_abs = torch.zeros(rows_t.numel(), D, dtype=torch.float64, device=dev)
        wsum = torch.zeros(rows_t.numel(), 1, dtype=torch.float64, device=dev)
        for head in rows_h.unique().tolist():
            m = rows_h == head
            pr = torch.softmax(s[rows_t[m], head], dim=-1)           # [R, n] fp64, masked keys exactly 0
            for idx in drop:
                pr = pr.scatter(1, idx[m][:, None], 0.0)
            t_abs[m] = pr @ Vr[:, head].abs()
            wsum[m] = pr.sum(-1, keepdim=True)
        return t_abs, wsum

    sel = lead >= E.MARGIN
    if sel.any():
        want = Vr[top[sel], hh[sel]].to(dtype)                       # [rows, D]: round(v_scale * v8)
        got = o[sel]
        t_abs, _ = others(sel, [top[sel]])
        zero = want == 0
        assert (got.double().abs()[zero] <= 2 * t_abs[zero]).all(), f"{what}: a needle element whose v is 0 is off"
        if needle_exact:
            bad = ((got != want) & ~zero).any(-1)
            assert not bad.any(), f"{what}: {int(bad.sum())} needle rows are not exactly their key's v"
        else:
            d = ((got.double() - want.double()).abs() / ulp(want, dtype))[~zero]
            nfrac = d.max().item() if d.numel() else 0.0
            assert nfrac <= 1, f"{what}: a needle row is {nfrac} ulp from its key's v"
    sel = (lead == 0) & (lead3 >= E.MARGIN)
    if sel.any():
        a, b, h = top[sel], second[sel], hh[sel]
        va, vb = Vr[a, h], Vr[b, h]
        want = (va + vb) / 2
        t_abs, wsum = others(sel, [a, b])
        floor = p_abs * torch.maximum(va.abs(), vb.abs()) + 2 * (t_abs + wsum * want.abs())
        tol = torch.maximum(tie_ulps * ulp(want, dtype), floor)
        d = (o[sel].double() - want).abs() / tol
        tfrac = d.max().item()
        assert tfrac <= 1, f"{what}: a tie row is {tfrac:.3f} of its tolerance from (v_a + v_b) / 2"
    return frac, nfrac, tfrac


# ---- a. stores, bit-exact ----------------------------------------------------------------------------------------------
def _qkv(T, H, KVH, D, dtype, g, scales, layer):
    """A fused qkv output [T, (H + 2 KVH) D]; k and v are strided slices of it. Values: N(0, 1) * scale with elements
    pushed beyond +-448 * scale, into the e4m3 subnormal range (|x| < 2^-6 * scale), onto rounding ties and to zero."""
    qkv = torch.randn(T, (H + 2 * KVH) * D, generator=g)
    k = qkv[:, H * D:(H + KVH) * D].view(T, KVH, D)
    v = qkv[:, (H + KVH) * D:].view(T, KVH, D)
    for x, s in ((k, scales[0, layer]), (v, scales[1, layer])):
        x *= s[None, :, None] * 8
        x[:, :, 0] *= 200.0                                  # saturates
        x[:, :, 1] = s[None, :] * 1e4 * torch.sign(x[:, :, 1])
        x[:, :, 2] *= 2.0 ** -10                             # subnormal codes and zeros
        x[:, :, 3] = s[None, :] * 2.0 ** -9 * torch.randint(-20, 21, x[:, :, 3].shape, generator=g) * 0.5   # ties, subnormal
        x[:, :, 4] = s[None, :] * (17.0 + 2 * torch.randint(0, 8, x[:, :, 4].shape, generator=g))           # ties at 16..32
        x[:, :, 5] = 0.0
        x[:, :, 6] = -0.0
    qkv = qkv.to(dtype)
    return qkv, qkv[:, H * D:(H + KVH) * D].view(T, KVH, D), qkv[:, (H + KVH) * D:].view(T, KVH, D)


def _on_gpu(qkv, H, KVH, D):
    """The same strided k / v slices of the fused output, on the device."""
    d = qkv.cuda()
    T = d.shape[0]
    k, v = d[:, H * D:(H + KVH) * D].view(T, KVH, D), d[:, (H + KVH) * D:].view(T, KVH, D)
    assert not k.is_contiguous() and k.stride(0) == (H + 2 * KVH) * D
    return k, v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("KVH,D", [(8, 128), (2, 64), (3, 32)])
@pytest.mark.parametrize("with_ctx", [False, True])
def test_prefill_store_bytes_equal_the_reference(dtype, KVH, D, with_ctx):
    from swiftllm_amd.worker.kernels.kvcache_mgmt import store_kvcache
    g = torch.Generator().manual_seed(KVH + D + with_ctx)
    L, layer, H = 3, 1, 2 * KVH
    lens = [1, 16, 17, 47, 5]
    ctxs = [0, 3, 16, 30, 15] if with_ctx else [0] * 5
    scales = _scales(L, KVH)
    inv = R.inv_scale(scales)
    T = sum(lens)
    qkv, k, v = _qkv(T, H, KVH, D, dtype, g, scales, layer)
    need = [-(-(c + n) // 16) for c, n in zip(ctxs, lens)]
    nb = sum(need) + 3
    perm = torch.randperm(nb, generator=g).tolist()
    bt = torch.full((8, 8), perm[-1], dtype=torch.int32)
    seq_ids = [6, 0, 3, 5, 2]
    want_k = torch.full((nb, L, KVH, 16, D), 0x5a, dtype=torch.uint8)
    want_v = torch.full((nb, L, KVH, 16, D), 0x5a, dtype=torch.uint8)
    off = 0
    for sid, c, n, nblk in zip(seq_ids, ctxs, lens, need):
        mine = torch.tensor([perm.pop() for _ in range(nblk)])
        bt[sid, :nblk] = mine.to(torch.int32)
        pos = torch.arange(c, c + n)
        want_k[mine[pos // 16], layer, :, pos % 16] = R.codes(R.quantise(k[off:off + n], inv[0, layer][None, :, None]))
        want_v[mine[pos // 16], layer, :, pos % 16] = R.codes(R.quantise(v[off:off + n], inv[1, layer][None, :, None]))
        off += n
    kc = torch.full((nb, L, KVH, 16, D), 0x5a, dtype=torch.uint8, device="cuda").view(FP8)
    vc = torch.full((nb, L, KVH, 16, D), 0x5a, dtype=torch.uint8, device="cuda").view(FP8)
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0)
    st = NS(num_prefill_seqs=len(lens), max_prefill_len=max(lens), num_prefill_tokens=T, num_decoding_seqs=0,
            prefill_seq_start_locs=cu[:-1].cuda(), prefill_seq_lens=torch.tensor(lens, dtype=torch.int32).cuda(),
            prefill_ctx_lens=torch.tensor(ctxs, dtype=torch.int32).cuda() if with_ctx else None,
            seq_ids=torch.tensor(seq_ids, dtype=torch.int32).cuda(), decoding_seq_lens=torch.zeros(0, dtype=torch.int32).cuda(),
            kv_inv_scales=inv.cuda(), kv_scales=scales.cuda())
    kd, vd = _on_gpu(qkv, H, KVH, D)
    store_kvcache(kd, vd, kc, vc, bt.cuda(), NS(num_layers=L, num_kv_heads=KVH, head_dim=D), NS(block_size=16), st, layer)
    torch.cuda.synchronize()
    assert torch.equal(kc.view(torch.uint8).cpu(), want_k), "K pool bytes differ from the reference (or a slot outside the chunk was touched)"
    assert torch.equal(vc.view(torch.uint8).cpu(), want_v), "V pool bytes differ from the reference (or a slot outside the chunk was touched)"
    assert (want_k == 0x7e).any() and (want_k == 0xfe).any(), "no saturated code in the data"
    assert ((want_k & 0x78) == 0).any(), "no subnormal code in the data"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("KVH,D", [(8, 128), (2, 64), (3, 32)])
def test_decode_store_bytes_equal_the_reference(dtype, KVH, D):
    from swiftllm_amd.worker.kernels.kvcache_mgmt import store_kvcache
    g = torch.Generator().manual_seed(KVH * 3 + D)
    L, layer, H = 2, 1, KVH
    lens = [1, 16, 17, 100, 0, 33]          # 0: an inert row of a padded batch
    scales = _scales(L, KVH)
    inv = R.inv_scale(scales)
    qkv, k, v = _qkv(len(lens), H, KVH, D, dtype, g, scales, layer)
    nb = 12
    bt = torch.randint(0, nb, (8, 8), generator=g).to(torch.int32)
    seq_ids = [1, 2, 3, 4, 4, 6]
    for i, sid in enumerate(seq_ids):        # distinct target blocks
        if lens[i] > 0:
            bt[sid, (lens[i] - 1) // 16] = i
    want_k = torch.full((nb, L, KVH, 16, D), 0xa5, dtype=torch.uint8)
    want_v = want_k.clone()
    for i, (sid, n) in enumerate(zip(seq_ids, lens)):
        if n > 0:
            want_k[i, layer, :, (n - 1) % 16] = R.codes(R.quantise(k[i], inv[0, layer][:, None]))
            want_v[i, layer, :, (n - 1) % 16] = R.codes(R.quantise(v[i], inv[1, layer][:, None]))
    kc = torch.full((nb, L, KVH, 16, D), 0xa5, dtype=torch.uint8, device="cuda").view(FP8)
    vc = torch.full((nb, L, KVH, 16, D), 0xa5, dtype=torch.uint8, device="cuda").view(FP8)
    st = NS(num_prefill_seqs=0, num_prefill_tokens=0, num_decoding_seqs=len(lens), prefill_ctx_lens=None,
            seq_ids=torch.tensor(seq_ids, dtype=torch.int32).cuda(),
            decoding_seq_lens=torch.tensor(lens, dtype=torch.int32).cuda(), kv_inv_scales=inv.cuda())
    kd, vd = _on_gpu(qkv, H, KVH, D)
    store_kvcache(kd, vd, kc, vc, bt.cuda(), NS(num_layers=L, num_kv_heads=KVH, head_dim=D), NS(block_size=16),
                  st, layer)
    torch.cuda.synchronize()
    assert torch.equal(kc.view(torch.uint8).cpu(), want_k) and torch.equal(vc.view(torch.uint8).cpu(), want_v)


# ---- b-d. decode attention ------------------------------------------------------------------------------------------------
def _fp8_paged(lens, H, KVH, D, L, layer, dtype, g, sbs, nw, nan_fill=False, unit=False):
    """The 16-bit case of test_gpu_attention_extremes._paged_setup, quantised: pools of codes, and per sequence the fp64
    stored values (code * scale) the reference runs on."""
    E = _ext()
    specs = [E.PAGED_SPECS[h % len(E.PAGED_SPECS)] for h in range(H)]
    q, kc, vc, bt, seq_ids, seqs = E._paged_setup(lens, KVH, D, L, layer, dtype, g, sbs, specs, nw)
    scales = _scales(L, KVH, unit)
    inv = R.inv_scale(scales)
    kc8 = R.quantise(kc, inv[0][None, :, :, None, None])
    vc8 = R.quantise(vc, inv[1][None, :, :, None, None])
    if nan_fill:        # every slot past a sequence's length and every block nobody owns: the NaN code
        keep = torch.zeros(kc.shape[0], 16, dtype=torch.bool)
        for sid, n in zip(seq_ids, lens):
            pos = torch.arange(n)
            keep[bt[sid, pos // 16].long(), pos % 16] = True
        for pool in (kc8, vc8):
            raw = pool.view(torch.uint8)
            raw[~keep[:, None, None, :, None].expand_as(raw)] = NAN_CODE
    stored = []
    for q_, k_, v_ in seqs:
        kd = R.dequantise(R.quantise(k_, inv[0, layer][None, :, None])) * scales[0, layer].double()[None, :, None]
        vd = R.dequantise(R.quantise(v_, inv[1, layer][None, :, None])) * scales[1, layer].double()[None, :, None]
        stored.append((q_, kd, vd))
    return q, kc8, vc8, bt, seq_ids, stored, scales


def _run_decode(q, kc8, vc8, bt, seq_ids, scales, lens, H, KVH, D, L, layer, sbs):
    E = _ext()
    o = torch.full_like(q, float("nan")).cuda()
    st = E._paged_state(lens, seq_ids, sbs, D, "cuda")
    st.kv_scales = scales.cuda()
    E.K().paged_attention(q.cuda(), kc8.cuda(), vc8.cuda(), bt.cuda(),
                          NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16), st, layer, o)
    torch.cuda.synchronize()
    return o.cpu()


FP8_PAGED_CASES = [
    # H, KVH, D, sbs, lens                          (G, waves, splits)
    (32, 8, 128, 64, [1, 17, 65, 300, 1500]),       # G = 4, 4-wave workgroups, phase 2
    (32, 8, 128, 4096, [1, 33, 700, 4096]),         # G = 4, 8-wave, one split (direct store)
    (8, 8, 128, 512, [2, 513, 1100, 1024, 512]),    # G = 1 on the matrix-core path, 8-wave, lengths at split boundaries
    (8, 4, 64, 128, [5, 129, 640, 128, 16]),        # G = 2, D = 64, 4-wave
    (16, 2, 32, 1024, [16, 1024, 2049]),            # G = 8, D = 32 (half-wave tiles), 8-wave
    (8, 1, 64, 2048, [31, 32, 2048]),               # G = 8, D = 64, one split
    (4, 4, 32, 64, [64, 65, 200]),                  # G = 1, D = 32
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D,sbs,lens", FP8_PAGED_CASES)
def test_fp8_paged_attention_extreme_scores(dtype, H, KVH, D, sbs, lens):
    """swl_paged_attn_decode_fp8 against fp64 on the stored values, the bounds of the 16-bit kernel: general rows
    |o - o64| <= (2u + 2 * 2^-22 log2(e) S) vmax, needle rows EXACTLY round(v_scale * v8), ties within 1 ulp.
    Measured on MI355X: the general bound at <= 0.29 of it, the needles exact, the ties at 0.5 of their tolerance."""
    E = _ext()
    g = E.gen(H * 5 + D + sbs + (dtype == torch.bfloat16))
    L, layer = 2, 1
    nw = 8 if sbs >= 512 else 4
    q, kc8, vc8, bt, seq_ids, stored, scales = _fp8_paged(lens, H, KVH, D, L, layer, dtype, g, sbs, nw)
    o = _run_decode(q, kc8, vc8, bt, seq_ids, scales, lens, H, KVH, D, L, layer, sbs)
    assert torch.isfinite(o.float()).all()
    worst = [0.0, 0.0, 0.0]
    for i, (q_, kd, vd) in enumerate(stored):
        ref = attn64(q_, kd, vd, D ** -0.5)
        fr = _check_stored(o[i:i + 1], ref, scores64(q_, kd, D ** -0.5), vd, dtype, 2, True, 1.0, 2.0 ** -15,
                           f"fp8 decode seq {i} (len {lens[i]})")
        worst = [max(a, b) for a, b in zip(worst, fr)]
    print(f"\n[fp8 paged extremes {dtype} {H}/{KVH}/{D} sbs {sbs}] bound fractions: general {worst[0]:.3f} "
          f"tie {worst[2]:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D,sbs,lens", [(32, 8, 128, 64, [1, 17, 65, 300, 1500]), (8, 8, 64, 2048, [31, 2, 700]),
                                              (16, 2, 32, 1024, [16, 1030])])
def test_fp8_paged_attention_ignores_nan_codes_past_the_length(dtype, H, KVH, D, sbs, lens):
    """Code 0x7f (NaN) in every slot past each sequence's length and in every unowned block: the outputs are finite and
    bit-equal to the run on pools holding quantised junk there."""
    E = _ext()
    L, layer = 2, 1
    nw = 8 if sbs >= 512 else 4
    outs = []
    for nan_fill in (False, True):
        g = E.gen(77 + D)
        q, kc8, vc8, bt, seq_ids, stored, scales = _fp8_paged(lens, H, KVH, D, L, layer, dtype, g, sbs, nw, nan_fill)
        outs.append(_run_decode(q, kc8, vc8, bt, seq_ids, scales, lens, H, KVH, D, L, layer, sbs))
    assert torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D,sbs,lens", [(32, 8, 128, 64, [1, 17, 65, 300, 1500]), (8, 8, 64, 64, [640, 2, 129])])
def test_fp8_phase1_partials(dtype, H, KVH, D, sbs, lens):
    """swl_paged_attn_phase1_fp8: mid_o / mid_lse of every split against the fp64 per-split softmax on the stored values,
    to the bounds of test_paged_phase1_partials_extreme_scores: |mid_o - o64| <= (2^-15 + 2 * 2^-22 log2(e) S) vmax,
    |lse - lse64| <= 2^-20 + 2 * 2^-22 log2(e) S. Splits past a sequence keep the -inf they were filled with.
    Measured on MI355X: mid_o at <= 0.04 of its bound, mid_lse at <= 0.47."""
    from swiftllm_amd import _hip
    E = _ext()
    g = E.gen(H + D + sbs + 3 * (dtype == torch.bfloat16))
    L, layer = 1, 0
    q, kc8, vc8, bt, seq_ids, stored, scales = _fp8_paged(lens, H, KVH, D, L, layer, dtype, g, sbs, 4)
    nd, nsb = len(lens), -(-max(lens) // sbs)
    mid_o = torch.full((nd, H, nsb, D), float("nan"), dtype=torch.float32, device="cuda")
    mid_lse = torch.full((nd, H, nsb), float("-inf"), dtype=torch.float32, device="cuda")
    st = E._paged_state(lens, seq_ids, sbs, D, "cuda")
    qd, kd_, vd_, btd, sc = q.cuda(), kc8.cuda(), vc8.cuda(), bt.cuda(), scales.cuda()
    _hip.call("swl_paged_attn_phase1_fp8", 0, qd.data_ptr(), kd_.data_ptr(), vd_.data_ptr(), sc.data_ptr(), btd.data_ptr(),
              st.seq_ids.data_ptr(), st.decoding_seq_lens.data_ptr(), mid_o.data_ptr(), mid_lse.data_ptr(),
              st.softmax_scale, nd, H, KVH, D, L, 16, layer, bt.shape[1], sbs, nsb, H * D, H * D,
              _hip.dtype_code(dtype), _hip.stream())
    mid_o, mid_lse = mid_o.cpu(), mid_lse.cpu()
    fo = fl = 0.0
    for i, (q_, kd, vd) in enumerate(stored):
        n = lens[i]
        ns = -(-n // sbs)
        assert torch.isfinite(mid_o[i, :, :ns]).all() and torch.isfinite(mid_lse[i, :, :ns]).all()
        assert torch.equal(mid_lse[i, :, ns:], torch.full((H, nsb - ns), float("-inf")))
        ref = attn64(q_, kd, vd, D ** -0.5, split=sbs)
        o64, l64, smag = ref["o_s"][0], ref["lse2_s"][0], ref["smag_s"][0]
        Vr = vd.repeat_interleave(H // KVH, dim=1).abs()
        vmax = torch.stack([Vr[k0:k0 + sbs].amax(dim=(0, 2)) for k0 in range(0, n, sbs)], 1)
        b_o = (2.0 ** -15 + 2 * 2.0 ** -22 * LOG2E * smag) * vmax
        e_o = (mid_o[i, :, :ns].double() - o64).abs().amax(-1)
        fo = max(fo, (e_o / b_o).max().item())
        assert (e_o <= b_o).all(), f"seq {i}: mid_o off by {(e_o / b_o).max().item():.2f} of the bound"
        b_l = 2.0 ** -20 + 2 * 2.0 ** -22 * LOG2E * smag
        e_l = (mid_lse[i, :, :ns].double() - l64).abs()
        fl = max(fl, (e_l / b_l).max().item())
        assert (e_l <= b_l).all(), f"seq {i}: mid_lse off by {(e_l / b_l).max().item():.2f} of the bound"
    print(f"\n[fp8 phase 1 {dtype} {H}/{KVH}/{D}] bound fractions: mid_o {fo:.3f} mid_lse {fl:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_paged_attention_is_run_to_run_deterministic(dtype):
    E = _ext()
    H, KVH, D, sbs, lens = 32, 8, 128, 256, [1, 300, 1500, 1027]
    q, kc8, vc8, bt, seq_ids, stored, scales = _fp8_paged(lens, H, KVH, D, 2, 1, dtype, E.gen(3), sbs, 4)
    dev = [t.cuda() for t in (q, kc8, vc8, bt, scales)]
    st = E._paged_state(lens, seq_ids, sbs, D, "cuda")
    st.kv_scales = dev[4]
    outs = []
    for _ in range(12):
        o = torch.full_like(dev[0], float("nan"))
        E.K().paged_attention(dev[0], dev[1], dev[2], dev[3], NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=2),
                              NS(block_size=16), st, 1, o)
        outs.append(o)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


# ---- d2 / e2. one pool of e4m3 values, stored as bytes or as 16-bit elements: the same bits --------------------------------
def _two_pools(shape, dtype, g):
    """K = randn * 0.5 and V = randn quantised at unit scale, in EVERY slot (slots past a length and unowned blocks hold
    finite codes too): the byte pools, and 16-bit pools holding exactly the same values."""
    k8 = R.quantise(torch.randn(shape, generator=g) * 0.5, 1.0)
    v8 = R.quantise(torch.randn(shape, generator=g), 1.0)
    return k8, v8, R.dequantise(k8, dtype), R.dequantise(v8, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D,sbs,lens", [FP8_PAGED_CASES[i] for i in (0, 3, 4, 5)])
def test_decode_bits_do_not_depend_on_the_pool_format(dtype, H, KVH, D, sbs, lens):
    """Matrix-core decode (G >= 2; at G = 1 the 16-bit kernel takes the VALU path) over a pool of e4m3 values at unit
    scales: swl_paged_attn_decode on the 16-bit copy and swl_paged_attn_decode_fp8 on the bytes give the same bits, and so
    do the phase-1 partials of the two entry points (first case)."""
    from swiftllm_amd import _hip
    E = _ext()
    g = E.gen(H * 7 + D + sbs + (dtype == torch.bfloat16))
    L, layer = 2, 1
    need = [-(-n // 16) for n in lens]
    nb = sum(need) + 3
    perm = torch.randperm(nb, generator=g)
    seq_ids = list(range(1, 1 + len(lens)))
    bt = torch.full((len(lens) + 2, max(need) + 1), int(perm[-1]), dtype=torch.int32)
    off = 0
    for sid, nblk in zip(seq_ids, need):
        bt[sid, :nblk] = perm[off:off + nblk].to(torch.int32)
        off += nblk
    k8, v8, k16, v16 = _two_pools((nb, L, KVH, 16, D), dtype, g)
    q = (torch.randn(len(lens), H, D, generator=g) * 0.5).to(dtype).cuda()
    st = E._paged_state(lens, seq_ids, sbs, D, "cuda")
    st.kv_scales = _scales(L, KVH, unit=True).cuda()
    mc, ec, btd = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16), bt.cuda()
    pools = {"fp8": (k8.cuda(), v8.cuda()), "16-bit": (k16.cuda(), v16.cuda())}
    outs = {}
    for name, (kc, vc) in pools.items():
        o = torch.full_like(q, float("nan"))
        E.K().paged_attention(q, kc, vc, btd, mc, ec, st, layer, o)
        outs[name] = o
    torch.cuda.synchronize()
    assert torch.isfinite(outs["fp8"].float()).all()
    assert torch.equal(outs["fp8"], outs["16-bit"]), "the output depends on the pool format"
    if (H, KVH, D, sbs) != FP8_PAGED_CASES[0][:4]:
        return
    nd, nsb = len(lens), -(-max(lens) // sbs)
    mids = {}
    for name, (kc, vc) in pools.items():
        mid_o = torch.full((nd, H, nsb, D), float("nan"), dtype=torch.float32, device="cuda")
        mid_lse = torch.full((nd, H, nsb), float("-inf"), dtype=torch.float32, device="cuda")
        tail = (btd.data_ptr(), st.seq_ids.data_ptr(), st.decoding_seq_lens.data_ptr(), mid_o.data_ptr(), mid_lse.data_ptr(),
                st.softmax_scale, nd, H, KVH, D, L, 16, layer, bt.shape[1], sbs, nsb, H * D, H * D, _hip.dtype_code(dtype),
                _hip.stream())
        if name == "fp8":
            _hip.call("swl_paged_attn_phase1_fp8", 0, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), st.kv_scales.data_ptr(), *tail)
        else:
            _hip.call("swl_paged_attn_phase1", 0, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), *tail)
        mids[name] = (mid_o, mid_lse)
    torch.cuda.synchronize()
    written = torch.isfinite(mids["fp8"][1])
    assert written.any() and torch.equal(written, torch.isfinite(mids["16-bit"][1]))
    assert torch.equal(mids["fp8"][1], mids["16-bit"][1]), "mid_lse depends on the pool format"
    assert torch.equal(mids["fp8"][0][written], mids["16-bit"][0][written]), "mid_o depends on the pool format"


# ---- e. chunked prefill -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D", [(8, 2, 128), (4, 2, 64), (4, 4, 32)])
def test_fp8_paged_prefill_attention(dtype, H, KVH, D):
    """swl_prefill_attn_paged_fp8 against attn64(causal=True) on the stored values: the bounds of
    tests/test_gpu_chunked_prefill.py (c = 3, needles <= 1 ulp, ties 1.5 ulp). Contexts 0, mid-block, >= one tile and past
    several; every slot past c + n and every unowned block holds the NaN code 0x7f.
    Measured on MI355X: the general bound at <= 0.30 of it, the needles at 0 ulp, the ties at 0.33 of their tolerance."""
    C = _chk()
    from swiftllm_amd.worker.kernels.prefill_attn import prefill_attention_paged
    g = C.gen(H * 11 + D + (dtype == torch.bfloat16))
    L, layer = C.NUM_LAYERS, C.LAYER
    scales = _scales(L, KVH)
    inv = R.inv_scale(scales)
    worst = [0.0, 0.0, 0.0]
    for n in (1, 37, 200):
        ctxs = [0, 5, 16, 64, 100, 331]
        seqs = [C._make_seq(c, n, H, KVH, D, dtype, g, i) for i, c in enumerate(ctxs)]
        need = [-(-k.shape[0] // 16) for _, k, _ in seqs]
        nb, ids = C._block_ids(sum(need))
        kc = torch.full((nb, L, KVH, 16, D), NAN_CODE, dtype=torch.uint8)
        vc = torch.full((nb, L, KVH, 16, D), NAN_CODE, dtype=torch.uint8)
        mbps = max(need) + 3
        rows = len(seqs) + 2
        bt = torch.full((rows, mbps), ids[-1], dtype=torch.int32)
        seq_ids, off, stored = [], 0, []
        for i, ((q_, k_, v_), nblk) in enumerate(zip(seqs, need)):
            row = rows - 1 - i
            mine = torch.tensor(ids[off:off + nblk], dtype=torch.int64)
            off += nblk
            bt[row, :nblk] = mine.to(torch.int32)
            pos = torch.arange(k_.shape[0])
            k8 = R.quantise(k_, inv[0, layer][None, :, None])
            v8 = R.quantise(v_, inv[1, layer][None, :, None])
            kc[mine[pos // 16], layer, :, pos % 16] = R.codes(k8)
            vc[mine[pos // 16], layer, :, pos % 16] = R.codes(v8)
            seq_ids.append(row)
            stored.append((q_, R.dequantise(k8) * scales[0, layer].double()[None, :, None],
                           R.dequantise(v8) * scales[1, layer].double()[None, :, None]))
        lens = [n] * len(seqs)
        q = torch.cat([s[0] for s in seqs]).cuda()
        o = torch.full_like(q, float("nan"))
        st = C._state(ctxs, lens, D, torch.tensor(seq_ids, dtype=torch.int32))
        st.kv_scales = scales.cuda()
        prefill_attention_paged(q, kc.cuda().view(FP8), vc.cuda().view(FP8), bt.cuda(), o,
                                NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16), st, layer)
        torch.cuda.synchronize()
        off = 0
        for c, (q_, kd, vd) in zip(ctxs, stored):
            ref, s, vdev = C._reference(q_, kd, vd, D)
            fr = _check_stored(o[off:off + n], ref, s, vdev, dtype, 3, False, 1.5, 2.0 ** (-11 if dtype == torch.float16 else -8),
                               f"fp8 paged prefill c={c} n={n}")
            worst = [max(a, b) for a, b in zip(worst, fr)]
            off += n
    print(f"\n[fp8 paged prefill {dtype} {H}/{KVH}/{D}] bound fractions: general {worst[0]:.3f} needle {worst[1]:.3f} "
          f"tie {worst[2]:.3f}")


CROSS_FORMAT_CHUNKS = [(0, 1), (0, 130), (5, 130), (64, 64), (200, 17), (37, 0)]     # (context, new tokens) of one launch


@pytest.mark.parametrize("dtype", [torch.bfloat16])
@pytest.mark.parametrize("H,KVH,D", [(8, 2, 128), (4, 2, 64), (4, 4, 32)])
def test_chunked_prefill_bits_do_not_depend_on_the_pool_format(dtype, H, KVH, D):
    """One kernel for both pool formats: over a pool of e4m3 values at unit scales, swl_prefill_attn_paged on the 16-bit
    copy and swl_prefill_attn_paged_fp8 on the bytes give the same bits. One launch with two q-blocks, a partial last
    tile, a tile-aligned context, staging passes that span two pool blocks, the non-staging threads of D = 32 and an
    empty chunk. The inputs are checked first: in fp64 the largest softmax weight is below 0.9 for at least half of the
    rows that see >= 8 keys, so the comparison is not one between one-hot rows.
    bfloat16 only. With float16 the two formats differ by 1 ulp in about 2^-15 of the output elements, and did before the
    kernels were merged (measured on MI355X with these inputs: 1 of 43 776 elements at D = 32, 11 of 350 208 at D = 128,
    each format repeatable): the 16-bit epilogue's `ot * inv` and its rounding become one v_fma_mixlo_f16 — the exact
    product rounded once — while the FP8 epilogue rounds `ot * inv` to fp32 for the v_scale multiply first (DESIGN.md
    section 3). bfloat16 has no such instruction: both formats round to fp32, then once to bfloat16."""
    C = _chk()
    from swiftllm_amd.worker.kernels.prefill_attn import prefill_attention_paged
    g = C.gen(H * 13 + D + (dtype == torch.bfloat16))
    L, layer = 2, 1
    ctxs, lens = [c for c, _ in CROSS_FORMAT_CHUNKS], [n for _, n in CROSS_FORMAT_CHUNKS]
    need = [-(-(c + n) // 16) for c, n in CROSS_FORMAT_CHUNKS]
    nb = sum(need) + 3
    perm = torch.randperm(nb, generator=g)
    rows = len(lens) + 2
    bt = torch.full((rows, max(need) + 3), int(perm[-1]), dtype=torch.int32)
    seq_ids, mine, off = [], [], 0
    for i, nblk in enumerate(need):
        seq_ids.append(rows - 1 - i)
        mine.append(perm[off:off + nblk])
        bt[seq_ids[-1], :nblk] = mine[-1].to(torch.int32)
        off += nblk
    k8, v8, k16, v16 = _two_pools((nb, L, KVH, 16, D), dtype, g)
    q = (torch.randn(sum(lens), H, D, generator=g) * 0.5).to(dtype)
    # the condition on the inputs, from the fp64 softmax on the stored values
    peaked = seen = 0
    off = 0
    for (c, n), blocks in zip(CROSS_FORMAT_CHUNKS, mine):
        if n == 0:
            continue
        pos = torch.arange(c + n)
        kd = R.dequantise(k8[blocks[pos // 16], layer, :, pos % 16])                 # [c + n, KVH, D] fp64
        s = scores64(q[off:off + n], kd, D ** -0.5)                                  # [n, H, c + n]
        vis = pos[None, :] <= torch.arange(n)[:, None] + c
        pmax = torch.softmax(s.masked_fill(~vis[:, None, :], float("-inf")), dim=-1).amax(-1)     # [n, H]
        wide = (vis.sum(-1) >= 8)[:, None].expand_as(pmax)
        seen += int(wide.sum())
        peaked += int((pmax[wide] >= 0.9).sum())
        off += n
    assert seen > 0 and 2 * peaked <= seen, f"{peaked} of {seen} rows with >= 8 keys are one-hot: the inputs decide nothing"
    st = C._state(ctxs, lens, D, torch.tensor(seq_ids, dtype=torch.int32))
    st.kv_scales = _scales(L, KVH, unit=True).cuda()
    mc, ec, qd, btd = NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=L), NS(block_size=16), q.cuda(), bt.cuda()
    outs = []
    for kc, vc in ((k8, v8), (k16, v16)):
        o = torch.full_like(qd, float("nan"))
        prefill_attention_paged(qd, kc.cuda(), vc.cuda(), btd, o, mc, ec, st, layer)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1]), "the output depends on the pool format"


# ---- f-h. the model -----------------------------------------------------------------------------------------------------------
def _engine_config(path, **kw):
    from swiftllm_amd import EngineConfig
    base = dict(model_path=path, use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                max_seqs_in_block_table=16, max_blocks_per_seq=32, max_batch_size=8, max_tokens_in_batch=1024)
    base.update(kw)
    return EngineConfig(**base)


def _make_model(path, cfg, sd, num_blocks=64, **kw):
    from oracle import synth
    from swiftllm_amd import LlamaModel
    synth.write_model_dir(str(path), cfg, sd)
    model = LlamaModel(_engine_config(str(path), **kw))
    model.load_weights()
    model.init_kvcache_and_swap(num_blocks)
    model.post_layer.logits_tap = []
    return model


def _fake_quant_oracle(monkeypatch, cfg, sd, tdtype, num_blocks=64, **ecfg):
    """oracle.ref_model.RefLlamaModel whose KV store writes dequant(quant(k)), dequant(quant(v)) (unit scales: exact in
    the 16-bit pool), so its decode attention reads what an FP8 pool holds. Nothing under oracle/ changes."""
    from oracle import eager_ops
    from oracle.ref_model import RefLlamaModel
    from swiftllm_amd import LlamaModelConfig
    real = eager_ops.store_kvcache

    def store(k, v, *rest, **kw):
        return real(R.fake_quant(k), R.fake_quant(v), *rest, **kw)
    monkeypatch.setattr(eager_ops, "store_kvcache", store)
    ref = RefLlamaModel(LlamaModelConfig(cfg), _engine_config("", **ecfg), sd, tdtype)
    ref.init_kvcache_and_swap(num_blocks)
    return ref


def _tol(dtype):
    return (2e-3, 2e-3) if dtype == "float16" else (1.6e-2, 1.6e-2)     # tests/test_gpu_model.py


def _excess(ours, theirs, rtol):
    return ((ours.float().cpu() - theirs).abs() - rtol * theirs.abs()).max().item()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_fp8_model_matches_fake_quant_oracle_graph_on_and_off(tmp_path, monkeypatch, dtype):
    """Prefill + 18 greedy decode steps (SMALL64: head_dim 64, GQA), FP8 pools, hipGraph replay and eager launches: bit-equal
    tokens and logits between the two, and both within the bar tests/test_gpu_model.py holds the 16-bit model to against
    the oracle (|dlogit| <= atol + rtol |logit|, identical greedy ids; teacher-forced with our tokens).
    Measured on MI355X: worst excess over rtol |logit| 1.4e-3 (float16, atol 2e-3) and 6.0e-3 (bfloat16, atol 1.6e-2);
    the piggybacked and chunked runs below: 1.0e-3 / 4.0e-3 and 1.4e-3 / 5.8e-3."""
    from oracle import synth
    cfg = synth.make_config(**synth.SMALL64)
    tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
    sd = synth.make_state_dict(cfg, seed=5, dtype=tdtype)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, cfg["vocab_size"], (n,), generator=g).tolist() for n in (1, 16, 17, 130, 65)]
    runs = {}
    for name, graph in (("graph", True), ("eager", False)):
        model = _make_model(tmp_path / name, cfg, sd, dtype=dtype, kv_cache_dtype="fp8_e4m3", use_hip_graph=graph)
        assert model.k_cache.dtype == FP8 and model.k_swap.dtype == FP8 and model.k_cache.element_size() == 1
        out = [model.forward(prompts, list(range(5)), [])]
        lens = [len(p) for p in prompts]
        for _ in range(18):
            lens = [n + 1 for n in lens]
            out.append(model.forward([[t] for t in out[-1]], list(range(5)), list(lens)))
        runs[name] = (out, [t.clone() for t in model.post_layer.logits_tap])
    assert runs["graph"][0] == runs["eager"][0]
    assert all(torch.equal(a, b) for a, b in zip(runs["graph"][1], runs["eager"][1]))
    got, taps = runs["graph"]
    ref = _fake_quant_oracle(monkeypatch, cfg, sd, tdtype, dtype=dtype)
    atol, rtol = _tol(dtype)
    want = [ref.forward(prompts, list(range(5)), [])]
    worst = _excess(taps[0], ref.last_logits, rtol)
    lens = [len(p) for p in prompts]
    for i in range(18):
        lens = [n + 1 for n in lens]
        want.append(ref.forward([[t] for t in got[i]], list(range(5)), list(lens)))
        worst = max(worst, _excess(taps[i + 1], ref.last_logits, rtol))
    print(f"\n[fp8 model {dtype}] worst logit excess over rtol |logit|: {worst:.3e} (atol {atol})")
    assert worst <= atol, worst
    assert got == want


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_fp8_model_piggybacked_step_matches_fake_quant_oracle(tmp_path, monkeypatch, dtype):
    """Two sequences decode while a new prompt rides along (two-stream path), then all three decode: FP8 pools against the
    fake-quant oracle, same bar."""
    from oracle import synth
    cfg = synth.make_config(**synth.SMALL64)
    tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
    sd = synth.make_state_dict(cfg, seed=9, dtype=tdtype)
    model = _make_model(tmp_path, cfg, sd, dtype=dtype, kv_cache_dtype="fp8_e4m3")
    ref = _fake_quant_oracle(monkeypatch, cfg, sd, tdtype, dtype=dtype)
    atol, rtol = _tol(dtype)
    g = torch.Generator().manual_seed(4)
    rp = lambda n: torch.randint(0, cfg["vocab_size"], (n,), generator=g).tolist()   # noqa: E731
    worst = [0.0]

    def both(ids, sids, dlens):
        a = model.forward(ids, sids, dlens)
        b = ref.forward(ids, sids, dlens)
        worst[0] = max(worst[0], _excess(model.post_layer.logits_tap[-1], ref.last_logits, rtol))
        assert a == b
        return a
    t = both([rp(40), rp(7)], [2, 5], [])
    lens = {2: 40, 5: 7}
    for _ in range(8):
        for s in lens:
            lens[s] += 1
        t = both([[t[0]], [t[1]]], [2, 5], [lens[2], lens[5]])
    for s in lens:
        lens[s] += 1
    t = both([rp(33), [t[0]], [t[1]]], [0, 2, 5], [lens[2], lens[5]])
    lens = {0: 33, 2: lens[2], 5: lens[5]}
    for _ in range(8):
        for s in lens:
            lens[s] += 1
        t = both([[x] for x in t], [0, 2, 5], [lens[0], lens[2], lens[5]])
    print(f"\n[fp8 model piggyback {dtype}] worst logit excess: {worst[0]:.3e} (atol {atol})")
    assert worst[0] <= atol, worst[0]


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_fp8_model_chunked_prefill_matches_fake_quant_oracle(tmp_path, monkeypatch, dtype):
    """A 100-token prompt fed as 40 + 40 + 20 (max_prefill_chunk = 40), then 16 decode steps. In FP8 mode a chunk attends
    to the QUANTISED pool, its own keys included, so the reference feeds the oracle the first chunk as a prompt (fresh
    keys, as ours) and every later prompt token as a one-token decode step (which attends to the fake-quantised cache,
    its own key included): same bar on the logits after the last prompt token and on every decode step."""
    from oracle import synth
    cfg = synth.make_config(**synth.SMALL64)
    tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
    sd = synth.make_state_dict(cfg, seed=11, dtype=tdtype)
    model = _make_model(tmp_path, cfg, sd, dtype=dtype, kv_cache_dtype="fp8_e4m3", max_prefill_chunk=40)
    ref = _fake_quant_oracle(monkeypatch, cfg, sd, tdtype, dtype=dtype)
    atol, rtol = _tol(dtype)
    g = torch.Generator().manual_seed(6)
    prompt = torch.randint(0, cfg["vocab_size"], (100,), generator=g).tolist()
    model.forward([prompt[:40]], [3], [], prefill_ctx_lens=[0])
    model.forward([prompt[40:80]], [3], [], prefill_ctx_lens=[40])
    tok = model.forward([prompt[80:]], [3], [], prefill_ctx_lens=[80])
    ref.forward([prompt[:40]], [3], [])
    for i in range(40, 100):
        rt = ref.forward([[prompt[i]]], [3], [i + 1])
    worst = _excess(model.post_layer.logits_tap[-1], ref.last_logits, rtol)
    assert tok == rt
    n = 100
    for _ in range(16):
        n += 1
        nxt = model.forward([[tok[0]]], [3], [n])
        rt = ref.forward([[tok[0]]], [3], [n])
        worst = max(worst, _excess(model.post_layer.logits_tap[-1], ref.last_logits, rtol))
        assert nxt == rt
        tok = nxt
    print(f"\n[fp8 model chunked {dtype}] worst logit excess: {worst:.3e} (atol {atol})")
    assert worst <= atol, worst


def test_fp8_swap_out_and_in_keeps_bytes_and_tokens(tmp_path):
    from oracle import synth
    cfg = synth.make_config(**synth.SMALL64)
    sd = synth.make_state_dict(cfg, seed=6)
    g = torch.Generator().manual_seed(8)
    pa = torch.randint(0, cfg["vocab_size"], (37,), generator=g).tolist()
    pb = torch.randint(0, cfg["vocab_size"], (60,), generator=g).tolist()

    def script(model, prompts, steps, sids):
        out = [model.forward(prompts, sids, [])]
        lens = [len(p) for p in prompts]
        for _ in range(steps):
            lens = [n + 1 for n in lens]
            out.append(model.forward([[t] for t in out[-1]], sids, list(lens)))
        return out
    clean = _make_model(tmp_path / "a", cfg, sd, 16, kv_cache_dtype="fp8_e4m3")
    want = [x[0] for x in script(clean, [pa], 8, [3])]
    model = _make_model(tmp_path / "b", cfg, sd, 16, kv_cache_dtype="fp8_e4m3")
    got = [x[0] for x in script(model, [pa], 3, [3])]
    torch.cuda.synchronize()
    ids = model.gpu_block_manager.get_block_ids_host(3)
    before = (model.k_cache.view(torch.uint8)[ids].cpu(), model.v_cache.view(torch.uint8)[ids].cpu())
    model.swap_out_seqs([3])
    assert model.gpu_block_manager.num_free_blocks == 16 and model.cpu_block_manager.num_free_blocks == 8 - 3
    script(model, [pb], 2, [1])                         # tramples the freed GPU blocks
    model.swap_in_seqs([3])
    torch.cuda.synchronize()
    ids2 = model.gpu_block_manager.get_block_ids_host(3)
    assert torch.equal(model.k_cache.view(torch.uint8)[ids2].cpu(), before[0])
    assert torch.equal(model.v_cache.view(torch.uint8)[ids2].cpu(), before[1])
    n, last = len(pa) + 3, got[-1]
    for _ in range(5):
        n += 1
        last = model.forward([[last]], [3], [n])[0]
        got.append(last)
    assert got == want
    with pytest.raises(RuntimeError):
        model.set_kv_scales(torch.ones(cfg["num_hidden_layers"], cfg["num_key_value_heads"]),
                            torch.ones(cfg["num_hidden_layers"], cfg["num_key_value_heads"]))
    model.free_seqs_resources([1, 3])
    model.set_kv_scales(torch.full((cfg["num_hidden_layers"], cfg["num_key_value_heads"]), 0.75),
                        torch.full((cfg["num_hidden_layers"], cfg["num_key_value_heads"]), 1.5))
    assert torch.equal(model.kv_inv_scales.cpu()[0], 1.0 / torch.full_like(model.kv_scales.cpu()[0], 0.75))
    toks = model.forward([pa], [3], [])
    assert len(toks) == 1


def test_fp8_pool_holds_about_twice_the_blocks(tmp_path):
    """profile_num_blocks on the same model and budget: the FP8 count is between 1.9x and 2.0x the 16-bit one once the
    block tables and the hipGraph reserve — which do not shrink — are accounted for, i.e. the two budgets in BYTES agree
    to within that: n8 * block_bytes8 vs n16 * block_bytes16."""
    from oracle import synth
    from swiftllm_amd import LlamaModel
    cfg = synth.make_config(**synth.SMALL128)
    synth.write_model_dir(str(tmp_path), cfg)
    counts = {}
    for kvd in ("auto", "fp8_e4m3"):
        model = LlamaModel(_engine_config(str(tmp_path), use_dummy=True, gpu_mem_utilization=0.5, max_batch_size=4,
                                          max_tokens_in_batch=512, dtype="bfloat16", kv_cache_dtype=kvd))
        model.load_weights()
        counts[kvd] = model.profile_num_blocks()
        del model
        torch.cuda.empty_cache()
    ratio = counts["fp8_e4m3"] / counts["auto"]
    print(f"\n[fp8 capacity] blocks: 16-bit {counts['auto']}, fp8 {counts['fp8_e4m3']} ({ratio:.4f}x)")
    assert 1.9 <= ratio <= 2.0 + 1e-3, counts


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_auto_leaves_the_16_bit_path_untouched(tmp_path, dtype):
    from oracle import synth
    cfg = synth.make_config(**synth.SMALL64)
    tdtype = torch.float16 if dtype == "float16" else torch.bfloat16
    sd = synth.make_state_dict(cfg, seed=5, dtype=tdtype)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, cfg["vocab_size"], (n,), generator=g).tolist() for n in (9, 40)]
    res = []
    for name, kw in (("plain", {}), ("auto", dict(kv_cache_dtype="auto"))):
        model = _make_model(tmp_path / name, cfg, sd, dtype=dtype, **kw)
        assert model.k_cache.dtype == tdtype and model.k_swap.dtype == tdtype and model.kv_scales is None
        t = model.forward(prompts, [0, 1], [])
        t2 = model.forward([[x] for x in t], [0, 1], [10, 41])
        res.append((t, t2, [x.clone() for x in model.post_layer.logits_tap]))
    assert res[0][:2] == res[1][:2]
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
