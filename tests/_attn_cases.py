"""Attention inputs with designed score profiles, and an fp64 softmax to hold the kernels to
(tests/test_attn_cases.py checks both on the CPU; tests/test_gpu_attention_extremes.py uses them on the GPU).

On torch.randn data the scores are ~N(0, 1) nats: the softmax is nearly flat and a row's maximum hardly moves after its
first tile, so a missing rescale, a maximum taken before the causal mask or an overflowing P cancel or stay in range.
The builders here place the profiles of real checkpoints (sinks, needles, ramps, ties, huge shifts) into FEATURE
columns, the last F of the D channels:

    K[j, h, D - F + f] = feature_f(j, h)          q[.., D - F + f] = w_f (per q head, per sequence)

and fill the other channels with small noise (sigma 0.5 on both sides: noise scores ~0.25 nats). The score of key j is
then scale * (sum_f w_f * feature_f(j) + noise), so every q head of one GQA group can carry its own profile in the
same launch (one matrix-core wave holds the heads of one group). Features:

    RAMP   j / 64                 rising (w > 0) or falling (w < 0) scores along the keys
    CONST  1                      shifts every score of a row by w nats / scale (the "shifted" cases)
    NEEDLE_i   1 at one key per kv head (or at two keys for a tie), 0 elsewhere

The profile is only nominal after rounding to the storage dtype: the reference is always computed on the STORED
values (attn64 casts what the kernel reads), and the CPU tests check the claimed margins / rises / tie bits on them.
"""
import math

import torch

LOG2E = 1.0 / math.log(2.0)
RAMP, CONST = 0, 1          # feature indices; needles follow
N_FIXED = 2
SIGMA = 0.5
# keys whose weight is below e^-RELEVANT of the row maximum contribute < n e^-30 of the output: their score errors
# cannot show, so the score term of a bound is sized by the keys above it only
RELEVANT = 30.0


def f32(x: float) -> float:
    """The value the kernel receives for a float argument (softmax_scale is passed as a C float)."""
    return float(torch.tensor(x, dtype=torch.float32))


def unit_roundoff(dtype) -> float:
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of the 16-bit `dtype` at |x| (its subnormal spacing below the normal range)."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(x.double().abs().clamp(min=2.0 ** emin)))
    return torch.exp2(e - mant)


def attn64(q, K, V, scale, causal=False, split=None):
    """fp64 softmax attention over the stored values.

    q [T, H, D], K / V [n, KVH, D] in their storage dtype; `scale` is rounded to fp32 first (what the kernel gets).
    Row t sees keys j <= t + (n - T) when `causal` (prefill: T == n; decode: T == 1 sees all n keys).
    Returns a dict:
      o     [T, H, D]   the output
      lse2  [T, H]      log2(sum_j 2^(s_j * scale * log2 e)), the base-2 scaled domain of the kernels' mid_lse
      smag  [T, H]      scale * max_j sum_d |q_d k_jd| over the keys within RELEVANT nats of the row maximum, in nats:
                        the magnitude the fp32 score error of the kernel is relative to
      smax  [T, H]      the row maximum score (nats)
    With `split` (tokens per split): also o_s [T, H, nsplit, D], lse2_s [T, H, nsplit] (-inf for splits without a
    visible key) and smag_s [T, H, nsplit] for the flash-decoding partials.
    """
    T, H, D = q.shape
    n, KVH, _ = K.shape
    G = H // KVH
    sc = f32(scale)
    qd, kd, vd = q.double(), K.double(), V.double()
    s = torch.einsum("thd,nhd->thn", qd, kd.repeat_interleave(G, dim=1)) * sc
    sa = torch.einsum("thd,nhd->thn", qd.abs(), kd.abs().repeat_interleave(G, dim=1)) * sc
    vis = torch.ones(T, 1, n, dtype=torch.bool)
    if causal:
        vis = (torch.arange(n)[None, :] <= torch.arange(T)[:, None] + (n - T))[:, None, :]
    s = s.masked_fill(~vis, float("-inf"))
    vr = vd.repeat_interleave(G, dim=1)               # [n, H, D]

    def softmax(s_, sa_, vr_):
        m = s_.amax(-1, keepdim=True)
        ok = torch.isfinite(m)
        msafe = torch.where(ok, m, torch.zeros_like(m))
        p = torch.exp(s_ - msafe)
        l = p.sum(-1, keepdim=True)
        o = torch.einsum("thn,nhd->thd", p, vr_) / l.clamp(min=1e-300)
        lse2 = torch.where(ok, (torch.log(l) + msafe) * LOG2E, torch.full_like(m, float("-inf"))).squeeze(-1)
        rel = s_ >= msafe - RELEVANT
        smag = torch.where(rel, sa_, torch.zeros_like(sa_)).amax(-1)
        return o, lse2, smag, m.squeeze(-1)

    o, lse2, smag, smax = softmax(s, sa, vr)
    out = dict(o=o, lse2=lse2, smag=smag, smax=smax)
    if split:
        ns = -(-n // split)
        os_, ls_, ms_ = [], [], []
        for k0 in range(0, n, split):   # one dense softmax per split
            o_k, l_k, m_k, _ = softmax(s[..., k0:k0 + split], sa[..., k0:k0 + split], vr[k0:k0 + split])
            os_.append(o_k)
            ls_.append(l_k)
            ms_.append(m_k)
        out.update(o_s=torch.stack(os_, 2), lse2_s=torch.stack(ls_, 2), smag_s=torch.stack(ms_, 2))
        assert out["o_s"].shape[2] == ns
    return out


# ---- builders --------------------------------------------------------------------------------------------------------
def make_kv(n, KVH, D, dtype, g, needles=(), ties=()):
    """K, V [n, KVH, D] in `dtype` with the feature columns (module docstring) in the last F channels.

    needles: per needle feature, a list of KVH key positions (one per kv head; None = no needle for that head).
    ties:    per tie feature, a list of KVH pairs (a, b): K[b] is made a bit-identical copy of K[a] (the whole row: the
             tie is exact whatever the q), and feature value 1 marks both.
    Returns K, V, F (feature count)."""
    F = N_FIXED + len(needles) + len(ties)
    assert D - F >= 16, "too many features for the head dim"
    K = torch.randn(n, KVH, D, generator=g) * SIGMA
    V = torch.randn(n, KVH, D, generator=g)
    c0 = D - F
    K[:, :, c0:] = 0.0
    K[:, :, c0 + RAMP] = (torch.arange(n, dtype=torch.float32) / 64.0)[:, None]
    K[:, :, c0 + CONST] = 1.0
    for i, pos in enumerate(needles):
        for h, j in enumerate(pos):
            if j is not None:
                K[j, h, c0 + N_FIXED + i] = 1.0
    K = K.to(dtype)
    for i, pairs in enumerate(ties):
        f = c0 + N_FIXED + len(needles) + i
        for h, ab in enumerate(pairs):
            if ab is None:
                continue
            a, b = ab
            K[a, h, f] = 1.0
            K[b, h] = K[a, h]
    return K, V.to(dtype), F


def make_q(T, H, D, F, dtype, g, specs, scale, shifts=None):
    """q [T, H, D]: q head h carries the profile specs[h], a dict (score in nats per unit of feature):
      {"kind": "flat"}                       q = 0: every score 0 (or exactly the shift)
      {"kind": "needle", "i": i, "delta": d} needle feature i scores +d nats
      {"kind": "tie", "i": i, "delta": d}    the same for a tie feature: i counts the needles first (the first tie of
                                             make_kv(needles=[a, b], ties=[..]) is feature i = 2)
      {"kind": "ramp", "slope": s}           s nats per key (negative: falling)
    plus an optional "shift": extra nats on every score of the head through the constant column. `shifts` (one per
    row of q, or one value) adds to every head: a decode batch anchors each sequence's ramp at ~0 nats with it."""
    q = torch.randn(T, H, D, generator=g) * SIGMA
    q[:, :, D - F:] = 0.0
    sc = f32(scale)
    for h, spec in enumerate(specs):
        kind = spec["kind"]
        if kind == "flat":
            q[:, h, :] = 0.0
        elif kind == "needle":
            q[:, h, D - F + N_FIXED + spec["i"]] = spec["delta"] / sc
        elif kind == "tie":
            q[:, h, D - F + N_FIXED + spec["i"]] = spec["delta"] / sc
        elif kind == "ramp":
            q[:, h, D - F + RAMP] = spec["slope"] * 64.0 / sc
        else:
            raise ValueError(spec)
        q[:, h, D - F + CONST] = spec.get("shift", 0.0) / sc
    if shifts is not None:
        sh = torch.as_tensor(shifts, dtype=torch.float32).reshape(-1, 1)
        q[:, :, D - F + CONST] += sh / sc
    return q.to(dtype)


def rise_per_tile(scores_row: torch.Tensor, tile: int = 64) -> torch.Tensor:
    """Increase of the running maximum (log2 units) at each tile after the first, for one row of nats."""
    x = scores_row * LOG2E
    n = x.shape[-1]
    tmax = torch.stack([x[..., k:k + tile].amax(-1) for k in range(0, n, tile)], -1)
    run = torch.cummax(tmax, -1).values
    return run[..., 1:] - run[..., :-1]


def scores64(q, K, scale):
    """scale * q.k in fp64 over the stored values: [T, H, n] nats (no mask)."""
    T, H, D = q.shape
    G = H // K.shape[1]
    return torch.einsum("thd,nhd->thn", q.double(), K.double().repeat_interleave(G, dim=1)) * f32(scale)
