"""tests/_families_ref.qk_prep_ref — the fp64 restatement of swl_qk_prep_rotary's contract — against HuggingFace's own
modules on fp32 inputs: Qwen3RMSNorm + apply_rotary_pos_emb (Qwen3), x + bias -> apply_rotary_pos_emb (Qwen2). Agreement to
fp32 noise ties the kernel's contract to the reference implementation before any GPU is involved."""
import pytest
import torch

from _families_ref import qk_prep_ref, ulp_of

T, H, KVH = 9, 4, 2


def _case(D, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    q, k, v = rnd(T, H, D), rnd(T, KVH, D), rnd(T, KVH, D)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    freqs = torch.outer(torch.arange(64, dtype=torch.float32), inv)
    pos = torch.randint(0, 64, (T,), generator=g)
    return q, k, v, torch.cos(freqs), torch.sin(freqs), pos, rnd


def _hf_rotary(q, k, cos, sin, pos):
    from transformers.models.qwen3.modeling_qwen3 import apply_rotary_pos_emb
    c, s = torch.cat((cos[pos], cos[pos]), -1)[None], torch.cat((sin[pos], sin[pos]), -1)[None]     # [1, T, D]
    qo, ko = apply_rotary_pos_emb(q.transpose(0, 1)[None], k.transpose(0, 1)[None], c, s)           # [1, heads, T, D]
    return qo[0].transpose(0, 1), ko[0].transpose(0, 1)


@pytest.mark.parametrize("D", [32, 128])
def test_qwen3_norm_then_rotary_is_the_contract(D):
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm
    q, k, v, cos, sin, pos, rnd = _case(D, D)
    eps = 1e-6
    qn, kn = Qwen3RMSNorm(D, eps=eps), Qwen3RMSNorm(D, eps=eps)
    with torch.no_grad():
        qn.weight.copy_(1 + 0.2 * rnd(D))
        kn.weight.copy_(1 + 0.2 * rnd(D))
        want_q, want_k = _hf_rotary(qn(q), kn(k), cos, sin, pos)
    got = qk_prep_ref(q, k, v, cos, sin, pos.int(), q_norm=qn.weight.detach(), k_norm=kn.weight.detach(), eps=eps)
    for name, want in (("q", want_q), ("k", want_k)):
        err = (got[name] - want.double()).abs()
        assert bool((err <= 2.0 ** -20 * got[name + "_mag"] + 1e-30).all()), (name, err.max().item())
    assert torch.equal(got["v"], v.double())


@pytest.mark.parametrize("D", [32, 128])
def test_qwen2_bias_then_rotary_is_the_contract(D):
    q, k, v, cos, sin, pos, rnd = _case(D, 100 + D)
    qb, kb, vb = 0.5 * rnd(H * D), 0.5 * rnd(KVH * D), 0.5 * rnd(KVH * D)
    want_q, want_k = _hf_rotary(q + qb.view(H, D), k + kb.view(KVH, D), cos, sin, pos)
    got = qk_prep_ref(q, k, v, cos, sin, pos.int(), q_bias=qb, k_bias=kb, v_bias=vb)
    for name, want in (("q", want_q), ("k", want_k)):
        err = (got[name] - want.double()).abs()
        assert bool((err <= 2.0 ** -20 * got[name + "_mag"] + 1e-30).all()), (name, err.max().item())
    assert torch.equal(got["v"], v.double() + vb.double().view(KVH, D))


def test_inert_rows_null_positions_and_the_ulp_helper():
    q, k, v, cos, sin, pos, rnd = _case(32, 7)
    pos = pos.int()
    pos[2] = pos[5] = -1
    w = 1 + 0.2 * rnd(32)
    got = qk_prep_ref(q, k, v, cos, sin, pos, v_bias=rnd(KVH * 32), q_norm=w, k_norm=w, eps=1e-6)
    for r in (2, 5):
        assert torch.equal(got["q"][r], q[r].double()) and torch.equal(got["k"][r], k[r].double())
        assert torch.equal(got["v"][r], v[r].double())
    assert got["live"].tolist() == [i not in (2, 5) for i in range(T)]
    # pos_idx None: row t
    a = qk_prep_ref(q, k, None, cos, sin, None)
    b = qk_prep_ref(q, k, None, cos, sin, torch.arange(T, dtype=torch.int32))
    assert torch.equal(a["q"], b["q"]) and torch.equal(a["k"], b["k"]) and a["v"] is None
    y = torch.tensor([1.0, 1.5, 2.0, 0.0, 1e-9, 65504.0], dtype=torch.float64)
    assert ulp_of(y, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 32.0]
    assert ulp_of(y, torch.bfloat16)[:3].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    assert ulp_of(torch.tensor([0.0], dtype=torch.float64), torch.bfloat16).item() == 2.0 ** -133
