"""The attention case builders and the fp64 reference of tests/_attn_cases.py, on the CPU: the reference agrees with
the oracle, and each builder yields the profile it claims on the ROUNDED tensors (what the kernels read)."""
import types

import pytest
import torch

from oracle import eager_ops as ops
from _attn_cases import LOG2E, attn64, make_kv, make_q, rise_per_tile, scores64

NS = types.SimpleNamespace
DTYPES = [torch.float16, torch.bfloat16]


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attn64_matches_oracle_paged_attention(dtype):
    g = gen(1)
    H, KVH, D, n = 8, 2, 64, 100
    q = torch.randn(1, H, D, generator=g).to(dtype)
    k = torch.randn(n, KVH, D, generator=g).to(dtype)
    v = torch.randn(n, KVH, D, generator=g).to(dtype)
    kc = torch.zeros(-(-n // 16), 1, KVH, 16, D, dtype=dtype)
    vc = torch.zeros_like(kc)
    for j in range(n):
        kc[j // 16, 0, :, j % 16] = k[j]
        vc[j // 16, 0, :, j % 16] = v[j]
    bt = torch.arange(kc.shape[0], dtype=torch.int32).view(1, -1)
    st = NS(num_decoding_seqs=1, num_prefill_seqs=0, seq_block_size=64, num_seq_blocks=2, softmax_scale=D ** -0.5,
            decoding_seq_lens=torch.tensor([n], dtype=torch.int32), seq_ids=torch.tensor([0], dtype=torch.int32))
    eo = torch.zeros_like(q)
    ops.paged_attention(q, kc, vc, bt, NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D, num_layers=1),
                        NS(block_size=16), st, 0, eo)
    ref = attn64(q, k, v, D ** -0.5)
    tol = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7      # one rounding of an output below 1
    assert (eo.double() - ref["o"]).abs().max().item() <= tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_attn64_matches_oracle_prefill_attention(dtype):
    g = gen(2)
    H, KVH, D, T = 4, 2, 32, 70
    q = torch.randn(T, H, D, generator=g).to(dtype)
    k = torch.randn(T, KVH, D, generator=g).to(dtype)
    v = torch.randn(T, KVH, D, generator=g).to(dtype)
    eo = torch.zeros_like(q)
    cu = torch.tensor([0, T], dtype=torch.int32)
    ops.prefill_attention(q, k, v, eo, NS(num_q_heads=H, num_kv_heads=KVH, head_dim=D), None,
                          NS(num_prefill_seqs=1, max_prefill_len=T, softmax_scale=D ** -0.5,
                             prefill_seq_start_locs_with_end=cu, num_prefill_tokens=T))
    ref = attn64(q, k, v, D ** -0.5, causal=True)
    tol = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    assert (eo.double() - ref["o"]).abs().max().item() <= tol
    # row 0 sees only key 0
    assert torch.allclose(ref["o"][0], v[0].double().repeat_interleave(H // KVH, 0))


def test_attn64_splits_merge_to_the_whole():
    """The per-split outputs / base-2 LSEs merge back to the one-pass result; the LSE is log2 sum 2^(s log2 e)."""
    g = gen(3)
    q = torch.randn(1, 4, 32, generator=g).half()
    k = torch.randn(150, 2, 32, generator=g).half()
    v = torch.randn(150, 2, 32, generator=g).half()
    r = attn64(q, k, v, 32 ** -0.5, split=64)
    assert r["o_s"].shape == (1, 4, 3, 32) and r["lse2_s"].shape == (1, 4, 3)
    w = torch.exp2(r["lse2_s"] - r["lse2"][..., None])
    assert torch.allclose(w.sum(-1), torch.ones(1, 4, dtype=torch.float64))
    assert torch.allclose((w[..., None] * r["o_s"]).sum(2), r["o"])
    s = scores64(q, k, 32 ** -0.5)
    assert torch.allclose(r["lse2"], torch.logsumexp(s, -1) * LOG2E)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 128])
def test_needle_sink_and_tie_profiles_hold_after_rounding(dtype, D):
    g = gen(D)
    n, KVH, H = 300, 2, 6
    needles = [[17, 255], [0, 0]]
    ties = [[(5, 200), (40, 41)]]
    k, v, F = make_kv(n, KVH, D, dtype, g, needles=needles, ties=ties)
    specs = [{"kind": "needle", "i": 0, "delta": 40.0}, {"kind": "needle", "i": 0, "delta": 12.0},
             {"kind": "needle", "i": 1, "delta": 40.0}, {"kind": "tie", "i": 2, "delta": 40.0},
             {"kind": "flat"}, {"kind": "needle", "i": 0, "delta": 40.0, "shift": -600.0}]
    q = make_q(1, H, D, F, dtype, g, specs, D ** -0.5)
    s = scores64(q, k, D ** -0.5)[0]                           # [H, n]
    G = H // KVH
    for h, spec in enumerate(specs):
        kvh = h // G
        top = s[h].topk(3)
        if spec["kind"] == "needle":
            pos = needles[spec["i"]][kvh]
            assert int(top.indices[0]) == pos
            # margin: the nominal one, less the noise scores (|noise| < 2.5 nats here)
            assert (top.values[0] - top.values[1]).item() >= spec["delta"] - 5.0
        elif spec["kind"] == "tie":
            a, b = ties[0][kvh]
            assert sorted(top.indices[:2].tolist()) == [a, b]
            assert torch.equal(k[a, kvh], k[b, kvh])            # the tie bits
            assert top.values[0] == top.values[1]
            assert (top.values[0] - top.values[2]).item() >= 35.0
        else:
            assert torch.equal(s[h], torch.zeros(n, dtype=torch.float64))
    # the shift moves every score by ~-600 nats and keeps the needle's margin
    assert abs(s[5].max().item() - (40.0 - 600.0)) < 5.0
    assert (s[5].topk(2).values[0] - s[5].topk(2).values[1]).item() >= 35.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_ramps_rise_on_every_tile_and_fall_below_fp32_range(dtype):
    """Rising ramp (prefill spec): the running maximum rises by >= 5 log2 units on every 64-key tile (more than
    kLazyMax = 4: a lazy raise every tile) and the masked future keys of a row hold larger scores than its visible ones.
    Falling ramp: 64-key splits after the first sit > 150 log2 units below it (their weight underflows fp32's exp2)."""
    g = gen(5)
    n, D = 1024, 128
    k, v, F = make_kv(n, 1, D, dtype, g)
    rise = {"kind": "ramp", "slope": 7.5 / (64 * LOG2E)}
    fall = {"kind": "ramp", "slope": -2.0}
    q = make_q(1, 2, D, F, dtype, g, [rise, fall], D ** -0.5)
    s = scores64(q, k, D ** -0.5)[0]
    r = rise_per_tile(s[0])
    assert r.min().item() >= 5.0
    row = 300                                                  # a row of a causal prefill: keys > 300 are masked
    assert s[0, row + 1:].max() > s[0, :row + 1].max()
    lse2 = torch.stack([torch.logsumexp(s[1, j:j + 64], -1) * LOG2E for j in range(0, n, 64)])
    assert (lse2[0] - lse2[1:]).min().item() > 150.0


def test_flat_and_shifted_flat_give_the_mean_of_v():
    g = gen(6)
    n, D = 4096, 64
    k, v, F = make_kv(n, 1, D, torch.float16, g)
    q = make_q(1, 2, D, F, torch.float16, g, [{"kind": "flat"}, {"kind": "flat", "shift": 600.0}], D ** -0.5)
    s = scores64(q, k, D ** -0.5)[0]
    assert torch.equal(s[0], torch.zeros(n, dtype=torch.float64))
    assert (s[1] == s[1, 0]).all() and abs(s[1, 0].item() - 600.0) < 1.0
    r = attn64(q, k, v, D ** -0.5)
    mean = v.double().mean(0)[0]
    assert torch.allclose(r["o"][0, 0], mean) and torch.allclose(r["o"][0, 1], mean)


def test_seq_block_size_gives_more_than_16_splits_at_1k_to_2k_tokens():
    """Why the n > 16 branch of the tiny-batch o_proj merge matters: at Llama-3-8B geometry (8 kv heads) one sequence
    of 1 025 to 2 048 tokens is split into 64-token blocks, 17 to 32 of them."""
    from swiftllm_amd.worker.batch_plan import select_seq_block_size
    assert select_seq_block_size([1024], 8) == 64 and -(-1024 // 64) == 16
    for ctx in (1025, 1100, 1536, 2000, 2048):
        sbs = select_seq_block_size([ctx], 8)
        assert sbs == 64 and -(-ctx // sbs) > 16, (ctx, sbs)
    assert -(-2048 // select_seq_block_size([2048], 8)) == 32
