"""The three forms of the decode-side rotary + KV store, held to one another at entry level on a padded batch:

  a. swl_rotary, then swl_store_kv_decode
  b. swl_rotary_store_kv_decode
  c. swl_splitk_rotary_store_kv_decode, fed one fp32 slab that holds exactly the 16-bit values

leave bit-equal q, k, v and pools; the pools equal the indexed closed form (the rotated k / the v of sequence i at slot
(len - 1) % 16 of block table[id][(len - 1) / 16], layer 1 of 2), every other slot keeps its sentinel, and the row of
length 0 — an inert row of a padded batch — changes nothing of q, k or the pools.

And the FP8 prefill store with ctx_lens == NULL against an all-zero ctx_lens, byte for byte."""
import pytest
import torch

from swiftllm_amd import _hip

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
SHAPES = [(4, 2, 32),        # the smallest head: two chunks per half
          (4, 2, 128),
          (32, 8, 128)]      # 448 items: two workgroups per token
BS, L, LAYER, MBPS, NB = 16, 2, 1, 4, 12
LENS = [1, 16, 17, 0, 33]    # 0: a padded row
SEQ_IDS = [3, 0, 5, 2, 1]
SENTINEL = 7.0


def _bits(t):
    return t.cpu().view(torch.int16)


def _block_table(lens):
    """Distinct blocks for the blocks each sequence needs, NB - 1 (written by nobody) everywhere else."""
    bt = torch.full((8, MBPS), NB - 1, dtype=torch.int32)
    free = [9, 2, 7, 0, 5, 10, 3, 8, 1, 6, 4]                  # scattered, all < NB - 1
    for sid, n in zip(SEQ_IDS, lens):
        need = -(-n // BS)
        bt[sid, :need] = torch.tensor([free.pop() for _ in range(need)], dtype=torch.int32)
    return bt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D", SHAPES)
def test_decode_store_forms_agree_and_equal_the_closed_form(dtype, H, KVH, D):
    g = torch.Generator().manual_seed(H * 1000 + D)
    B, n = len(LENS), (H + 2 * KVH) * D
    qkv = torch.randn(B, n, generator=g).to(dtype)
    ang = torch.rand(64, D // 2, generator=g) * 6.28
    cos, sin = torch.cos(ang).to(dtype).cuda(), torch.sin(ang).to(dtype).cuda()
    lens = torch.tensor(LENS, dtype=torch.int32).cuda()
    pos = (lens - 1).contiguous()                              # -1 on the padded row
    ids = torch.tensor(SEQ_IDS, dtype=torch.int32).cuda()
    bt = _block_table(LENS)
    btd = bt.cuda()
    shape = (NB, L, KVH, BS, D)
    code, stream = _hip.dtype_code(dtype), _hip.stream()
    P = _hip.ptr

    def fresh():
        buf = qkv.clone().cuda()
        q, k, v = buf[:, :H * D], buf[:, H * D:(H + KVH) * D], buf[:, (H + KVH) * D:]
        kc, vc = torch.full(shape, SENTINEL, dtype=dtype).cuda(), torch.full(shape, SENTINEL, dtype=dtype).cuda()
        return buf, q, k, v, kc, vc

    out = []
    # a. two launches
    buf, q, k, v, kc, vc = fresh()
    _hip.call("swl_rotary", P(q), P(k), P(cos), P(sin), P(pos), B, H, KVH, D, n, n, code, stream)
    _hip.call("swl_store_kv_decode", P(kc), P(vc), P(k), P(v), P(btd), P(ids), P(lens), B, LAYER, L, KVH, BS, D, MBPS, n, n,
              code, stream)
    out.append((buf, kc, vc))
    # b. fused
    buf, q, k, v, kc, vc = fresh()
    _hip.call("swl_rotary_store_kv_decode", P(q), P(k), P(v), P(cos), P(sin), P(pos), P(kc), P(vc), P(btd), P(ids), P(lens),
              B, H, KVH, D, LAYER, L, BS, MBPS, n, n, n, code, stream)
    out.append((buf, kc, vc))
    # c. slab-fed: q, k, v are outputs; the padded row of them is not written, so they start as the inputs too
    buf, q, k, v, kc, vc = fresh()
    slab = qkv.float().cuda().contiguous()
    assert torch.equal(slab.to(dtype).cpu(), qkv)
    _hip.call("swl_splitk_rotary_store_kv_decode", P(q), P(k), P(v), P(slab), 1, P(cos), P(sin), P(pos), P(kc), P(vc), P(btd),
              P(ids), P(lens), B, H, KVH, D, LAYER, L, BS, MBPS, n, n, n, code, stream)
    out.append((buf, kc, vc))
    torch.cuda.synchronize()

    (buf_a, kc_a, vc_a), rest = out[0], out[1:]
    for name, (buf_x, kc_x, vc_x) in zip(("fused", "slab-fed"), rest):
        assert torch.equal(_bits(buf_a), _bits(buf_x)), f"{name}: q, k or v differ from rotary + store"
        assert torch.equal(_bits(kc_a), _bits(kc_x)) and torch.equal(_bits(vc_a), _bits(vc_x)), f"{name}: the pools differ"

    # the closed form, sentinels included. It indexes the k that form (a) rotated: what is held here is WHERE each row lands
    # and that the forms agree; the rotation's arithmetic is held to the reference in test_gpu_kernels.py.
    got = buf_a.cpu()
    k_rot, v_in = got[:, H * D:(H + KVH) * D].view(B, KVH, D), got[:, (H + KVH) * D:].view(B, KVH, D)
    ek, ev = torch.full(shape, SENTINEL, dtype=dtype), torch.full(shape, SENTINEL, dtype=dtype)
    for i, (sid, ln) in enumerate(zip(SEQ_IDS, LENS)):
        if ln > 0:
            blk = int(bt[sid, (ln - 1) // BS])
            ek[blk, LAYER, :, (ln - 1) % BS] = k_rot[i]
            ev[blk, LAYER, :, (ln - 1) % BS] = v_in[i]
    assert torch.equal(_bits(kc_a), _bits(ek)) and torch.equal(_bits(vc_a), _bits(ev))
    # the padded row is untouched, every other row of q and k is rotated, v never changes
    pad = LENS.index(0)
    assert torch.equal(_bits(got[pad]), _bits(qkv[pad]))
    live = [i for i, ln in enumerate(LENS) if ln > 1]          # position 0 has angle row 0: any angle, still a rotation
    assert all(not torch.equal(_bits(got[i, :(H + KVH) * D]), _bits(qkv[i, :(H + KVH) * D])) for i in live)
    assert torch.equal(_bits(got[:, (H + KVH) * D:]), _bits(qkv[:, (H + KVH) * D:]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KVH,D", SHAPES)
def test_fp8_prefill_store_null_contexts_equal_zero_contexts(dtype, H, KVH, D):
    g = torch.Generator().manual_seed(KVH * 100 + D)
    plens = [n for n in LENS if n > 0]
    sids = [s for s, n in zip(SEQ_IDS, LENS) if n > 0]
    T, n = sum(plens), (H + 2 * KVH) * D
    qkv = (torch.randn(T, n, generator=g) * 4).to(dtype).cuda()
    k, v = qkv[:, H * D:(H + KVH) * D], qkv[:, (H + KVH) * D:]
    inv = (0.5 + torch.rand(2, L, KVH, generator=g)).cuda()
    btd = _block_table(LENS).cuda()
    ids = torch.tensor(sids, dtype=torch.int32).cuda()
    lens = torch.tensor(plens, dtype=torch.int32).cuda()
    starts = (torch.cumsum(lens, 0) - lens).to(torch.int32).contiguous()
    zeros = torch.zeros(len(plens), dtype=torch.int32).cuda()
    shape = (NB, L, KVH, BS, D)
    pools = []
    for ctx in (None, zeros):
        kc, vc = torch.full(shape, 0x5a, dtype=torch.uint8).cuda(), torch.full(shape, 0x5a, dtype=torch.uint8).cuda()
        _hip.call("swl_store_kv_prefill_at_fp8", _hip.ptr(kc), _hip.ptr(vc), _hip.ptr(k), _hip.ptr(v), _hip.ptr(inv),
                  _hip.ptr(btd), _hip.ptr(ids), _hip.ptr(starts), _hip.ptr(lens), _hip.ptr(ctx), len(plens), max(plens),
                  LAYER, L, KVH, BS, D, MBPS, n, n, _hip.dtype_code(dtype), _hip.stream())
        pools.append((kc.cpu(), vc.cpu()))
    (k0, v0), (k1, v1) = pools
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    assert (k0 != 0x5a).any() and (v0 != 0x5a).any()
    assert (k0[:, 0] == 0x5a).all() and (v0[NB - 1] == 0x5a).all()       # the other layer, the block nobody owns
