"""swl_kv_copy_blocks (csrc/kv_copy.hip) on the GPU: one launch copies whole KV blocks inside both pools.

The kernel moves bytes, so the pools here are uint8 tensors of random bytes and every comparison is on integers over the
WHOLE pool — blocks the call must not touch are checked with the ones it must write. The expectation is a copy applied
from the host on a clone of the pool (torch index assignment, valid pairs only).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

MIB = 1 << 20
# 512 = L1 . KVH1 . 16 . D32 . 1 byte, the smallest FP8 block (a quarter of one wave's 16-byte lanes);
# 30720 = L3 . KVH5 . 16 . D64 . 2 bytes, no power of two (one 16 KiB slice and a partial one); 1 MiB = Llama-3-8B bf16
BLOCK_BYTES = [512, 30720, MIB]
NUM_BLOCKS = 640


def _hip():
    from swiftllm_amd import _hip
    return _hip


def _pools(num_blocks, block_bytes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = torch.randint(0, 256, (num_blocks, block_bytes), dtype=torch.uint8, device="cuda", generator=g)
    v = torch.randint(0, 256, (num_blocks, block_bytes), dtype=torch.uint8, device="cuda", generator=g)
    return k, v


def _pairs(n, nb):
    """(src ids, dst ids) of n pairs in a pool of nb blocks. The distinct valid destinations are disjoint from the sources.
    n = 300: 100 pairs with descending ids, 190 scattered ones (sources and destinations interleave in the pool), and in
    the middle of them: a pair with src == dst, three pairs with an id outside the pool (their neighbours must be copied),
    the highest block as a source, the lowest as a destination, and five sources copied a second time."""
    if n == 0:
        return [], []
    if n == 1:
        return [nb - 1], [0]                    # the highest block of the pool, as a source
    if n == 2:
        return [1, nb - 2], [nb - 1, 0]         # ... and as a destination; descending destinations
    assert n == 300 and nb >= 620
    perm = (torch.randperm(nb - 2, generator=torch.Generator().manual_seed(3)) + 1).tolist()     # ids 1 .. nb - 2
    src, dst = perm[:290], perm[290:580]
    src[:100] = sorted(src[:100], reverse=True)
    dst[:100] = sorted(dst[:100], reverse=True)
    extra_src = [perm[600], nb, perm[602], perm[603], nb - 1] + src[:5]
    extra_dst = [perm[600], perm[601], -1, nb + 7, 0] + perm[604:609]
    src[150:150], dst[150:150] = extra_src, extra_dst
    assert len(src) == len(dst) == 300
    return src, dst


def _expected(pool, src, dst, nb):
    """The copy applied from the host on a clone: valid pairs only, every pair reading the ORIGINAL pool."""
    ref = pool.clone()
    ok = [(s, d) for s, d in zip(src, dst) if 0 <= s < nb and 0 <= d < nb and s != d]
    if ok:
        s_idx = torch.tensor([s for s, _ in ok], device=pool.device)
        d_idx = torch.tensor([d for _, d in ok], device=pool.device)
        assert len(set(d_idx.tolist())) == len(ok) and not set(d_idx.tolist()) & set(s_idx.tolist())
        ref[d_idx] = pool[s_idx]
    return ref


@pytest.mark.parametrize("n", [0, 1, 2, 300])
@pytest.mark.parametrize("block_bytes", BLOCK_BYTES)
def test_copy_matches_a_host_applied_copy_over_the_whole_pool(block_bytes, n):
    from swiftllm_amd.worker.kernels.kv_copy import kv_copy_blocks
    nb = NUM_BLOCKS
    k, v = _pools(nb, block_bytes, seed=block_bytes + n)
    src, dst = _pairs(n, nb)
    want_k, want_v = _expected(k, src, dst, nb), _expected(v, src, dst, nb)
    if n:
        assert not torch.equal(want_k, k) and not torch.equal(want_v, v)        # (the case copies something)
    kv_copy_blocks(k, v, torch.tensor(src, dtype=torch.int32, device="cuda"),
                   torch.tensor(dst, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(k, want_k)
    assert torch.equal(v, want_v)


def test_byte_offsets_past_4_gib():
    """block_bytes = 1 MiB in pools of 4100 blocks: id * block_bytes passes 2^32 for blocks >= 4096, on both sides of
    the copy. The pools are uninitialised memory; the touched blocks are filled, and compared with their sources."""
    from swiftllm_amd.worker.kernels.kv_copy import kv_copy_blocks
    nb = 4100
    k = torch.empty((nb, MIB), dtype=torch.uint8, device="cuda")
    v = torch.empty((nb, MIB), dtype=torch.uint8, device="cuda")
    src, dst = [4097, 5, 4099, 2], [4098, 4096, 7, 1]
    # what a 32-bit offset would touch instead: blocks id - 4096 (1, 2, 0, 3); 1 and 2 are in the lists so that a wrapped
    # copy collides with a checked block, 0 and 3 are guards
    guards = [0, 3, 6, 4095]
    g = torch.Generator(device="cuda").manual_seed(9)
    before = {}
    for pool in (k, v):
        for b in src + dst + guards:
            pool[b] = torch.randint(0, 256, (MIB,), dtype=torch.uint8, device="cuda", generator=g)
            before[(pool.data_ptr(), b)] = pool[b].clone()
    kv_copy_blocks(k, v, torch.tensor(src, dtype=torch.int32, device="cuda"),
                   torch.tensor(dst, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for pool in (k, v):
        for s, d in zip(src, dst):
            assert torch.equal(pool[d], before[(pool.data_ptr(), s)]), (s, d)
            assert torch.equal(pool[s], before[(pool.data_ptr(), s)]), s
        for b in guards:
            assert torch.equal(pool[b], before[(pool.data_ptr(), b)]), b


def test_entry_point_refusals_launch_nothing():
    """The contract of include/swiftllm_hip.h, through the C ABI directly, on real device pointers: every refused call
    returns its code and the pools keep their bytes (the ids would copy block 0 over block 1)."""
    hip = _hip()
    lib = hip.load()
    OK, BAD, UNSUPPORTED = 0, -1, -2
    k, v = _pools(4, 512, seed=1)
    k0, v0 = k.clone(), v.clone()
    src = torch.tensor([0], dtype=torch.int32, device="cuda")
    dst = torch.tensor([1], dtype=torch.int32, device="cuda")
    kp, vp, sp, dp, st = k.data_ptr(), v.data_ptr(), src.data_ptr(), dst.data_ptr(), hip.stream()
    f = lib.swl_kv_copy_blocks
    assert f(None, None, None, None, 0, 512, 4, st) == OK                  # n == 0: nothing to do, nothing looked at
    assert f(kp, vp, sp, dp, 0, 512, 4, st) == OK
    for args in ((None, vp, sp, dp), (kp, None, sp, dp), (kp, vp, None, dp), (kp, vp, sp, None)):
        assert f(*args, 1, 512, 4, st) == BAD
    assert f(kp, vp, sp, dp, -1, 512, 4, st) == BAD
    assert f(kp, vp, sp, dp, 1, 0, 4, st) == BAD
    assert f(kp, vp, sp, dp, 1, -512, 4, st) == BAD
    assert f(kp, vp, sp, dp, 1, 512, 0, st) == BAD
    assert f(kp, vp, sp, dp, 1, 512, -4, st) == BAD
    assert f(kp, vp, sp, dp, 1, 520, 4, st) == UNSUPPORTED                 # block_bytes % 16 != 0
    assert f(kp + 8, vp, sp, dp, 1, 512, 3, st) == BAD                     # misaligned pool base
    assert f(kp, vp + 4, sp, dp, 1, 512, 3, st) == BAD
    with pytest.raises(hip.HipLibraryError):
        hip.call("swl_kv_copy_blocks", kp, vp, sp, dp, 1, 520, 4, st)
    torch.cuda.synchronize()
    assert torch.equal(k, k0) and torch.equal(v, v0)
    assert f(kp, vp, sp, dp, 1, 512, 4, st) == OK                          # ... and the legal call copies
    torch.cuda.synchronize()
    assert torch.equal(k[1], k0[0]) and torch.equal(v[1], v0[0]) and torch.equal(k[[0, 2, 3]], k0[[0, 2, 3]])
