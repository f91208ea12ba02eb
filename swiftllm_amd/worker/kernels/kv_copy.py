"""kv_copy_blocks — copy whole KV blocks inside the GPU pools (csrc/kv_copy.hip; no reference counterpart).

One launch on torch's current stream for every (source, destination) pair, K and V pool; the ids are device tensors."""
import torch

from swiftllm_amd import _hip


def kv_copy_blocks(k_cache: torch.Tensor, v_cache: torch.Tensor, src_block_ids: torch.Tensor,
                   dst_block_ids: torch.Tensor):
    """Block src_block_ids[i] -> block dst_block_ids[i] in both pools (int32 device tensors of one length). Pairs with
    equal ids or an id outside the pool are skipped by the kernel; the distinct destinations must be disjoint from the
    sources (the caller's guarantee)."""
    n = int(src_block_ids.numel())
    if n != int(dst_block_ids.numel()):
        raise ValueError("kv_copy_blocks needs as many destination ids as source ids")
    if n == 0:
        return
    _hip.require_gpu_tensor(k_cache, "k_cache")
    _hip.require_gpu_tensor(src_block_ids, "src_block_ids")
    _hip.require_gpu_tensor(dst_block_ids, "dst_block_ids")
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape == v_cache.shape
    assert src_block_ids.dtype == torch.int32 and dst_block_ids.dtype == torch.int32
    assert src_block_ids.is_contiguous() and dst_block_ids.is_contiguous()
    block_bytes = k_cache.numel() * k_cache.element_size() // k_cache.shape[0]
    _hip.call("swl_kv_copy_blocks", _hip.ptr(k_cache), _hip.ptr(v_cache), _hip.ptr(src_block_ids),
              _hip.ptr(dst_block_ids), n, block_bytes, int(k_cache.shape[0]), _hip.stream())
