"""KV-cache store operator. Reference: swiftllm/worker/kernels/kvcache_mgmt.py:81-122."""
import torch

from swiftllm_amd import _hip
from ._layout import token_stride


# ---- the argument groups of the KV-store entries (csrc/kv_store.h), shared with rotary_emb.py ---------------------------------
def _prefill_ctx(st):
    """`st.prefill_ctx_lens` (chunked prefill: token t of sequence s goes to logical position ctx[s] + t), or None."""
    ctx = getattr(st, "prefill_ctx_lens", None)
    if ctx is not None:
        assert ctx.dtype == torch.int32 and ctx.is_contiguous() and ctx.numel() == st.num_prefill_seqs
    return ctx


def _prefill_tables(block_table, st, *ctx):
    """block table, ids, start rows, lengths [, contexts] of the prefill sequences, then their count and longest length"""
    return (_hip.ptr(block_table), _hip.ptr(st.seq_ids), _hip.ptr(st.prefill_seq_start_locs),
            _hip.ptr(st.prefill_seq_lens), *map(_hip.ptr, ctx), st.num_prefill_seqs, st.max_prefill_len)


def _decode_tables(block_table, st):
    """block table, ids and lengths of the decoding sequences (they follow the prefill ones), then their count"""
    ids = st.seq_ids[st.num_prefill_seqs:] if st.num_prefill_seqs else st.seq_ids
    return _hip.ptr(block_table), _hip.ptr(ids), _hip.ptr(st.decoding_seq_lens), st.num_decoding_seqs


def _geometry(cur_layer, model_config, engine_config, block_table, kv_heads, head_dim, *q_heads):
    """cur_layer L [H] KVH bs D mbps: the order of every entry but the two fused decode ones"""
    return (cur_layer, model_config.num_layers, *q_heads, kv_heads, engine_config.block_size, head_dim,
            block_table.shape[1])


def _rows(**tensors):
    """the token pitch of each [tokens, heads, head_dim] view, then the dtype code and the stream"""
    first = next(iter(tensors.values()))
    return (*(token_stride(t, name) for name, t in tensors.items()), _hip.dtype_code(first.dtype), _hip.stream())


def store_kvcache(k: torch.Tensor, v: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                  block_table: torch.Tensor, model_config, engine_config, infer_state,
                  cur_layer: int):
    """Write this forward's K/V rows into the paged pools: whole prefill sequences block by block
    (prompt CHUNKS at their offset when `infer_state.prefill_ctx_lens` is set), and the single new
    token of every decoding sequence."""
    _hip.require_gpu_tensor(k, "k")
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and block_table.is_contiguous()
    assert infer_state.seq_ids.is_contiguous() and infer_state.decoding_seq_lens.is_contiguous()
    st = infer_state
    ctx = _prefill_ctx(st) if st.num_prefill_seqs > 0 else None
    if k_cache.dtype == torch.float8_e4m3fn:
        # FP8 (e4m3fn) pools: the quantising instantiations (csrc/kvcache.hip). Whole prompts go through the `_at` store
        # with null contexts. `infer_state.kv_inv_scales` is fp32 [2, L, KVH] = 1 / scale.
        inv = st.kv_inv_scales
        assert k.dtype == v.dtype and v_cache.dtype == torch.float8_e4m3fn
        assert inv is not None and inv.dtype == torch.float32 and inv.is_contiguous()
        assert inv.shape == (2, model_config.num_layers, model_config.num_kv_heads)
        prefill, decode, scales, ctx_arg = "swl_store_kv_prefill_at_fp8", "swl_store_kv_decode_fp8", (_hip.ptr(inv),), (ctx,)
    else:
        assert k.dtype == v.dtype == k_cache.dtype == v_cache.dtype
        decode, scales = "swl_store_kv_decode", ()
        prefill, ctx_arg = ("swl_store_kv_prefill", ()) if ctx is None else ("swl_store_kv_prefill_at", (ctx,))
    pools = _hip.ptr(k_cache), _hip.ptr(v_cache)
    common = (*_geometry(cur_layer, model_config, engine_config, block_table, model_config.num_kv_heads,
                         model_config.head_dim), *_rows(k=k, v=v))
    if st.num_prefill_seqs > 0:
        _hip.call(prefill, *pools, _hip.ptr(k), _hip.ptr(v), *scales, *_prefill_tables(block_table, st, *ctx_arg), *common)
    if st.num_decoding_seqs > 0:
        p = st.num_prefill_tokens
        _hip.call(decode, *pools, _hip.ptr(k[p:]), _hip.ptr(v[p:]), *scales, *_decode_tables(block_table, st), *common)
