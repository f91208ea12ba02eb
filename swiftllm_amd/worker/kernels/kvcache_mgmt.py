"""KV-cache store operator. Reference: swiftllm/worker/kernels/kvcache_mgmt.py:81-122."""
import torch

from swiftllm_amd import _hip
from ._layout import token_stride


def store_kvcache(k: torch.Tensor, v: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                  block_table: torch.Tensor, model_config, engine_config, infer_state,
                  cur_layer: int):
    """Write this forward's K/V rows into the paged pools: whole prefill sequences block by block
    (prompt CHUNKS at their offset when `infer_state.prefill_ctx_lens` is set), and the single new
    token of every decoding sequence."""
    _hip.require_gpu_tensor(k, "k")
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and block_table.is_contiguous()
    assert infer_state.seq_ids.is_contiguous() and infer_state.decoding_seq_lens.is_contiguous()
    if k_cache.dtype == torch.float8_e4m3fn:
        return _store_kvcache_fp8(k, v, k_cache, v_cache, block_table, model_config, engine_config, infer_state, cur_layer)
    assert k.dtype == v.dtype == k_cache.dtype == v_cache.dtype
    ks, vs = token_stride(k, "k"), token_stride(v, "v")
    code, stream = _hip.dtype_code(k.dtype), _hip.stream()
    common = (cur_layer, model_config.num_layers, model_config.num_kv_heads,
              engine_config.block_size, model_config.head_dim, block_table.shape[1], ks, vs, code,
              stream)
    ctx = getattr(infer_state, "prefill_ctx_lens", None)
    if infer_state.num_prefill_seqs > 0 and ctx is not None:
        # chunked prefill: token t of sequence s goes to logical position ctx[s] + t
        assert ctx.dtype == torch.int32 and ctx.is_contiguous() and ctx.numel() == infer_state.num_prefill_seqs
        _hip.call("swl_store_kv_prefill_at", _hip.ptr(k_cache), _hip.ptr(v_cache), _hip.ptr(k),
                  _hip.ptr(v), _hip.ptr(block_table), _hip.ptr(infer_state.seq_ids),
                  _hip.ptr(infer_state.prefill_seq_start_locs),
                  _hip.ptr(infer_state.prefill_seq_lens), _hip.ptr(ctx), infer_state.num_prefill_seqs,
                  infer_state.max_prefill_len, *common)
    elif infer_state.num_prefill_seqs > 0:
        _hip.call("swl_store_kv_prefill", _hip.ptr(k_cache), _hip.ptr(v_cache), _hip.ptr(k),
                  _hip.ptr(v), _hip.ptr(block_table), _hip.ptr(infer_state.seq_ids),
                  _hip.ptr(infer_state.prefill_seq_start_locs),
                  _hip.ptr(infer_state.prefill_seq_lens), infer_state.num_prefill_seqs,
                  infer_state.max_prefill_len, *common)
    if infer_state.num_decoding_seqs > 0:
        p = infer_state.num_prefill_tokens
        _hip.call("swl_store_kv_decode", _hip.ptr(k_cache), _hip.ptr(v_cache), _hip.ptr(k[p:]),
                  _hip.ptr(v[p:]), _hip.ptr(block_table),
                  _hip.ptr(infer_state.seq_ids[infer_state.num_prefill_seqs:]),
                  _hip.ptr(infer_state.decoding_seq_lens), infer_state.num_decoding_seqs, *common)


def _store_kvcache_fp8(k, v, k_cache, v_cache, block_table, model_config, engine_config, infer_state, cur_layer: int):
    """FP8 (e4m3fn) pools: the quantising twins (csrc/kvcache_fp8.hip). Whole prompts go through the `_at` store with
    null contexts. `infer_state.kv_inv_scales` is fp32 [2, L, KVH] = 1 / scale."""
    inv = infer_state.kv_inv_scales
    assert k.dtype == v.dtype and v_cache.dtype == torch.float8_e4m3fn
    assert inv is not None and inv.dtype == torch.float32 and inv.is_contiguous()
    assert inv.shape == (2, model_config.num_layers, model_config.num_kv_heads)
    common = (cur_layer, model_config.num_layers, model_config.num_kv_heads, engine_config.block_size,
              model_config.head_dim, block_table.shape[1], token_stride(k, "k"), token_stride(v, "v"),
              _hip.dtype_code(k.dtype), _hip.stream())
    if infer_state.num_prefill_seqs > 0:
        ctx = getattr(infer_state, "prefill_ctx_lens", None)
        if ctx is not None:
            assert ctx.dtype == torch.int32 and ctx.is_contiguous() and ctx.numel() == infer_state.num_prefill_seqs
        _hip.call("swl_store_kv_prefill_at_fp8", _hip.ptr(k_cache), _hip.ptr(v_cache), _hip.ptr(k), _hip.ptr(v),
                  _hip.ptr(inv), _hip.ptr(block_table), _hip.ptr(infer_state.seq_ids),
                  _hip.ptr(infer_state.prefill_seq_start_locs), _hip.ptr(infer_state.prefill_seq_lens), _hip.ptr(ctx),
                  infer_state.num_prefill_seqs, infer_state.max_prefill_len, *common)
    if infer_state.num_decoding_seqs > 0:
        p = infer_state.num_prefill_tokens
        _hip.call("swl_store_kv_decode_fp8", _hip.ptr(k_cache), _hip.ptr(v_cache), _hip.ptr(k[p:]), _hip.ptr(v[p:]),
                  _hip.ptr(inv), _hip.ptr(block_table), _hip.ptr(infer_state.seq_ids[infer_state.num_prefill_seqs:]),
                  _hip.ptr(infer_state.decoding_seq_lens), infer_state.num_decoding_seqs, *common)
