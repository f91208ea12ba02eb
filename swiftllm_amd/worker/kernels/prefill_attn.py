"""Prefill (varlen causal) attention operator.

Reference: swiftllm/worker/kernels/prefill_attn.py:102-139 (`prefill_attention`), which has the
contract of the `vllm_flash_attn.flash_attn_varlen_func` call the reference's layer actually makes
(transformer_layer.py:83-96). Here it is the one and only prefill attention path.
"""
import torch

from swiftllm_amd import _hip
from ._layout import token_stride


def prefill_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, o: torch.Tensor,
                      model_config, engine_config, infer_state):
    """o[:P] = causal softmax(q k^T * scale) v per prefill sequence (GQA). q/k/v/o are
    [tokens, heads, head_dim]; only the first `num_prefill_tokens` rows are touched."""
    _hip.require_gpu_tensor(q, "q")
    if infer_state.num_prefill_seqs == 0:
        return
    cu = infer_state.prefill_seq_start_locs_with_end
    assert cu.dtype == torch.int32 and cu.is_contiguous() and cu.numel() == infer_state.num_prefill_seqs + 1
    assert q.dtype == k.dtype == v.dtype == o.dtype
    if o.dim() == 2:
        o = o.view(o.shape[0], model_config.num_q_heads, model_config.head_dim)
    _hip.call("swl_prefill_attn_varlen", _hip.ptr(o), _hip.ptr(q), _hip.ptr(k), _hip.ptr(v),
              _hip.ptr(cu), infer_state.num_prefill_seqs, infer_state.max_prefill_len,
              model_config.num_q_heads, model_config.num_kv_heads, model_config.head_dim,
              infer_state.softmax_scale, token_stride(q, "q"), token_stride(k, "k"),
              token_stride(v, "v"), token_stride(o, "o"), _hip.dtype_code(q.dtype), _hip.stream())


def prefill_attention_paged(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                            o: torch.Tensor, model_config, engine_config, infer_state, cur_layer: int):
    """Chunked prefill (no reference counterpart): prefill sequence s has `infer_state.prefill_ctx_lens[s]` tokens in
    the pool already and its new tokens' K/V were stored behind them on this stream; row i of its chunk attends to every
    resident key up to its own position. All K/V is read from the pools, 16-bit or FP8 (e4m3): one kernel, csrc/prefill_attn_paged.hip. q/o are
    [tokens, heads, head_dim]; only the first `num_prefill_tokens` rows are touched."""
    _hip.require_gpu_tensor(q, "q")
    st = infer_state
    if st.num_prefill_seqs == 0:
        return
    cu, ctx = st.prefill_seq_start_locs_with_end, st.prefill_ctx_lens
    assert cu.dtype == torch.int32 and cu.is_contiguous() and cu.numel() == st.num_prefill_seqs + 1
    assert ctx is not None and ctx.dtype == torch.int32 and ctx.is_contiguous() and ctx.numel() == st.num_prefill_seqs
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and block_table.is_contiguous()
    if o.dim() == 2:
        o = o.view(o.shape[0], model_config.num_q_heads, model_config.head_dim)
    if k_cache.dtype == torch.float8_e4m3fn:    # the FP8 instantiation: the chunk's own keys come back quantised
        scales = st.kv_scales
        assert q.dtype == o.dtype and v_cache.dtype == torch.float8_e4m3fn
        assert scales is not None and scales.dtype == torch.float32 and scales.is_contiguous()
        assert scales.shape == (2, model_config.num_layers, model_config.num_kv_heads)
        _hip.call("swl_prefill_attn_paged_fp8", _hip.ptr(o), _hip.ptr(q), _hip.ptr(k_cache), _hip.ptr(v_cache),
                  _hip.ptr(scales), _hip.ptr(block_table), _hip.ptr(st.seq_ids), _hip.ptr(cu), _hip.ptr(ctx),
                  st.num_prefill_seqs, st.max_prefill_len, st.max_prefill_total_len, model_config.num_q_heads,
                  model_config.num_kv_heads, model_config.head_dim, model_config.num_layers, engine_config.block_size,
                  cur_layer, block_table.shape[1], st.softmax_scale, token_stride(q, "q"), token_stride(o, "o"),
                  _hip.dtype_code(q.dtype), _hip.stream())
        return
    assert q.dtype == o.dtype == k_cache.dtype == v_cache.dtype
    _hip.call("swl_prefill_attn_paged", _hip.ptr(o), _hip.ptr(q), _hip.ptr(k_cache), _hip.ptr(v_cache),
              _hip.ptr(block_table), _hip.ptr(st.seq_ids), _hip.ptr(cu), _hip.ptr(ctx), st.num_prefill_seqs,
              st.max_prefill_len, st.max_prefill_total_len, model_config.num_q_heads, model_config.num_kv_heads,
              model_config.head_dim, model_config.num_layers, engine_config.block_size, cur_layer, block_table.shape[1],
              st.softmax_scale, token_stride(q, "q"), token_stride(o, "o"), _hip.dtype_code(q.dtype), _hip.stream())
