"""LlamaInferState — the per-forward metadata bundle handed to every operator.

Field-compatible with the reference's swiftllm/worker/infer_state.py:4-29 (same names and meaning:
this is the kernel-argument contract), plus a few optional fields this implementation uses to keep
the hot path free of extra launches.
"""
import dataclasses
from typing import Optional

import torch


@dataclasses.dataclass
class LlamaInferState:
    batch_size: int
    num_tokens: int

    seq_ids: torch.Tensor   # [batch_size] int32
    softmax_scale: float    # head_dim ** -0.5

    num_prefill_seqs: int
    num_prefill_tokens: int
    prefill_seq_start_locs: torch.Tensor            # [num_prefill_seqs] int32
    prefill_seq_start_locs_with_end: torch.Tensor   # [num_prefill_seqs + 1] int32
    prefill_seq_lens: torch.Tensor                  # [num_prefill_seqs] int32
    max_prefill_len: int

    num_decoding_seqs: int
    decoding_seq_lens: torch.Tensor     # [num_decoding_seqs] int32, INCLUDING the token being decoded
    max_decoding_len: int

    seq_block_size: int     # split-K width of flash-decoding (tokens)
    num_seq_blocks: int     # ceil(max_decoding_len / seq_block_size)

    position_cos: torch.Tensor  # [num_tokens, head_dim/2] rows, or the whole rope cache (see below)
    position_sin: torch.Tensor

    ignore_kvcache: bool    # profiling run: no KV store, no paged attention

    # ---- additions --------------------------------------------------------------------------------
    # When set, position_cos/sin are the model's full rope tables and the rotary kernel looks up row
    # position_indices[t] itself (the reference gathers the rows first, model.py:350-351).
    position_indices: Optional[torch.Tensor] = None     # [num_tokens] int32
    # Row index of each sequence's last token in the activation matrix (post layer gather).
    last_token_indices: Optional[torch.Tensor] = None   # [batch_size] int32
    # Preallocated fp32 scratch for the flash-decoding partials.
    paged_attn_scratch: Optional[torch.Tensor] = None
    # A step with logits options (some row guided, processed, sampled or asking for logprobs): worker/step_logits.LogitsArgs,
    # one set of device views over the model's persistent buffers per option in use — the post layer masks, adjusts, draws
    # and scores with them. None: a plain step, argmax of the raw logits and no further launch.
    logits: Optional[object] = None
    # Chunked prefill: tokens of each prefill sequence already resident in the pool (int32 [num_prefill_seqs]); its new
    # tokens take logical positions [ctx, ctx + len) and attend to the pool (kernels/prefill_attn.prefill_attention_paged).
    # None: every prompt starts at position 0 and attends to its fresh projections — the reference's prefill.
    prefill_ctx_lens: Optional[torch.Tensor] = None
    max_prefill_total_len: int = 0      # max over prefill sequences of ctx + len (only read when prefill_ctx_lens is set)
    # FP8 KV pools (EngineConfig.kv_cache_dtype = "fp8_e4m3"): fp32 [2, L, KVH] k/v scales and their host-computed
    # reciprocals (what the quantising stores multiply by). None with 16-bit pools.
    kv_scales: Optional[torch.Tensor] = None
    kv_inv_scales: Optional[torch.Tensor] = None
    # Speculative-decoding verify step (LlamaModel.forward_verify): the "prefill" sequences bring their last accepted token
    # and drafts, attention is kernels/paged_attn.paged_attention_verify with seq_block_size / num_seq_blocks taken over
    # the total lengths, and verify_row_lens (int32 [num_tokens]) is position + 1 of every row.
    verify: bool = False
    verify_row_lens: Optional[torch.Tensor] = None
    # A LoRA step (some row names an adapter; worker/lora.LoraStep): the step's row -> slot tiles on the device and the
    # layers' slot stacks. Every layer then runs LlamaTransformerLayer._forward_lora. None: no adapter row — today's paths.
    lora: Optional[object] = None
