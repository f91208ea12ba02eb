"""Guided decoding on the device: build a guide's token bitmasks from its byte DFA, and apply one mask row per row of
logits before anything reads them (contract: csrc/guided.hip). The reference has no guided decoding
(swiftllm/worker/layers/post_layer.py:40 takes the argmax of the raw logits)."""
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from swiftllm_amd import _hip


class GuideArgs(NamedTuple):
    """Device views (fixed addresses: a captured hipGraph reads them on every replay)."""
    masks: torch.Tensor         # int32 [mask rows, W]: the pool
    row_index: torch.Tensor     # int32 [rows]: the mask row of each row of logits; outside the pool: the row is not guided


class DeviceVocab(NamedTuple):
    """The flat form of a guided.TokenVocab on the device."""
    tok_bytes: torch.Tensor     # uint8 [total] (at least one element)
    tok_offsets: torch.Tensor   # int32 [vocab + 1]
    vocab: int


def upload_vocab(vocab, vocab_size: int, device) -> DeviceVocab:
    """`vocab`: a guided.TokenVocab of exactly `vocab_size` ids."""
    if len(vocab) != vocab_size:
        raise ValueError(f"the guide vocabulary spells {len(vocab)} ids, the model's vocabulary has {vocab_size}")
    data, offsets = vocab.flat()
    if data.size == 0:
        data = np.zeros(1, dtype=np.uint8)
    return DeviceVocab(torch.from_numpy(data).to(device), torch.from_numpy(offsets).to(device), vocab_size)


def pack_rows(cursors: Sequence[Optional[object]], buf: np.ndarray) -> np.ndarray:
    """Write each row's mask row (`cursor.mask_row`) into `buf` (int32 [rows_cap]); None entries and rows past
    len(cursors) are not guided (-1)."""
    buf[:] = -1
    for r, c in enumerate(cursors):
        if c is not None:
            buf[r] = c.mask_row
    return buf


def build_guide_masks(masks: torch.Tensor, row_base: int, trans: torch.Tensor, accepting: torch.Tensor,
                      vocab: DeviceVocab, end_ids: Optional[torch.Tensor]) -> None:
    """Fill rows [row_base, row_base + S) of the pool `masks` (int32 [rows, W]) with the masks of the DFA `trans`
    (int32 [S, 256], -1 = dead) / `accepting` (uint8 or bool [S]) over `vocab`; `end_ids`: int32 device tensor or None.
    One launch on the current stream."""
    if masks.dim() != 2 or masks.dtype != torch.int32 or not masks.is_contiguous():
        raise ValueError("build_guide_masks: the pool must be a contiguous int32 [rows, W] tensor")
    _hip.require_gpu_tensor(masks, "the guide mask pool")
    dev = masks.device
    s = trans.shape[0]
    if trans.dim() != 2 or trans.shape[1] != 256 or trans.dtype != torch.int32 or not trans.is_contiguous():
        raise ValueError("build_guide_masks: trans must be a contiguous int32 [S, 256] tensor")
    if accepting.dtype not in (torch.uint8, torch.bool) or accepting.numel() != s or not accepting.is_contiguous():
        raise ValueError("build_guide_masks: accepting must be a contiguous uint8 / bool [S] tensor")
    if row_base < 0 or row_base + s > masks.shape[0]:
        raise ValueError(f"build_guide_masks: rows [{row_base}, {row_base + s}) do not fit a pool of {masks.shape[0]}")
    if masks.shape[1] * 32 < vocab.vocab:
        raise ValueError("build_guide_masks: the pool's rows are narrower than the vocabulary")
    if (vocab.tok_offsets.dtype != torch.int32 or vocab.tok_offsets.numel() != vocab.vocab + 1
            or vocab.tok_bytes.dtype != torch.uint8 or not vocab.tok_offsets.is_contiguous()
            or not vocab.tok_bytes.is_contiguous()):
        raise ValueError("build_guide_masks: the vocabulary's flat form is int32 [vocab + 1] offsets over uint8 bytes")
    n_end = 0
    if end_ids is not None and end_ids.numel():
        if end_ids.dtype != torch.int32 or not end_ids.is_contiguous() or end_ids.device != dev:
            raise ValueError("build_guide_masks: end_ids must be a contiguous int32 tensor on the pool's device")
        n_end = end_ids.numel()
    for t in (trans, accepting, vocab.tok_bytes, vocab.tok_offsets):
        if t.device != dev:
            raise ValueError("build_guide_masks: every tensor must live on the pool's device")
    _hip.call("swl_guide_build_masks", _hip.ptr(masks), row_base, s, masks.shape[1], _hip.ptr(trans), _hip.ptr(accepting),
              _hip.ptr(vocab.tok_bytes), _hip.ptr(vocab.tok_offsets), vocab.vocab,
              _hip.ptr(end_ids) if n_end else 0, n_end, _hip.stream())


def mask_logits(logits: torch.Tensor, args: GuideArgs) -> torch.Tensor:
    """Apply mask row `args.row_index[r]` to row r of [rows, n] fp16/bf16 logits, in place (csrc/guided.hip), and return
    them: elements whose bit is clear become -inf; a row whose index lies outside the pool is left alone."""
    if logits.dim() != 2 or logits.dtype not in (torch.float16, torch.bfloat16) or logits.stride(1) != 1:
        raise ValueError("mask_logits: logits must be a [rows, n] fp16/bf16 tensor with unit column stride")
    rows, n = logits.shape
    if rows == 0:
        return logits
    masks, row_index = args.masks, args.row_index
    if masks.dim() != 2 or masks.dtype != torch.int32 or not masks.is_contiguous() or masks.device != logits.device:
        raise ValueError("mask_logits: the pool must be a contiguous int32 [rows, W] tensor on the logits' device")
    if masks.shape[1] * 32 < n:
        raise ValueError(f"mask_logits: mask rows of {masks.shape[1]} words do not cover {n} logits")
    if (row_index.dtype != torch.int32 or not row_index.is_contiguous() or row_index.numel() < rows
            or row_index.device != logits.device):
        raise ValueError(f"mask_logits: row_index must be a contiguous int32 tensor of at least {rows} elements on the "
                         "logits' device")
    _hip.call("swl_logits_mask", _hip.ptr(logits), rows, n, logits.stride(0), _hip.dtype_code(logits.dtype),
              _hip.ptr(masks), masks.shape[0], masks.shape[1], _hip.ptr(row_index), _hip.stream())
    return logits
