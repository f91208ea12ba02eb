"""Penalties, logit bias and min-p on the logits, in place, before a token is picked (contract: csrc/logits_adjust.hip).
The reference has no logits processing (swiftllm/worker/layers/post_layer.py:40 takes the argmax of the raw logits)."""
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from swiftllm_amd import _hip


class RowEdits(NamedTuple):
    """What one row asks for, on the host: its entries (each id once) and its four parameters."""
    ids: np.ndarray     # int32 [E]
    meta: np.ndarray    # int32 [E]: bits 0..30 = count among the output tokens, bit 31 = seen in the prompt
    bias: np.ndarray    # float32 [E]: finite or -inf
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    min_p_gap: float = -np.inf      # T * ln(min_p); -inf: min-p off


class AdjustArgs(NamedTuple):
    """Device views over one persistent buffer (fixed addresses: a captured hipGraph reads them on every replay)."""
    offsets: torch.Tensor       # int32 [rows + 1]: CSR index into the three arrays below
    ids: torch.Tensor           # int32 [E]
    meta: torch.Tensor          # int32 [E]
    bias: torch.Tensor          # float32 [E]
    row_params: torch.Tensor    # float32 [rows, 4]: repetition, presence, frequency penalty, min-p gap


def buffer_len(rows_cap: int, edit_cap: int) -> int:
    """int32 words of a buffer for `rows_cap` rows and `edit_cap` entries: [rows_cap + 1] offsets, [rows_cap, 4]
    parameter bits, then `edit_cap` ids, `edit_cap` meta words, `edit_cap` bias bits."""
    return 5 * rows_cap + 1 + 3 * edit_cap


def edit_capacity(buf_len: int, rows_cap: int) -> int:
    return (buf_len - 5 * rows_cap - 1) // 3


def pack_edits(rows: Sequence[Optional[RowEdits]], buf: np.ndarray, rows_cap: int, vocab_size: Optional[int] = None) -> int:
    """Fill the host twin `buf` (flat int32 [buffer_len(rows_cap, edit_cap)]) of the device buffer. Rows past len(rows)
    and None rows are inert: an empty segment, repetition penalty 1, gap -inf. Returns the number of entries written.
    With `vocab_size`, every id is held to [0, vocab_size) and to appearing once in its row (ValueError otherwise)."""
    if buf.dtype != np.int32 or buf.ndim != 1 or not buf.flags.c_contiguous:
        raise ValueError("pack_edits: the host buffer must be a contiguous flat int32 array")
    if len(rows) > rows_cap:
        raise ValueError(f"pack_edits: {len(rows)} rows, the buffer holds {rows_cap}")
    cap = edit_capacity(buf.size, rows_cap)
    if cap < 0:
        raise ValueError("pack_edits: the buffer is smaller than its row header")
    base = 5 * rows_cap + 1
    offsets = buf[:rows_cap + 1]
    params = buf[rows_cap + 1:base].view(np.float32).reshape(rows_cap, 4)
    params[:] = (1.0, 0.0, 0.0, -np.inf)
    ids, meta = buf[base:base + cap], buf[base + cap:base + 2 * cap]
    bias = buf[base + 2 * cap:base + 3 * cap].view(np.float32)
    at = 0
    for r, row in enumerate(rows):
        offsets[r] = at
        if row is None:
            continue
        k = len(row.ids)
        if len(row.meta) != k or len(row.bias) != k:
            raise ValueError(f"pack_edits: row {r}: ids, meta and bias differ in length")
        if at + k > cap:
            raise ValueError(f"pack_edits: {at + k} entries, the buffer holds {cap}")
        if vocab_size is not None and k:
            rid = np.asarray(row.ids)
            if int(rid.min()) < 0 or int(rid.max()) >= vocab_size:
                raise ValueError(f"row {r}: token ids must lie in [0, {vocab_size})")
            if np.unique(rid).size != k:
                raise ValueError(f"row {r}: a token id appears twice")
        ids[at:at + k] = row.ids
        meta[at:at + k] = row.meta
        bias[at:at + k] = row.bias
        params[r] = (row.repetition_penalty, row.presence_penalty, row.frequency_penalty, row.min_p_gap)
        at += k
    offsets[len(rows):] = at
    return at


def device_args(dev_buf: torch.Tensor, rows_cap: int) -> AdjustArgs:
    """AdjustArgs over a device int32 [buffer_len(rows_cap, edit_cap)] buffer laid out by `pack_edits`."""
    cap = edit_capacity(dev_buf.numel(), rows_cap)
    base = 5 * rows_cap + 1
    return AdjustArgs(dev_buf[:rows_cap + 1], dev_buf[base:base + cap], dev_buf[base + cap:base + 2 * cap],
                      dev_buf[base + 2 * cap:base + 3 * cap].view(torch.float32),
                      dev_buf[rows_cap + 1:base].view(torch.float32).view(rows_cap, 4))


def adjust_logits(logits: torch.Tensor, args) -> torch.Tensor:
    """Edit [rows, n] fp16/bf16 logits in place (csrc/logits_adjust.hip) and return them. `args`: AdjustArgs (device
    views, e.g. the model's persistent buffer — capturable; its values are the caller's promise), or a list of RowEdits /
    None per row (checked against the vocabulary and for duplicate ids, packed and uploaded here)."""
    if logits.dim() != 2 or logits.dtype not in (torch.float16, torch.bfloat16) or logits.stride(1) != 1:
        raise ValueError("adjust_logits: logits must be a [rows, n] fp16/bf16 tensor with unit column stride")
    rows, n = logits.shape
    if rows == 0:
        return logits
    if not isinstance(args, AdjustArgs):
        if len(args) != rows:
            raise ValueError(f"adjust_logits: {len(args)} rows of edits for {rows} rows of logits")
        total = sum(len(r.ids) for r in args if r is not None)
        host = np.empty(buffer_len(rows, max(total, 1)), dtype=np.int32)
        pack_edits(args, host, rows, vocab_size=n)
        args = device_args(torch.from_numpy(host).to(logits.device), rows)
    for name, t, dt, need in (("offsets", args.offsets, torch.int32, rows + 1), ("ids", args.ids, torch.int32, 0),
                              ("meta", args.meta, torch.int32, 0), ("bias", args.bias, torch.float32, 0),
                              ("row_params", args.row_params, torch.float32, 4 * rows)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() < need or t.device != logits.device:
            raise ValueError(f"adjust_logits: `{name}` must be a contiguous {dt} tensor of at least {need} elements on the "
                             "logits' device")
    if not (args.ids.numel() == args.meta.numel() == args.bias.numel()):
        raise ValueError("adjust_logits: ids, meta and bias differ in length")
    _hip.call("swl_logits_adjust", _hip.ptr(logits), rows, n, logits.stride(0), _hip.dtype_code(logits.dtype),
              _hip.ptr(args.offsets), _hip.ptr(args.ids), _hip.ptr(args.meta), _hip.ptr(args.bias),
              _hip.ptr(args.row_params), _hip.stream())
    return logits
