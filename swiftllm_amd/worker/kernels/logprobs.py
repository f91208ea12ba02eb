"""Log-probability and rank of the token each row picked, and the row's top-N alternatives (contract: csrc/logprobs.hip).
The reference returns token ids only (swiftllm/worker/layers/post_layer.py:40); this is an addition."""
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from swiftllm_amd import _hip
from swiftllm_amd.sampling_params import MAX_LOGPROBS, TokenLogprob


class LogprobArgs(NamedTuple):
    """Device views over one persistent buffer (fixed addresses: a captured hipGraph reads and writes them on every
    replay). Column 0 of `lp` / `ids` is the chosen token, columns 1..top_n[r] the alternatives."""
    top_n: torch.Tensor     # int32 [rows]: N of the row, < 0: the row does not ask
    lp: torch.Tensor        # float32 [rows, cap + 1]
    ids: torch.Tensor       # int32 [rows, cap + 1]
    rank: torch.Tensor      # int32 [rows]
    cap: int                # alternatives a row holds at most (0..20)


def buffer_len(rows_cap: int, cap: int = MAX_LOGPROBS) -> int:
    """int32 words of a buffer for `rows_cap` rows: [rows_cap] top_n, then what comes back — [rows_cap] rank,
    [rows_cap, cap + 1] logprob bits, [rows_cap, cap + 1] ids."""
    return rows_cap * (2 + 2 * (cap + 1))


def device_args(dev_buf: torch.Tensor, rows_cap: int, cap: int = MAX_LOGPROBS) -> LogprobArgs:
    """LogprobArgs over a device int32 [buffer_len(rows_cap, cap)] buffer."""
    w = rows_cap * (cap + 1)
    return LogprobArgs(dev_buf[:rows_cap], dev_buf[2 * rows_cap:2 * rows_cap + w].view(torch.float32).view(rows_cap, cap + 1),
                       dev_buf[2 * rows_cap + w:2 * rows_cap + 2 * w].view(rows_cap, cap + 1),
                       dev_buf[rows_cap:2 * rows_cap], cap)


def pack_top_n(top_n: Sequence[Optional[int]], buf: np.ndarray) -> np.ndarray:
    """Write the rows' N into `buf` (int32 [rows_cap]); None entries and rows past len(top_n) do not ask (-1)."""
    buf[:] = -1
    for r, n in enumerate(top_n):
        if n is not None:
            buf[r] = n
    return buf


def unpack(results: np.ndarray, rows_cap: int, top_n: Sequence[Optional[int]],
           cap: int = MAX_LOGPROBS) -> List[Optional[TokenLogprob]]:
    """The host copy of a buffer's results (int32 [buffer_len - rows_cap]: everything behind top_n) as one TokenLogprob
    per asking row of `top_n`, None for the others. Alternatives a narrow row could not fill (id -1) are left out."""
    w = rows_cap * (cap + 1)
    rank = results[:rows_cap]
    lp = results[rows_cap:rows_cap + w].view(np.float32).reshape(rows_cap, cap + 1)
    ids = results[rows_cap + w:rows_cap + 2 * w].reshape(rows_cap, cap + 1)
    out = []
    for r, n in enumerate(top_n):
        if n is None:
            out.append(None)
            continue
        row_ids, row_lp = ids[r, :min(n, cap) + 1].tolist(), lp[r, :min(n, cap) + 1].tolist()
        out.append(TokenLogprob(row_ids[0], row_lp[0], int(rank[r]),
                                tuple((i, v) for i, v in zip(row_ids[1:], row_lp[1:]) if i >= 0)))
    return out


def token_logprobs(logits: torch.Tensor, tokens: torch.Tensor, args) -> LogprobArgs:
    """Score the picked `tokens` (int64 [rows], device) against [rows, n] fp16/bf16 logits: one launch (csrc/logprobs.hip)
    that fills `args` and returns it. `args`: LogprobArgs (device views, e.g. the model's persistent buffer — capturable),
    or a list with one N (0..20) or None per row: a fresh buffer is made and uploaded here."""
    if logits.dim() != 2 or logits.dtype not in (torch.float16, torch.bfloat16) or logits.stride(1) != 1:
        raise ValueError("token_logprobs: logits must be a [rows, n] fp16/bf16 tensor with unit column stride")
    rows, n = logits.shape
    dev = logits.device
    if not isinstance(args, LogprobArgs):
        if len(args) != rows:
            raise ValueError(f"token_logprobs: {len(args)} entries of N for {rows} rows of logits")
        if any(v is not None and not 0 <= v <= MAX_LOGPROBS for v in args):
            raise ValueError(f"token_logprobs: N must lie in [0, {MAX_LOGPROBS}]")
        host = np.zeros(buffer_len(max(rows, 1)), dtype=np.int32)
        pack_top_n(args, host[:max(rows, 1)])
        args = device_args(torch.from_numpy(host).to(dev), max(rows, 1))
    if rows == 0:
        return args
    if tokens.dtype != torch.int64 or not tokens.is_contiguous() or tokens.numel() < rows or tokens.device != dev:
        raise ValueError("token_logprobs: tokens must be a contiguous int64 tensor of at least `rows` elements on the "
                         "logits' device")
    cols = args.cap + 1
    for name, t, dt, need in (("top_n", args.top_n, torch.int32, rows), ("lp", args.lp, torch.float32, rows * cols),
                              ("ids", args.ids, torch.int32, rows * cols), ("rank", args.rank, torch.int32, rows)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() < need or t.device != dev:
            raise ValueError(f"token_logprobs: `{name}` must be a contiguous {dt} tensor of at least {need} elements on "
                             "the logits' device")
    _hip.call("swl_logprobs", _hip.ptr(args.lp), _hip.ptr(args.ids), _hip.ptr(args.rank), _hip.ptr(logits), rows, n,
              logits.stride(0), _hip.dtype_code(logits.dtype), _hip.ptr(tokens), _hip.ptr(args.top_n), args.cap,
              _hip.stream())
    return args
