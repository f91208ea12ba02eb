"""Greedy and seeded sampling. Reference: swiftllm/worker/layers/post_layer.py:40 (`torch.argmax(logits, dim=1)`);
the reference has no stochastic sampling — `sample_rows` is an addition (contract: csrc/sampling.hip)."""
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from swiftllm_amd import _hip
from swiftllm_amd.sampling_params import SamplingParams

_scratch = {}   # device -> persistent candidate buffer (fixed address: hipGraph replays use it)
_retired = []   # outgrown buffers stay allocated: a captured hipGraph may still replay against them


def argmax_rows(logits: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """[rows, n] fp16/bf16 -> int64 [rows]; ties go to the lowest index (what torch.argmax does too). `out`: a caller-owned
    contiguous int64 [rows] destination (the one-sequence decode engine keeps its error word next to the token)."""
    rows, n = logits.shape
    if n % 8 or logits.stride(1) != 1 or logits.stride(0) % 8 or rows > 65535 or \
            logits.dtype not in (torch.float16, torch.bfloat16):
        res = torch.argmax(logits, dim=1)       # odd vocabularies: the generic device reduce
        return res if out is None else out.copy_(res)
    need = _hip.load().swl_argmax_scratch_bytes(rows)
    buf = _scratch.get(logits.device)
    if buf is None or buf.numel() < need:
        if buf is not None:
            _retired.append(buf)
        buf = torch.empty(max(need, 512 * 64 * 8), dtype=torch.uint8, device=logits.device)
        _scratch[logits.device] = buf
    if out is None:
        out = torch.empty((rows,), dtype=torch.int64, device=logits.device)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == rows
    _hip.call("swl_argmax", _hip.ptr(out), _hip.ptr(logits), _hip.ptr(buf), buf.numel(), rows, n,
              logits.stride(0), _hip.dtype_code(logits.dtype), _hip.stream())
    return out


class SampleArgs(NamedTuple):
    """Device views of per-row sampling parameters (at least `rows` entries each) and the rows' positions."""
    temperature: torch.Tensor   # float32 [rows]
    top_k: torch.Tensor         # int32 [rows]
    top_p: torch.Tensor         # float32 [rows]
    seed: torch.Tensor          # int32 [rows, 2]: (low, high) 32-bit halves of the 64-bit seed
    pos: torch.Tensor           # int32 [rows]: the index the sampled token takes in its sequence


def pack_params(params: Sequence[Optional[SamplingParams]], buf: np.ndarray) -> np.ndarray:
    """Write per-row parameters into `buf` (flat int32 [5 * cap], cap >= len(params)): [cap, 2] seed halves (low, high),
    then cap temperature bits, cap top_k, cap top_p bits. Rows past len(params) and None / greedy entries are greedy.
    None seeds must have been resolved (SamplingParams.with_seed)."""
    cap = buf.size // 5
    temp = np.zeros(cap, dtype=np.float32)
    top_p = np.ones(cap, dtype=np.float32)
    top_k = np.zeros(cap, dtype=np.int32)
    seeds = np.zeros(cap, dtype=np.uint64)
    for r, sp in enumerate(params):
        if sp is None or sp.greedy:
            continue
        assert sp.seed is not None, "resolve None seeds first (SamplingParams.with_seed)"
        temp[r], top_k[r], top_p[r], seeds[r] = sp.temperature, sp.top_k, sp.top_p, sp.seed
    pairs = buf[:2 * cap].reshape(cap, 2)
    pairs[:, 0] = (seeds & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)
    pairs[:, 1] = (seeds >> np.uint64(32)).astype(np.uint32).view(np.int32)
    buf[2 * cap:3 * cap] = temp.view(np.int32)
    buf[3 * cap:4 * cap] = top_k
    buf[4 * cap:5 * cap] = top_p.view(np.int32)
    return buf


def device_args(dev_buf: torch.Tensor, pos: torch.Tensor) -> SampleArgs:
    """SampleArgs over a device int32 [5 * cap] buffer laid out by `pack_params` (fixed addresses: capturable)."""
    cap = dev_buf.numel() // 5
    return SampleArgs(dev_buf[2 * cap:3 * cap].view(torch.float32), dev_buf[3 * cap:4 * cap],
                      dev_buf[4 * cap:5 * cap].view(torch.float32), dev_buf[:2 * cap].view(cap, 2), pos)


def sample_rows(logits: torch.Tensor, params, pos, out: torch.Tensor = None) -> torch.Tensor:
    """[rows, n] fp16/bf16 -> int64 [rows]: one seeded draw per row (csrc/sampling.hip), greedy rows exactly argmax_rows.
    `params`: SampleArgs (device, e.g. the model's persistent buffer — capturable), or a list of SamplingParams (uploaded
    here; None seeds are drawn fresh); `pos`: int32 device tensor [rows] or a list of ints (ignored when `params` is a
    SampleArgs: its own `pos` is used)."""
    rows, n = logits.shape
    if logits.dtype not in (torch.float16, torch.bfloat16) or logits.stride(1) != 1:
        raise ValueError("sample_rows: logits must be fp16/bf16 with unit column stride")
    dev = logits.device
    if not isinstance(params, SampleArgs):
        assert len(params) == rows
        host = pack_params([None if p is None else p.with_seed() for p in params], np.empty(5 * rows, np.int32))
        buf = torch.from_numpy(host).to(dev)
        pos_t = pos if isinstance(pos, torch.Tensor) else torch.tensor(list(pos), dtype=torch.int32)
        params = device_args(buf, pos_t.to(device=dev, dtype=torch.int32).contiguous())
    if out is None:
        out = torch.empty((rows,), dtype=torch.int64, device=dev)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == rows
    seed = params.seed
    assert seed.is_contiguous() and seed.shape[0] >= rows, "seed must be a contiguous int32 [rows, 2]"
    assert params.pos.dtype == torch.int32 and params.pos.is_contiguous() and params.pos.numel() >= rows
    _hip.call("swl_sample", _hip.ptr(out), _hip.ptr(logits), rows, n, logits.stride(0), _hip.dtype_code(logits.dtype),
              _hip.ptr(params.temperature), _hip.ptr(params.top_k), _hip.ptr(params.top_p), _hip.ptr(seed),
              _hip.ptr(params.pos), _hip.stream())
    return out
