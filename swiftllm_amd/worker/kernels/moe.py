"""Mixture-of-experts FFN (Qwen3-MoE, Mixtral): the host side of csrc/moe.hip.

    logits = x @ router.T                                   (the dense `linear()`; storage dtype, as HuggingFace computes it)
    ids, w = top-k of softmax(logits)                       (moe_route: on the device, never read by the host)
    out[t] = sum_j w[t, j] * down[ids[t, j]] (up[ids[t, j]] x[t] * silu(gate[ids[t, j]] x[t]))

`moe_route`, `moe_align`, `moe_up_gate_silu`, `moe_down` and `moe_combine` are the five launches, each checking its
arguments; `moe_ffn` chains them behind the router GEMM. Nothing synchronises with the host and every grid is a function of
(tokens, k, E) alone, so a decode step's FFN is captured into the decode hipGraph like any other launch. A call takes at most
`max_pairs() // k` tokens: `moe_ffn` walks a longer step in token blocks, which bounds the workspace (per block: act
[pairs, I] 16-bit, y [pairs, H] fp32, the two tile tables) whatever the step; the buffers come from torch's caching
allocator, so the profiling forward of `profile_num_blocks` sees them. There is no fallback: a shape the kernels do not take
is an error.
"""
import torch

from swiftllm_amd import _hip
from .linear import linear

TILE_ROWS = 16
LOGITS_F32 = 2      # SWL_MOE_LOGITS_F32
MAX_EXPERTS = 256
MAX_TOP_K = 16


def supported(hidden: int, inter: int, num_experts: int, top_k: int, dtype: torch.dtype = torch.bfloat16) -> bool:
    """Whether the expert GEMMs take the geometry (host arithmetic only): hidden % 64 == 0, inter % 32 == 0, at most 256
    experts, top-k at most 16 and at most the expert count."""
    return bool(_hip.load().swl_moe_supported(int(hidden), int(inter), int(num_experts), int(top_k), _hip.dtype_code(dtype)))


def max_pairs() -> int:
    """(token, expert) pairs one call of the kernels takes."""
    return int(_hip.load().swl_moe_max_pairs())


def max_tiles(num_tokens: int, top_k: int, num_experts: int) -> int:
    """ceil(T k / 16) + min(E, T k): the tiles an alignment of the step can need."""
    return int(_hip.load().swl_moe_max_tiles(int(num_tokens), int(top_k), int(num_experts)))


def _logits_code(dtype: torch.dtype) -> int:
    return LOGITS_F32 if dtype == torch.float32 else _hip.dtype_code(dtype)


def moe_route(logits: torch.Tensor, top_k: int, norm_topk_prob: bool):
    """logits [T, E] (float16, bfloat16 or float32) -> (topk_ids int32 [T, k], topk_w fp32 [T, k])."""
    _hip.require_gpu_tensor(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    t, e = logits.shape
    ids = torch.empty((t, top_k), dtype=torch.int32, device=logits.device)
    w = torch.empty((t, top_k), dtype=torch.float32, device=logits.device)
    _hip.call("swl_moe_route", _hip.ptr(ids), _hip.ptr(w), _hip.ptr(logits), t, e, int(top_k), int(bool(norm_topk_prob)),
              logits.stride(0), _logits_code(logits.dtype), _hip.stream())
    return ids, w


def moe_align(topk_ids: torch.Tensor, num_experts: int):
    """topk_ids int32 [T, k] -> (tile_rows int32 [tiles * 16], tile_experts int32 [tiles]), tiles = max_tiles(T, k, E)."""
    _hip.require_gpu_tensor(topk_ids, "topk_ids")
    assert topk_ids.dtype == torch.int32 and topk_ids.is_contiguous() and topk_ids.dim() == 2
    t, k = topk_ids.shape
    tiles = max_tiles(t, k, num_experts) if t else 0
    if t and not tiles:
        raise _hip.HipLibraryError(f"swl_moe_align takes no step of {t} tokens x top-{k} over {num_experts} experts")
    rows = torch.empty((tiles * TILE_ROWS,), dtype=torch.int32, device=topk_ids.device)
    experts = torch.empty((tiles,), dtype=torch.int32, device=topk_ids.device)
    _hip.call("swl_moe_align", _hip.ptr(rows), _hip.ptr(experts), _hip.ptr(topk_ids), t, k, int(num_experts), tiles,
              _hip.stream())
    return rows, experts


def moe_up_gate_silu(x: torch.Tensor, expert_up_gate: torch.Tensor, tile_rows, tile_experts, top_k: int,
                     act: torch.Tensor = None) -> torch.Tensor:
    """x [T, H], expert_up_gate [E, 2 I, H] ([up ; gate] per expert) -> act [T k, I] = up * silu(gate) of every pair."""
    _hip.require_gpu_tensor(x, "x")
    e, two_i, h = expert_up_gate.shape
    assert x.dim() == 2 and x.shape[1] == h and x.stride(1) == 1 and x.dtype == expert_up_gate.dtype
    assert expert_up_gate.is_contiguous() and two_i % 2 == 0
    t, inter = x.shape[0], two_i // 2
    if act is None:
        act = torch.empty((t * top_k, inter), dtype=x.dtype, device=x.device)
    assert act.is_contiguous() and tuple(act.shape) == (t * top_k, inter) and act.dtype == x.dtype
    assert tile_rows.numel() == tile_experts.numel() * TILE_ROWS
    _hip.call("swl_moe_up_gate_silu", _hip.ptr(act), _hip.ptr(x), _hip.ptr(expert_up_gate), _hip.ptr(tile_rows),
              _hip.ptr(tile_experts), tile_experts.numel(), t, int(top_k), h, inter, e, x.stride(0),
              _hip.dtype_code(x.dtype), _hip.stream())
    return act


def moe_down(act: torch.Tensor, expert_down: torch.Tensor, tile_rows, tile_experts, top_k: int,
             y: torch.Tensor = None) -> torch.Tensor:
    """act [T k, I], expert_down [E, H, I] -> y fp32 [T k, H]: every pair's down projection, unrounded."""
    _hip.require_gpu_tensor(act, "act")
    e, h, inter = expert_down.shape
    assert act.dim() == 2 and act.shape[1] == inter and act.is_contiguous() and act.dtype == expert_down.dtype
    assert expert_down.is_contiguous() and act.shape[0] % top_k == 0
    pairs = act.shape[0]
    if y is None:
        y = torch.empty((pairs, h), dtype=torch.float32, device=act.device)
    assert y.is_contiguous() and tuple(y.shape) == (pairs, h) and y.dtype == torch.float32
    assert tile_rows.numel() == tile_experts.numel() * TILE_ROWS
    _hip.call("swl_moe_down", _hip.ptr(y), _hip.ptr(act), _hip.ptr(expert_down), _hip.ptr(tile_rows), _hip.ptr(tile_experts),
              tile_experts.numel(), pairs // top_k, int(top_k), h, inter, e, _hip.dtype_code(act.dtype), _hip.stream())
    return y


def moe_combine(y: torch.Tensor, topk_w: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[t] = T(sum_j topk_w[t, j] * y[t k + j]) in slot order: one rounding, no atomics."""
    _hip.require_gpu_tensor(y, "y")
    t, k = topk_w.shape
    h = y.shape[1]
    assert y.dtype == torch.float32 and y.is_contiguous() and y.shape[0] == t * k
    assert topk_w.dtype == torch.float32 and topk_w.is_contiguous()
    assert out.dim() == 2 and tuple(out.shape) == (t, h) and out.stride(1) == 1
    _hip.call("swl_moe_combine", _hip.ptr(out), _hip.ptr(y), _hip.ptr(topk_w), t, k, h, out.stride(0),
              _hip.dtype_code(out.dtype), _hip.stream())
    return out


def moe_ffn(x: torch.Tensor, router: torch.Tensor, expert_up_gate: torch.Tensor, expert_down: torch.Tensor, top_k: int,
            norm_topk_prob: bool, skinny: bool = False, tap=None, layer_id: int = 0) -> torch.Tensor:
    """The FFN of a mixture-of-experts layer on the normalised activations x [T, H]: a new [T, H] tensor. `tap` (tests): a
    list that receives (layer_id, topk_ids.cpu(), topk_w.cpu()) — a host copy, so a tapped step is never graph-captured."""
    t = x.shape[0]
    e = router.shape[0]
    out = torch.empty_like(x)
    if t == 0:
        return out
    logits = linear(x, router, skinny)
    block = max(1, max_pairs() // top_k)
    act = y = None
    tapped = []
    for t0 in range(0, t, block):
        n = min(block, t - t0)
        xs = x[t0:t0 + n]
        ids, w = moe_route(logits[t0:t0 + n], top_k, norm_topk_prob)
        rows, experts = moe_align(ids, e)
        if act is None or act.shape[0] != n * top_k:        # (a step's blocks share one workspace; the last may be shorter)
            act = y = None
        act = moe_up_gate_silu(xs, expert_up_gate, rows, experts, top_k, act)
        y = moe_down(act, expert_down, rows, experts, top_k, y)
        moe_combine(y, w, out[t0:t0 + n])
        if tap is not None:
            tapped.append((ids, w))
    if tap is not None:
        tap.append((layer_id, torch.cat([i for i, _ in tapped]).cpu(), torch.cat([w for _, w in tapped]).cpu()))
    return out
