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

Prompt-sized steps: csrc/moe_wide.hip holds a second form of the two expert GEMMs in which a workgroup serves up to
`row_tiles` (2 or 4) consecutive 16-row tiles of one expert with one pass over a block of its weights. It reads the same
tile tables and writes the same bits, so `moe_ffn` picks the form per token block from `wide_row_tiles` (host arithmetic on
(tokens, k, E, H, I): capture and replay agree) and a token's output does not depend on the choice. Still six launches.

FP8 expert weights (EngineConfig.moe_weight_dtype = "fp8_e4m3"; csrc/moe_fp8.h states the contract): the two stacks hold one
e4m3fn code per element and come with one fp32 scale per output row (`up_gate_scale` [E, 2 I], `down_scale` [E, H]).
`quantise_rows` is the loader's kernel; `moe_up_gate_silu` / `moe_down` / `moe_ffn` take the scales and call the FP8 entries
(both forms, the same tables, the same grids, the same six launches) whenever the stacks are 8-bit.

Block-scaled FP8 checkpoints (csrc/moe_fp8_block.h): the stacks hold the checkpoint's own codes and come with its own scales,
one fp32 per 128 x 128 block — `up_gate_bscale` [E, 2 ceil(I / 128), ceil(H / 128)] (up's row blocks, then gate's) and
`down_bscale` [E, ceil(H / 128), ceil(I / 128)]. The same three functions take them in place of the row scales and call the
block entries. Their row-tile form is built for 2 tiles only (4 do not fit a wave's registers): a `row_tiles` of 4 runs the
2-tile kernels, which write the same bits.
"""
import torch

from swiftllm_amd import _hip
from .linear import linear

TILE_ROWS = 16
LOGITS_F32 = 2      # SWL_MOE_LOGITS_F32
MAX_EXPERTS = 256
MAX_TOP_K = 16
WIDE_ROW_TILES = (2, 4)     # what swl_moe_*_wide take
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
BLOCK = 128         # rows and k one scale of a block-scaled FP8 checkpoint covers
BLOCK_WIDE_ROW_TILES = 2    # what swl_moe_*_fp8_block_wide take


def supported(hidden: int, inter: int, num_experts: int, top_k: int, dtype: torch.dtype = torch.bfloat16) -> bool:
    """Whether the expert GEMMs take the geometry (host arithmetic only): hidden % 64 == 0, inter % 32 == 0, at most 256
    experts, top-k at most 16 and at most the expert count."""
    return bool(_hip.load().swl_moe_supported(int(hidden), int(inter), int(num_experts), int(top_k), _hip.dtype_code(dtype)))


def fp8_supported(hidden: int, inter: int, num_experts: int, top_k: int, dtype: torch.dtype = torch.bfloat16) -> bool:
    """Whether the FP8 expert GEMMs take the geometry: `supported` with hidden % 64 == 0 and inter % 64 == 0."""
    return bool(_hip.load().swl_moe_fp8_supported(int(hidden), int(inter), int(num_experts), int(top_k),
                                                  _hip.dtype_code(dtype)))


def fp8_block_supported(hidden: int, inter: int, num_experts: int, top_k: int, dtype: torch.dtype = torch.bfloat16) -> bool:
    """Whether the block-scaled FP8 expert GEMMs take the geometry: that of `fp8_supported`."""
    return bool(_hip.load().swl_moe_fp8_block_supported(int(hidden), int(inter), int(num_experts), int(top_k),
                                                        _hip.dtype_code(dtype)))


def row_scales(w: torch.Tensor):
    """(scale, inv) fp32 [rows] of a 16-bit [rows, K] tensor, on its device: scale = max |w_row| / 448 (a zero row: 1),
    inv = 1 / scale. The row maxima are exact wherever they are taken; the two divisions are done on the HOST (IEEE
    division, one rounding each — a device's division need not be), which is what makes the codes reproducible there."""
    amax = w.abs().amax(dim=1).float().cpu()
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    return scale.to(w.device), (1.0 / scale).to(w.device)


def quantise_rows(w: torch.Tensor, inv: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    """codes[r] = e4m3(clamp(fp32(w[r]) * inv[r], -448, 448)): w [rows, K] float16 / bfloat16, K % 16 == 0, inv fp32 [rows],
    codes [rows, K] float8_e4m3fn (a contiguous slice of a stack), written in place."""
    _hip.require_gpu_tensor(w, "w")
    rows, k = w.shape
    assert w.is_contiguous() and codes.is_contiguous() and tuple(codes.shape) == (rows, k) and codes.dtype == FP8
    assert inv.dtype == torch.float32 and inv.is_contiguous() and inv.numel() == rows
    _hip.call("swl_moe_quantise_rows", _hip.ptr(codes), _hip.ptr(w), _hip.ptr(inv), rows, k, _hip.dtype_code(w.dtype),
              _hip.stream())
    return codes


def _fp8_scale(stack: torch.Tensor, scale, name: str) -> tuple:
    """() for a 16-bit stack; (pointer of its row scales,) for an FP8 one."""
    if stack.dtype != FP8:
        assert scale is None, f"{name} is for FP8 stacks"
        return ()
    assert scale is not None and scale.dtype == torch.float32 and scale.is_contiguous(), f"FP8 stacks need {name}"
    assert tuple(scale.shape) == tuple(stack.shape[:2]) and scale.device == stack.device
    return (_hip.ptr(scale),)


def block_scales_shape(rows: int, k: int) -> tuple:
    """(row blocks, k blocks) of a [rows, k] projection's block scales: a checkpoint's weight_scale_inv shape."""
    return (rows + BLOCK - 1) // BLOCK, (k + BLOCK - 1) // BLOCK


def _fp8_block_scale(stack: torch.Tensor, bscale: torch.Tensor, halves: int, name: str) -> tuple:
    """(pointer, row blocks, k blocks) of the block scales of an FP8 stack [E, halves * rows, k]."""
    e, rows, k = stack.shape
    rb, kb = block_scales_shape(rows // halves, k)
    assert stack.dtype == FP8, f"{name} is for FP8 stacks"
    assert bscale.dtype == torch.float32 and bscale.is_contiguous() and bscale.device == stack.device
    assert tuple(bscale.shape) == (e, halves * rb, kb), f"{name} must be {(e, halves * rb, kb)}, got {tuple(bscale.shape)}"
    return _hip.ptr(bscale), rb, kb


def max_pairs() -> int:
    """(token, expert) pairs one call of the kernels takes."""
    return int(_hip.load().swl_moe_max_pairs())


def max_tiles(num_tokens: int, top_k: int, num_experts: int) -> int:
    """ceil(T k / 16) + min(E, T k): the tiles an alignment of the step can need."""
    return int(_hip.load().swl_moe_max_tiles(int(num_tokens), int(top_k), int(num_experts)))


def wide_row_tiles(num_tokens: int, top_k: int, num_experts: int, hidden: int, inter: int) -> int:
    """The form a call of this step should take: 0 = the 16-row kernels, else the `row_tiles` of the wide ones. 0 for
    num_tokens <= 32 and wherever num_tokens * top_k / num_experts < 32."""
    return int(_hip.load().swl_moe_wide_row_tiles(int(num_tokens), int(top_k), int(num_experts), int(hidden), int(inter)))


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
                     act: torch.Tensor = None, row_tiles: int = 0, up_gate_scale: torch.Tensor = None,
                     up_gate_bscale: torch.Tensor = None) -> torch.Tensor:
    """x [T, H], expert_up_gate [E, 2 I, H] ([up ; gate] per expert) -> act [T k, I] = up * silu(gate) of every pair.
    `row_tiles` > 0: the wide form (same bits). An FP8 stack comes with `up_gate_scale` fp32 [E, 2 I], or — a block-scaled
    checkpoint's — with `up_gate_bscale` fp32 [E, 2 ceil(I / 128), ceil(H / 128)]."""
    _hip.require_gpu_tensor(x, "x")
    e, two_i, h = expert_up_gate.shape
    block = up_gate_bscale is not None
    if block:
        assert up_gate_scale is None, "one kind of scales"
        scale = _fp8_block_scale(expert_up_gate, up_gate_bscale, 2, "up_gate_bscale")
        row_tiles = min(int(row_tiles), BLOCK_WIDE_ROW_TILES)
    else:
        scale = _fp8_scale(expert_up_gate, up_gate_scale, "up_gate_scale")
    assert x.dim() == 2 and x.shape[1] == h and x.stride(1) == 1 and (scale or x.dtype == expert_up_gate.dtype)
    assert expert_up_gate.is_contiguous() and two_i % 2 == 0
    t, inter = x.shape[0], two_i // 2
    if act is None:
        act = torch.empty((t * top_k, inter), dtype=x.dtype, device=x.device)
    assert act.is_contiguous() and tuple(act.shape) == (t * top_k, inter) and act.dtype == x.dtype
    assert tile_rows.numel() == tile_experts.numel() * TILE_ROWS
    wide = (int(row_tiles),) if row_tiles > 0 else ()
    name = "swl_moe_up_gate_silu" + ("_fp8" if scale else "") + ("_block" if block else "") + ("_wide" if wide else "")
    _hip.call(name, _hip.ptr(act), _hip.ptr(x), _hip.ptr(expert_up_gate), *scale, _hip.ptr(tile_rows),
              _hip.ptr(tile_experts), tile_experts.numel(), t, int(top_k), h, inter, e, x.stride(0), *wide,
              _hip.dtype_code(x.dtype), _hip.stream())
    return act


def moe_down(act: torch.Tensor, expert_down: torch.Tensor, tile_rows, tile_experts, top_k: int,
             y: torch.Tensor = None, row_tiles: int = 0, down_scale: torch.Tensor = None,
             down_bscale: torch.Tensor = None) -> torch.Tensor:
    """act [T k, I], expert_down [E, H, I] -> y fp32 [T k, H]: every pair's down projection, unrounded. `row_tiles` > 0:
    the wide form (same bits). An FP8 stack comes with `down_scale` fp32 [E, H], or — a block-scaled checkpoint's — with
    `down_bscale` fp32 [E, ceil(H / 128), ceil(I / 128)]."""
    _hip.require_gpu_tensor(act, "act")
    e, h, inter = expert_down.shape
    block = down_bscale is not None
    if block:
        assert down_scale is None, "one kind of scales"
        scale = _fp8_block_scale(expert_down, down_bscale, 1, "down_bscale")
        row_tiles = min(int(row_tiles), BLOCK_WIDE_ROW_TILES)
    else:
        scale = _fp8_scale(expert_down, down_scale, "down_scale")
    assert act.dim() == 2 and act.shape[1] == inter and act.is_contiguous() and (scale or act.dtype == expert_down.dtype)
    assert expert_down.is_contiguous() and act.shape[0] % top_k == 0
    pairs = act.shape[0]
    if y is None:
        y = torch.empty((pairs, h), dtype=torch.float32, device=act.device)
    assert y.is_contiguous() and tuple(y.shape) == (pairs, h) and y.dtype == torch.float32
    assert tile_rows.numel() == tile_experts.numel() * TILE_ROWS
    wide = (int(row_tiles),) if row_tiles > 0 else ()
    name = "swl_moe_down" + ("_fp8" if scale else "") + ("_block" if block else "") + ("_wide" if wide else "")
    _hip.call(name, _hip.ptr(y), _hip.ptr(act), _hip.ptr(expert_down), *scale, _hip.ptr(tile_rows), _hip.ptr(tile_experts),
              tile_experts.numel(), pairs // top_k, int(top_k), h, inter, e, *wide, _hip.dtype_code(act.dtype),
              _hip.stream())
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
            norm_topk_prob: bool, skinny: bool = False, tap=None, layer_id: int = 0, wide_tiles: int = -1,
            up_gate_scale: torch.Tensor = None, down_scale: torch.Tensor = None, up_gate_bscale: torch.Tensor = None,
            down_bscale: torch.Tensor = None) -> torch.Tensor:
    """The FFN of a mixture-of-experts layer on the normalised activations x [T, H]: a new [T, H] tensor. `tap` (tests): a
    list that receives (layer_id, topk_ids.cpu(), topk_w.cpu()) — a host copy, so a tapped step is never graph-captured.
    `wide_tiles`: -1 = `wide_row_tiles` decides the form of the expert GEMMs per token block, 0 = always the 16-row
    kernels, 2 / 4 = always the wide ones with that many row tiles (the bits are the same either way). FP8 stacks come with
    `up_gate_scale` / `down_scale` (per row) or `up_gate_bscale` / `down_bscale` (per 128 x 128 block) and take the FP8
    entries of both forms."""
    if wide_tiles not in (-1, 0) + WIDE_ROW_TILES:
        raise ValueError(f"wide_tiles must be -1 (choose), 0 (16-row) or one of {list(WIDE_ROW_TILES)}, got {wide_tiles}")
    t = x.shape[0]
    e = router.shape[0]
    h, inter = expert_down.shape[1], expert_down.shape[2]
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
        form = wide_row_tiles(n, top_k, e, h, inter) if wide_tiles < 0 else wide_tiles
        act = moe_up_gate_silu(xs, expert_up_gate, rows, experts, top_k, act, form, up_gate_scale, up_gate_bscale)
        y = moe_down(act, expert_down, rows, experts, top_k, y, form, down_scale, down_bscale)
        moe_combine(y, w, out[t0:t0 + n])
        if tap is not None:
            tapped.append((ids, w))
    if tap is not None:
        tap.append((layer_id, torch.cat([i for i, _ in tapped]).cpu(), torch.cat([w for _, w in tapped]).cpu()))
    return out
