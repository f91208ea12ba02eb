"""Dense projections on block-scaled FP8 weights (csrc/gemm_fp8_block.hip; the storage contract: csrc/gemm_fp8_block.h).

A projection is `codes` [N, K] (torch.float8_e4m3fn: the checkpoint's own bytes), `bscale` fp32 [sum of ceil(rows_s / 128),
ceil(K / 128)] and `segments`, the row counts of the tensors it concatenates — (q, k, v), (up, gate) or (N,).

  linear_fp8_block            x @ W^T. Up to 64 rows: the weight-streaming FP8 kernel (each code byte read once). Beyond: the
                              projection is dequantised into ONE scratch tensor (sized for the largest projection asked for so
                              far, fixed address) and the existing `linear` multiplies it (hipBLASLt). 64 is the kernel's
                              limit, not a tuned crossover.
                              `wide=True` (the model passes it up to WIDE_ROUTED_MAX_M rows under
                              EngineConfig.dense_fp8_wide): 65..256 rows run the wide weight-streaming FP8 kernel
                              (csrc/gemm_fp8_block_wide.hip) instead; a row's bits are then the 64-row kernel's at the same split.
  linear_silu_gate_fp8_block  up * silu(gate) over [up ; gate] codes, no [M, 2 I] intermediate up to 64 rows; beyond, the
                              dequantising route and swl_silu_mul.
  dequantise_fp8_block        out[N, K] = T(fp32(code) * scale), bit-equal to worker/weight.py: dequantise_blocks.
  reserve_scratch, dequantised  the one scratch tensor of a card and dtype, and a projection's 16-bit image inside it.
"""
import torch

from swiftllm_amd import _hip
from .linear import _row_stride, _workspace, linear
from .silu_and_mul import silu_and_mul_inplace

FP8 = torch.float8_e4m3fn
BLOCK = 128
MAX_M = 64          # swl_gemm_fp8_block: four token tiles
WIDE_MAX_M = 256    # swl_gemm_fp8_block_wide: sixteen token tiles; what `wide=True` sends to it (the C entry's limit)
WIDE_ROUTED_MAX_M = 192     # what EngineConfig.dense_fp8_wide routes to it: at 256 rows up/gate loses to the dequantising route
MAX_SPLITS = 8
_scratch = {}       # (device, dtype) -> the 16-bit image of the projection being multiplied by the dequantising route
_retired = []       # outgrown ones stay allocated: captured hipGraphs may still replay against them


def blocks(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def scale_rows(segments) -> int:
    return sum(blocks(int(r)) for r in segments)


def supported(n: int, k: int, dtype: torch.dtype = torch.bfloat16) -> bool:
    return bool(_hip.load().swl_gemm_fp8_block_supported(int(n), int(k), _hip.dtype_code(dtype)))


def choose_splits(n_out: int, k: int) -> int:
    return int(_hip.load().swl_gemm_fp8_block_choose_splits(int(n_out), int(k)))


def choose_splits_wide(weight_rows: int, k: int) -> int:
    """The wide kernels' split for a launch that streams `weight_rows` rows of codes (N; 2 I for the SiLU-gate form)."""
    return int(_hip.load().swl_gemm_fp8_block_wide_choose_splits(int(weight_rows), int(k)))


def max_splits(k: int) -> int:
    """The largest split a caller may force: a power of two <= 8 and <= ceil(k / 128)."""
    ks = 1
    while 2 * ks <= min(MAX_SPLITS, blocks(k)):
        ks *= 2
    return ks


def _check(x, codes, bscale, segments):
    segments = tuple(int(r) for r in segments)
    if not 1 <= len(segments) <= 3:
        raise ValueError(f"a block-scaled projection has one to three segments, got {segments}")
    n, k = codes.shape
    if codes.dtype != FP8 or not codes.is_contiguous() or sum(segments) != n:
        raise ValueError(f"codes must be contiguous float8_e4m3fn [{sum(segments)}, K], got {codes.dtype} {tuple(codes.shape)}")
    want = (scale_rows(segments), blocks(k))
    if bscale.dtype != torch.float32 or tuple(bscale.shape) != want or not bscale.is_contiguous():
        raise ValueError(f"bscale must be contiguous float32 {want}, got {bscale.dtype} {tuple(bscale.shape)}")
    if x is not None:
        _hip.require_gpu_tensor(x, "x")
        if x.dim() != 2 or x.shape[1] != k or x.stride(1) != 1:
            raise ValueError(f"x must be [M, {k}] with unit column stride, got {tuple(x.shape)}")
    return segments + (0,) * (3 - len(segments)), n, k


def dequantise_fp8_block(codes: torch.Tensor, bscale: torch.Tensor, segments, out: torch.Tensor) -> torch.Tensor:
    seg, n, k = _check(None, codes, bscale, segments)
    if tuple(out.shape) != (n, k) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous [{n}, {k}], got {tuple(out.shape)}")
    _hip.call("swl_fp8_block_dequant", _hip.ptr(out), _hip.ptr(codes), _hip.ptr(bscale), *seg, k, bscale.shape[0],
              bscale.shape[1], _hip.dtype_code(out.dtype), _hip.stream())
    return out


def _scratch_key(device, dtype: torch.dtype) -> tuple:
    """One key per card: torch.device("cuda") and torch.device("cuda:0") are different objects with different hashes."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device, dtype


def reserve_scratch(device, dtype: torch.dtype, numel: int) -> torch.Tensor:
    """The dequantising route's scratch, holding at least `numel` elements (the model: its largest projection, once, at
    load, so that no step allocates it)."""
    key = _scratch_key(device, dtype)
    cur = _scratch.get(key)
    if cur is None or cur.numel() < numel:
        if cur is not None:
            _retired.append(cur)
        cur = _scratch[key] = torch.empty(numel, dtype=dtype, device=key[0])
    return cur


def dequantised(codes: torch.Tensor, bscale: torch.Tensor, segments, dtype: torch.dtype) -> torch.Tensor:
    """The projection's 16-bit image in the scratch: valid until the next call on the same card and dtype."""
    out = reserve_scratch(codes.device, dtype, codes.numel())[:codes.numel()].view(codes.shape)
    return dequantise_fp8_block(codes, bscale, segments, out)


def linear_fp8_block(x: torch.Tensor, codes: torch.Tensor, bscale: torch.Tensor, segments, k_splits: int = 0,
                     wide: bool = False) -> torch.Tensor:
    seg, n, k = _check(x, codes, bscale, segments)
    m = x.shape[0]
    use_wide = wide and MAX_M < m <= WIDE_MAX_M
    if m > MAX_M and not use_wide:
        return linear(x, dequantised(codes, bscale, segments, x.dtype))
    out = torch.empty((m, n), dtype=x.dtype, device=x.device)
    ks = k_splits or (choose_splits_wide(n, k) if use_wide else choose_splits(n, k))
    ws = _workspace(x.device, ks * m * n * 4) if ks > 1 and m else None
    _hip.call("swl_gemm_fp8_block_wide" if use_wide else "swl_gemm_fp8_block", _hip.ptr(out), _hip.ptr(x), _hip.ptr(codes),
              _hip.ptr(bscale), _hip.ptr(ws), ws.numel() * 4 if ws is not None else 0, m, *seg, k, bscale.shape[0], bscale.shape[1], _row_stride(x), k_splits,
              _hip.dtype_code(x.dtype), _hip.stream())
    return out


def linear_silu_gate_fp8_block(x: torch.Tensor, codes: torch.Tensor, bscale: torch.Tensor, inter: int,
                               k_splits: int = 0, wide: bool = False) -> torch.Tensor:
    inter = int(inter)
    _, n, k = _check(x, codes, bscale, (inter, inter))
    m = x.shape[0]
    use_wide = wide and MAX_M < m <= WIDE_MAX_M
    if m > MAX_M and not use_wide:
        up_gate = linear(x, dequantised(codes, bscale, (inter, inter), x.dtype))
        silu_and_mul_inplace(up_gate)
        return up_gate[:, :inter]
    act = torch.empty((m, inter), dtype=x.dtype, device=x.device)
    ks = k_splits or (choose_splits_wide(n, k) if use_wide else choose_splits(inter, k))
    ws = _workspace(x.device, ks * m * n * 4) if ks > 1 and m else None
    _hip.call("swl_gemm_fp8_block_wide_silu_gate" if use_wide else "swl_gemm_fp8_block_silu_gate", _hip.ptr(act),
              _hip.ptr(x), _hip.ptr(codes), _hip.ptr(bscale), _hip.ptr(ws), ws.numel() * 4 if ws is not None else 0, m, inter, k, bscale.shape[0], bscale.shape[1], _row_stride(x), k_splits,
              _hip.dtype_code(x.dtype), _hip.stream())
    return act
