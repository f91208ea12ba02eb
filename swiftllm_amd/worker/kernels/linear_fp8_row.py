"""Dense projections on per-row FP8 weights in packed order (csrc/gemm_fp8_row.hip; the contract: csrc/gemm_fp8_row.h).

A projection is `codes` [N, K] (torch.float8_e4m3fn; the BYTES are in the packed order of the header, so indexing the tensor
by row and column means nothing) and `scale` fp32 [N], one per output row. N % 16 == 0, K % 64 == 0.

  quantise_pack_rows        a 16-bit row-major [rows, K] tensor -> its packed codes, written into a caller's slice of a
                            projection's codes (16 rows of codes are 16 K contiguous bytes, so a fused projection's tensors
                            are quantised one by one into their places); returns the row scales.
  linear_fp8_row            x @ W^T. Up to 64 rows: the weight-streaming FP8 kernel (each code byte read once). Beyond: the
                            projection is unpacked and dequantised into the scratch tensor of kernels/linear_fp8.py and the
                            existing `linear` multiplies it (hipBLASLt). 64 is the kernel's limit, not a tuned crossover.
  linear_silu_gate_fp8_row  up * silu(gate) over [up ; gate] codes, no [M, 2 I] intermediate up to 64 rows; beyond, the
                            dequantising route and swl_silu_mul.
  dequantise_fp8_row        out[N, K] = T(fp32(code) * scale[row]), row-major.
"""
import torch

from swiftllm_amd import _hip
from .linear import _row_stride, _workspace, linear
from .linear_fp8 import reserve_scratch
from .moe import row_scales
from .silu_and_mul import silu_and_mul_inplace

FP8 = torch.float8_e4m3fn
MAX_M = 64          # swl_gemm_fp8_row: four token tiles
MAX_SPLITS = 8


def supported(n: int, k: int, dtype: torch.dtype = torch.bfloat16) -> bool:
    return bool(_hip.load().swl_gemm_fp8_row_supported(int(n), int(k), _hip.dtype_code(dtype)))


def choose_splits(n_out: int, k: int) -> int:
    return int(_hip.load().swl_gemm_fp8_row_choose_splits(int(n_out), int(k)))


def max_splits(k: int) -> int:
    """The largest split a caller may force: a power of two <= 8 and <= k / 64."""
    ks = 1
    while 2 * ks <= min(MAX_SPLITS, k // 64):
        ks *= 2
    return ks


def _check(x, codes, scale):
    n, k = codes.shape
    if codes.dtype != FP8 or not codes.is_contiguous() or n % 16 or k % 64:
        raise ValueError(f"codes must be contiguous float8_e4m3fn [N % 16 == 0, K % 64 == 0], got {codes.dtype} {tuple(codes.shape)}")
    if scale.dtype != torch.float32 or tuple(scale.shape) != (n,) or not scale.is_contiguous() or scale.device != codes.device:
        raise ValueError(f"scale must be contiguous float32 ({n},) next to the codes, got {scale.dtype} {tuple(scale.shape)}")
    if x is not None:
        _hip.require_gpu_tensor(x, "x")
        if x.dim() != 2 or x.shape[1] != k or x.stride(1) != 1:
            raise ValueError(f"x must be [M, {k}] with unit column stride, got {tuple(x.shape)}")
    return n, k


def quantise_pack_rows(w: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    """Packed codes of the 16-bit `w` [rows, K] into `codes` (float8_e4m3fn, rows * K elements, contiguous: a whole
    projection or rows [r, r + rows), r % 16 == 0, of a fused one); returns scale fp32 [rows]."""
    _hip.require_gpu_tensor(w, "w")
    rows, k = w.shape
    if not w.is_contiguous() or rows % 16 or k % 64:
        raise ValueError(f"w must be contiguous [rows % 16 == 0, K % 64 == 0], got {tuple(w.shape)}")
    if codes.dtype != FP8 or not codes.is_contiguous() or codes.numel() != rows * k or codes.device != w.device:
        raise ValueError(f"codes must be {rows * k} contiguous float8_e4m3fn next to w, got {codes.dtype} {tuple(codes.shape)}")
    scale, inv = row_scales(w)
    _hip.call("swl_gemm_fp8_row_quantise_pack", _hip.ptr(codes), _hip.ptr(w), _hip.ptr(inv), rows, k, _hip.dtype_code(w.dtype),
              _hip.stream())
    return scale


def dequantise_fp8_row(codes: torch.Tensor, scale: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    n, k = _check(None, codes, scale)
    if tuple(out.shape) != (n, k) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous [{n}, {k}], got {tuple(out.shape)}")
    _hip.call("swl_fp8_row_dequant", _hip.ptr(out), _hip.ptr(codes), _hip.ptr(scale), n, k, _hip.dtype_code(out.dtype),
              _hip.stream())
    return out


def dequantised(codes: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The projection's 16-bit row-major image in the scratch: valid until the next call on the same card and dtype."""
    out = reserve_scratch(codes.device, dtype, codes.numel())[:codes.numel()].view(codes.shape)
    return dequantise_fp8_row(codes, scale, out)


def linear_fp8_row(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, k_splits: int = 0) -> torch.Tensor:
    n, k = _check(x, codes, scale)
    m = x.shape[0]
    if m > MAX_M:
        return linear(x, dequantised(codes, scale, x.dtype))
    out = torch.empty((m, n), dtype=x.dtype, device=x.device)
    ks = k_splits or choose_splits(n, k)
    ws = _workspace(x.device, ks * m * n * 4) if ks > 1 and m else None
    _hip.call("swl_gemm_fp8_row", _hip.ptr(out), _hip.ptr(x), _hip.ptr(codes), _hip.ptr(scale), _hip.ptr(ws),
              ws.numel() * 4 if ws is not None else 0, m, n, k, _row_stride(x), k_splits, _hip.dtype_code(x.dtype), _hip.stream())
    return out


def linear_silu_gate_fp8_row(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, k_splits: int = 0) -> torch.Tensor:
    n, k = _check(x, codes, scale)
    if n % 32:
        raise ValueError(f"[up ; gate] codes have 2 I rows with I % 16 == 0, got {n}")
    m, inter = x.shape[0], n // 2
    if m > MAX_M:
        up_gate = linear(x, dequantised(codes, scale, x.dtype))
        silu_and_mul_inplace(up_gate)
        return up_gate[:, :inter]
    act = torch.empty((m, inter), dtype=x.dtype, device=x.device)
    ks = k_splits or choose_splits(inter, k)
    ws = _workspace(x.device, ks * m * n * 4) if ks > 1 and m else None
    _hip.call("swl_gemm_fp8_row_silu_gate", _hip.ptr(act), _hip.ptr(x), _hip.ptr(codes), _hip.ptr(scale), _hip.ptr(ws),
              ws.numel() * 4 if ws is not None else 0, m, inter, k, _row_stride(x), k_splits, _hip.dtype_code(x.dtype),
              _hip.stream())
    return act
