"""Dense projections on MXFP4 weights in packed order (csrc/gemm_mxfp4.hip; the contract: csrc/gemm_mxfp4.h), bfloat16.

A projection is `codes` [N, K // 2] uint8 (two e2m1 codes a byte; the BYTES are in the packed order of the header, so
indexing the tensor by row and column means nothing) and `scales`, uint8 [scale_bytes(N, K)]: one e8m0 byte per 32 k of a
row, in lane order. N % 16 == 0, K % 128 == 0. The weight means e2m1(code) * 2^(byte - 127), exact in bfloat16.

  quantise_pack_rows      a 16-bit row-major [rows, K] tensor -> its packed codes and scales, written into a caller's
                          slices of a projection's codes and scales (16 rows are contiguous in both, so a fused projection's
                          tensors are quantised one by one into their places).
  linear_mxfp4            x @ W^T. Up to 64 rows: the weight-streaming kernel (each code byte read once). Beyond: the
                          projection is unpacked and dequantised into the scratch tensor of kernels/linear_fp8.py and the
                          existing `linear` multiplies it (hipBLASLt). 64 is the kernel's limit, not a tuned crossover.
  linear_silu_gate_mxfp4  up * silu(gate) over [up ; gate] codes, no [M, 2 I] intermediate up to 64 rows; beyond, the
                          dequantising route and swl_silu_mul.
  dequantise_mxfp4        out[N, K] = bfloat16(e2m1(code) * 2^e), row-major.
"""
import torch

from swiftllm_amd import _hip
from .linear import _row_stride, _workspace, linear
from .linear_fp8 import reserve_scratch
from .silu_and_mul import silu_and_mul_inplace

MAX_M = 64          # swl_gemm_mxfp4: four token tiles
MAX_SPLITS = 8
K_TILE = 128


def supported(n: int, k: int, dtype: torch.dtype = torch.bfloat16) -> bool:
    return bool(_hip.load().swl_gemm_mxfp4_supported(int(n), int(k), _hip.dtype_code(dtype)))


def choose_splits(n_out: int, k: int) -> int:
    return int(_hip.load().swl_gemm_mxfp4_choose_splits(int(n_out), int(k)))


def max_splits(k: int) -> int:
    """The largest split a caller may force: a power of two <= 8 and <= k / 128."""
    ks = 1
    while 2 * ks <= min(MAX_SPLITS, k // K_TILE):
        ks *= 2
    return ks


def scale_bytes(rows: int, k: int) -> int:
    """Bytes of the scales of `rows` (% 16 == 0) rows: 256 per row group and four k tiles."""
    return rows // 16 * ((k // K_TILE + 3) // 4) * 256


def _check(x, codes, scales):
    n, half = codes.shape
    k = 2 * half
    if codes.dtype != torch.uint8 or not codes.is_contiguous() or n % 16 or k % K_TILE:
        raise ValueError(f"codes must be contiguous uint8 [N % 16 == 0, K / 2 with K % 128 == 0], got {codes.dtype} {tuple(codes.shape)}")
    if scales.dtype != torch.uint8 or scales.numel() != scale_bytes(n, k) or not scales.is_contiguous() or scales.device != codes.device:
        raise ValueError(f"scales must be {scale_bytes(n, k)} contiguous uint8 next to the codes, got {scales.dtype} {tuple(scales.shape)}")
    if x is not None:
        _hip.require_gpu_tensor(x, "x")
        if x.dtype != torch.bfloat16:
            raise ValueError(f"MXFP4 projections multiply bfloat16 activations, got {x.dtype}")
        if x.dim() != 2 or x.shape[1] != k or x.stride(1) != 1:
            raise ValueError(f"x must be [M, {k}] with unit column stride, got {tuple(x.shape)}")
    return n, k


def quantise_pack_rows(w: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> None:
    """Packed codes and scales of the 16-bit `w` [rows, K] into `codes` (uint8, rows * K / 2 elements) and `scales` (uint8,
    scale_bytes(rows, K) elements), both contiguous: a whole projection, or the slices of rows [r, r + rows), r % 16 == 0,
    of a fused one."""
    _hip.require_gpu_tensor(w, "w")
    rows, k = w.shape
    if not w.is_contiguous() or rows % 16 or k % K_TILE:
        raise ValueError(f"w must be contiguous [rows % 16 == 0, K % 128 == 0], got {tuple(w.shape)}")
    for name, t, want in (("codes", codes, rows * k // 2), ("scales", scales, scale_bytes(rows, k))):
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != want or t.device != w.device:
            raise ValueError(f"{name} must be {want} contiguous uint8 next to w, got {t.dtype} {tuple(t.shape)}")
    _hip.call("swl_gemm_mxfp4_quantise_pack", _hip.ptr(codes), _hip.ptr(scales), _hip.ptr(w), rows, k, _hip.dtype_code(w.dtype),
              _hip.stream())


def dequantise_mxfp4(codes: torch.Tensor, scales: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    n, k = _check(None, codes, scales)
    if tuple(out.shape) != (n, k) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous [{n}, {k}], got {tuple(out.shape)}")
    _hip.call("swl_mxfp4_dequant", _hip.ptr(out), _hip.ptr(codes), _hip.ptr(scales), n, k, _hip.dtype_code(out.dtype),
              _hip.stream())
    return out


def dequantised(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The projection's 16-bit row-major image in the scratch: valid until the next call on the same card and dtype."""
    n, k = codes.shape[0], 2 * codes.shape[1]
    return dequantise_mxfp4(codes, scales, reserve_scratch(codes.device, dtype, n * k)[:n * k].view(n, k))


def linear_mxfp4(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, k_splits: int = 0) -> torch.Tensor:
    n, k = _check(x, codes, scales)
    m = x.shape[0]
    if m > MAX_M:
        return linear(x, dequantised(codes, scales, x.dtype))
    out = torch.empty((m, n), dtype=x.dtype, device=x.device)
    ks = k_splits or choose_splits(n, k)
    ws = _workspace(x.device, ks * m * n * 4) if ks > 1 and m else None
    _hip.call("swl_gemm_mxfp4", _hip.ptr(out), _hip.ptr(x), _hip.ptr(codes), _hip.ptr(scales), _hip.ptr(ws),
              ws.numel() * 4 if ws is not None else 0, m, n, k, _row_stride(x), k_splits, _hip.dtype_code(x.dtype), _hip.stream())
    return out


def linear_silu_gate_mxfp4(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, k_splits: int = 0) -> torch.Tensor:
    n, k = _check(x, codes, scales)
    if n % 32:
        raise ValueError(f"[up ; gate] codes have 2 I rows with I % 16 == 0, got {n}")
    m, inter = x.shape[0], n // 2
    if m > MAX_M:
        up_gate = linear(x, dequantised(codes, scales, x.dtype))
        silu_and_mul_inplace(up_gate)
        return up_gate[:, :inter]
    act = torch.empty((m, inter), dtype=x.dtype, device=x.device)
    ks = k_splits or choose_splits(inter, k)
    ws = _workspace(x.device, ks * m * n * 4) if ks > 1 and m else None
    _hip.call("swl_gemm_mxfp4_silu_gate", _hip.ptr(act), _hip.ptr(x), _hip.ptr(codes), _hip.ptr(scales), _hip.ptr(ws),
              ws.numel() * 4 if ws is not None else 0, m, inter, k, _row_stride(x), k_splits, _hip.dtype_code(x.dtype),
              _hip.stream())
    return act
