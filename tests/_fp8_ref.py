"""The torch reference of the FP8 (OCP e4m3fn) KV-cache storage contract (include/swiftllm_hip.h, csrc/fp8_kv.h).

    quantise    codes = (x.float() * inv).clamp(-448, 448).to(torch.float8_e4m3fn)      inv = fp32(1 / scale), on the host
    dequantise  value = code (exact in float16 and bfloat16) * scale

torch's conversion rounds to nearest even and handles the e4m3 subnormals; beyond +-448 it yields NaN, hence the clamp
first (the kernels clamp explicitly as well). tests/test_kv_fp8_host.py checks all of that on the CPU.
"""
import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def inv_scale(scale: torch.Tensor) -> torch.Tensor:
    """fp32(1 / scale): what LlamaModel.set_kv_scales keeps next to the scales."""
    return 1.0 / scale.to(torch.float32)


def quantise(x: torch.Tensor, inv) -> torch.Tensor:
    """x (any float dtype) * inv (python float or broadcastable fp32 tensor) -> e4m3fn codes, the bit-exact reference."""
    inv = torch.as_tensor(inv, dtype=torch.float32)
    return x.float().mul(inv).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def codes(x8: torch.Tensor) -> torch.Tensor:
    return x8.view(torch.uint8)


def dequantise(x8: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """The value of every code in `dtype` (exact for float16 / bfloat16 / float32 / float64), without the scale."""
    return x8.to(torch.float32).to(dtype)


def stored(x: torch.Tensor, scale) -> torch.Tensor:
    """fp64 values a reader of the pool sees for x stored under `scale` (broadcastable): code * scale."""
    scale = torch.as_tensor(scale, dtype=torch.float32)
    return dequantise(quantise(x, inv_scale(scale))) * scale.double()


def fake_quant(x: torch.Tensor, scale=1.0) -> torch.Tensor:
    """dequant(quant(x)) rounded back to x's dtype (exact when scale == 1)."""
    scale = torch.as_tensor(scale, dtype=torch.float32)
    return (dequantise(quantise(x, inv_scale(scale)), torch.float32) * scale).to(x.dtype)
