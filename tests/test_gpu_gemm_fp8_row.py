"""Per-row FP8 dense projections in packed order (csrc/gemm_fp8_row.h, gemm_fp8_row.hip, kernels/linear_fp8_row.py), float16
and bfloat16. The packed order is restated here from the header's formula, the numbers from its torch twin.

GEMM bound, derived: every product of a 16-bit activation and an e4m3 code is exact in fp32, so the fp32 accumulation of K
products and k_splits - 1 slab adds errs by at most e1 = (K + k_splits) 2^-24 scale sum |x_k code_k| in any order; the multiply
by the scale adds 2^-24 |y| and the rounding to T u_T |y| (u_T = 2^-8 bfloat16, 2^-11 float16), |y| <= |ref| + e1. The
SiLU-gate form takes the bound tests/test_gpu_gemm_fp8_block.py applies to its own, with a = e1 + 2^-24 |ref|."""
import pytest
import torch

from swiftllm_amd.worker.kernels import linear_fp8_row as L
from swiftllm_amd.worker.kernels.moe import row_scales

import _moe_ref as R
from test_gpu_moe_fp8 import bits

pytestmark = pytest.mark.gpu

DEV, DTYPES = "cuda", [torch.float16, torch.bfloat16]
SHAPES = [(16, 64), (48, 192), (80, 576)]
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
_W = {}


def weights(N, K, dtype):
    """(w 16-bit, packed codes, scale, the row-major code bytes read through the header's formula) — with a zero row and a row
    whose largest element is its last."""
    if (N, K, dtype) not in _W:
        w = (torch.randn((N, K), generator=torch.Generator().manual_seed(7 * N + K)) * 0.05).to(dtype)
        w[3] = 0
        w[N - 1, K - 1] = 1.5
        w = w.to(DEV)
        codes = torch.empty((N, K), dtype=L.FP8, device=DEV)
        scale = L.quantise_pack_rows(w, codes)
        n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
        byte = 1024 * ((n // 16) * (K // 64) + k // 64) + 16 * (16 * ((k % 64) // 16) + n % 16) + k % 16
        _W[(N, K, dtype)] = (w, codes, scale, codes.view(torch.uint8).flatten()[byte.to(DEV)])
    return _W[(N, K, dtype)]


def splits_of(K):
    return sorted({1, min(2, L.max_splits(K)), L.max_splits(K)})


def reference(x, N, K, dtype):
    """fp64 (ref, e1 per unit of K + k_splits) on the CPU."""
    _, _, scale, raw = weights(N, K, dtype)
    code, s = raw.view(L.FP8).double().cpu(), scale.double().cpu()
    return x.double() @ (code * s[:, None]).T, 2.0 ** -24 * (x.double().abs() @ code.abs().T) * s[None, :]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N, K", SHAPES)
def test_quantise_pack_and_unpack_are_the_torch_twin_bit_for_bit(N, K, dtype):
    w, codes, scale, raw = weights(N, K, dtype)
    want_scale, inv = row_scales(w)
    twin = w.float().mul(inv[:, None]).clamp(-448, 448).to(L.FP8)
    assert torch.equal(scale, want_scale) and float(scale[3]) == 1.0 and torch.equal(raw, twin.view(torch.uint8))
    got = L.dequantise_fp8_row(codes, scale, torch.empty((N, K), dtype=dtype, device=DEV))
    assert torch.equal(bits(got), bits((twin.float() * scale[:, None]).to(dtype)))
    assert not got[3].any() and float(got[N - 1, K - 1]) == 1.5


@pytest.mark.parametrize("M", [1, 15, 17, 33, 64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N, K", SHAPES)
def test_every_element_meets_the_derived_bound(N, K, dtype, M):
    _, codes, scale, _ = weights(N, K, dtype)
    wide = torch.randn((M, K + 8), generator=torch.Generator().manual_seed(600 + M + K)).to(dtype)
    x = wide[:, :K]                                         # M = 17: launched with x_row_stride = K + 8
    ref, unit = reference(x, N, K, dtype)
    xg = wide.to(DEV)[:, :K] if M == 17 else x.contiguous().to(DEV)
    for ks in splits_of(K):
        e1 = (K + ks) * unit
        got = L.linear_fp8_row(xg, codes, scale, k_splits=ks).cpu().double()
        worst = float(((got - ref).abs() / (e1 + (2.0 ** -24 + U[dtype]) * (ref.abs() + e1)).clamp(min=1e-300)).max())   # (a zero row: 0 / tiny)
        print(f"\n[gemm N={N} K={K} M={M} ks={ks} {dtype}] error / bound {worst:.3f}")
        assert float(got.abs().max()) > 0 and worst <= 1.0, (N, K, M, ks, worst)


@pytest.mark.parametrize("M", [1, 15, 17, 33, 64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inter, K", [(16, 64), (48, 576)])
def test_silu_gate_form_meets_the_block_form_s_bound(inter, K, dtype, M):
    _, codes, scale, _ = weights(2 * inter, K, dtype)
    x = torch.randn((M, K), generator=torch.Generator().manual_seed(700 + M + K)).to(dtype)
    ref, unit = reference(x, 2 * inter, K, dtype)
    h = lambda v: 0.5 * R.ulp_of(v, dtype)                  # noqa: E731
    for ks in splits_of(K):
        a = (K + ks) * unit + 2.0 ** -24 * ref.abs()
        act = L.linear_silu_gate_fp8_row(x.to(DEV), codes, scale, k_splits=ks).cpu().double()
        (up, gate), (au, ag) = (ref[:, :inter], ref[:, inter:]), (a[:, :inter], a[:, inter:])
        du, dg, s = au + h(up.abs() + au), ag + h(gate.abs() + ag), R.silu(gate)
        ds = 1.1 * dg + 2.0 ** -21 * s.abs() + h(s.abs() + 1.1 * dg)
        e = up.abs() * ds + s.abs() * du + du * ds
        worst = float(((act - up * s).abs() / (e + h((up * s).abs() + e))).max())
        print(f"\n[silu_gate I={inter} K={K} M={M} ks={ks} {dtype}] error / bound {worst:.3f}")
        assert float(act.abs().max()) > 0 and worst <= 1.0, (inter, K, M, ks, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N, K", SHAPES[1:] + [(96, 576)])     # (96 = [up ; gate] of I = 48)
def test_a_row_has_the_same_bits_alone_and_in_a_batch(N, K, dtype):
    _, codes, scale, _ = weights(N, K, dtype)
    x = torch.randn((64, K), generator=torch.Generator().manual_seed(61)).to(dtype).to(DEV)
    forms = [L.linear_fp8_row] + ([L.linear_silu_gate_fp8_row] if N % 32 == 0 else [])
    for form in forms:
        for ks in splits_of(K):
            full = form(x, codes, scale, k_splits=ks)
            for t in (0, 16, 63):
                assert torch.equal(bits(form(x[t:t + 1], codes, scale, k_splits=ks)), bits(full[t:t + 1])), (ks, t)
