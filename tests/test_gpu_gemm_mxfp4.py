"""MXFP4 dense projections in packed order (csrc/gemm_mxfp4.h, gemm_mxfp4.hip, kernels/linear_mxfp4.py), bfloat16. The packed
orders are restated here from the header's byte formulas, the numbers from a torch twin written from the e2m1 grid.

GEMM bound, derived: every product of a bfloat16 activation and an MX value is exact in fp32, so the fp32 accumulation of K
products and k_splits - 1 slab adds errs by at most e1 = (K + k_splits) 2^-24 sum |x_k w_k| in any order, and the rounding to
bfloat16 adds 2^-8 |y|, |y| <= |ref| + e1. The SiLU-gate form takes tests/test_gpu_gemm_fp8_row.py's bound with a = e1."""
import pytest
import torch

from swiftllm_amd.worker.kernels import linear_mxfp4 as L

import _moe_ref as R
from test_gpu_moe_fp8 import bits

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16
SHAPES = [(16, 128), (48, 384), (80, 1152)]
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
_W = {}


def twin(w):
    """(value fp32 [N, K], scale byte [N, K / 32]) of the contract, in torch."""
    blocks = w.float().view(w.shape[0], -1, 32)
    amax = blocks.abs().amax(dim=2)
    e = torch.where(amax > 0, (torch.frexp(amax)[1] - 3).clamp(-126, 127), torch.zeros((), dtype=torch.int32))
    a = torch.ldexp(blocks, -e[:, :, None]).abs()
    d = (a[..., None] - GRID).abs()
    lo = d.argmin(dim=3).clamp(max=6)                       # the lower of the two nearest codes
    pair = torch.gather(d, 3, torch.stack((lo, lo + 1), dim=3))
    code = lo + ((pair[..., 1] < pair[..., 0]) | ((pair[..., 1] == pair[..., 0]) & (lo % 2 == 1)))      # a tie: the even code
    value = torch.ldexp(GRID[code] * torch.sign(blocks), e[:, :, None])
    return value.view(w.shape), (e + 127).to(torch.uint8)


def weights(N, K):
    """(w, packed codes, packed scales, decoded values and scale bytes read through the header's byte formulas, the twin's)."""
    if (N, K) not in _W:
        w = (torch.randn((N, K), generator=torch.Generator().manual_seed(7 * N + K)) * 0.05).to(BF)
        w[3] = 0                                            # a zero row
        w[5, 64:96] = w[5, 64:96].clamp(-0.1, 0.1)
        w[5, 95] = 0.75                                     # a block whose largest element is its last
        w[7, 32:64] = w[7, 32:64].clamp(-0.1, 0.1)
        w[7, 40] = 0.21875                                  # 1.75 * 2^-3: e = -5, w / 2^e = 7, saturates at 6
        wg = w.to(DEV)
        codes = torch.empty((N, K // 2), dtype=torch.uint8, device=DEV)
        scales = torch.empty((L.scale_bytes(N, K),), dtype=torch.uint8, device=DEV)
        L.quantise_pack_rows(wg, codes, scales)
        n, k, KT = torch.arange(N)[:, None], torch.arange(K)[None, :], K // 128
        byte = 1024 * ((n // 16) * KT + k // 128) + 16 * (16 * ((k % 128) // 32) + n % 16) + (k % 32) // 2
        nib = (codes.cpu().flatten()[byte] >> (4 * (k % 2))) & 15
        sbyte = 256 * ((n // 16) * ((KT + 3) // 4) + k // 512) + 4 * (16 * ((k % 128) // 32) + n % 16) + (k // 128) % 4
        sc = scales.cpu()[sbyte]
        value = torch.ldexp(GRID[nib & 7] * (1 - 2 * (nib >> 3).float()), sc.int() - 127)
        _W[(N, K)] = (wg, codes, scales, value, sc[:, ::32], twin(w))
    return _W[(N, K)]


splits_of = lambda K: sorted({1, min(2, L.max_splits(K)), L.max_splits(K)})       # noqa: E731


def reference(x, N, K):
    """fp64 (ref, e1 per unit of K + k_splits) on the CPU."""
    wd = weights(N, K)[3].double()
    return x.double() @ wd.T, 2.0 ** -24 * (x.double().abs() @ wd.abs().T)


@pytest.mark.parametrize("N, K", SHAPES)
def test_quantise_pack_and_unpack_are_the_torch_twin_bit_for_bit(N, K):
    w, codes, scales, value, sc, (want, want_sc) = weights(N, K)
    assert torch.equal(sc, want_sc) and torch.equal(value, want) and int(sc.min()) >= 1 and int(sc.max()) <= 254
    assert int(sc[3].min()) == 127 and not value[3].any() and float(value[5, 95]) == 0.75 and float(value[7, 40]) == 0.1875
    if (K // 128) % 4:                                      # entries past KT are 127
        assert bool((scales.cpu().view(N // 16, -1, 64, 4)[:, -1, :, (K // 128) % 4:] == 127).all())
    got = L.dequantise_mxfp4(codes, scales, torch.empty((N, K), dtype=BF, device=DEV))
    assert torch.equal(got.cpu().float(), want) and torch.equal(bits(got).cpu(), bits(want.to(BF)))


@pytest.mark.parametrize("M", [1, 15, 17, 33, 64])
@pytest.mark.parametrize("N, K", SHAPES)
def test_every_element_meets_the_derived_bound(N, K, M):
    _, codes, scales = weights(N, K)[:3]
    wide = torch.randn((M, K + 8), generator=torch.Generator().manual_seed(600 + M + K)).to(BF)
    x = wide[:, :K]                                         # M = 17: launched with x_row_stride = K + 8
    ref, unit = reference(x, N, K)
    xg = wide.to(DEV)[:, :K] if M == 17 else x.contiguous().to(DEV)
    for ks in splits_of(K):
        e1 = (K + ks) * unit
        got = L.linear_mxfp4(xg, codes, scales, k_splits=ks).cpu().double()
        worst = float(((got - ref).abs() / (e1 + 2.0 ** -8 * (ref.abs() + e1)).clamp(min=1e-300)).max())   # (a zero row: 0 / tiny)
        print(f"\n[gemm N={N} K={K} M={M} ks={ks}] error / bound {worst:.3f}")
        assert float(got.abs().max()) > 0 and worst <= 1.0, (N, K, M, ks, worst)


@pytest.mark.parametrize("M", [1, 15, 17, 33, 64])
@pytest.mark.parametrize("inter, K", [(16, 128), (48, 1152)])
def test_silu_gate_form_meets_the_row_form_s_bound(inter, K, M):
    _, codes, scales = weights(2 * inter, K)[:3]
    x = torch.randn((M, K), generator=torch.Generator().manual_seed(700 + M + K)).to(BF)
    ref, unit = reference(x, 2 * inter, K)
    h = lambda v: 0.5 * R.ulp_of(v, BF)                     # noqa: E731
    for ks in splits_of(K):
        a = (K + ks) * unit
        act = L.linear_silu_gate_mxfp4(x.to(DEV), codes, scales, k_splits=ks).cpu().double()
        (up, gate), (au, ag) = (ref[:, :inter], ref[:, inter:]), (a[:, :inter], a[:, inter:])
        du, dg, s = au + h(up.abs() + au), ag + h(gate.abs() + ag), R.silu(gate)
        ds = 1.1 * dg + 2.0 ** -21 * s.abs() + h(s.abs() + 1.1 * dg)
        e = up.abs() * ds + s.abs() * du + du * ds
        worst = float(((act - up * s).abs() / (e + h((up * s).abs() + e))).max())
        print(f"\n[silu_gate I={inter} K={K} M={M} ks={ks}] error / bound {worst:.3f}")
        assert float(act.abs().max()) > 0 and worst <= 1.0, (inter, K, M, ks, worst)


@pytest.mark.parametrize("N, K", SHAPES[1:] + [(96, 1152)])     # (96 = [up ; gate] of I = 48)
def test_a_row_has_the_same_bits_alone_and_in_a_batch(N, K):
    _, codes, scales = weights(N, K)[:3]
    x = torch.randn((64, K), generator=torch.Generator().manual_seed(61)).to(BF).to(DEV)
    for form in [L.linear_mxfp4] + ([L.linear_silu_gate_mxfp4] if N % 32 == 0 else []):
        for ks in splits_of(K):
            full = form(x, codes, scales, k_splits=ks)
            for t in (0, 16, 63):
                assert torch.equal(bits(form(x[t:t + 1], codes, scales, k_splits=ks)), bits(full[t:t + 1])), (ks, t)
