"""The packed ring kernel's wave-to-tile assignment (csrc/gemm_skinny.hip, SPREAD: the four-wave SiLU-gate forms today): which
wave of which workgroup computes a 32-row tile of W is free, what it computes is not. Every packed entry of the ring kernel
— SiLU-gate, partial and direct, whichever assignment it runs — must give the bits of the row-major
entry of the same mode — output, slabs and (norm on the fly) the slabs of the pre-multiplied activations — at the smallest
shapes that reach each path: three-wave / four-wave / last partial workgroup (N), shallow / deep ring (K), every legal split.

The entries that scale by 1/rms (_silu_gate_rs / _nf / _nx, _partial_nx) have no row-major twin. They are held to the
row-major entry all the same, bit for bit, on inputs whose 1/rms is an exact power of two, 2^(m % 3) for token m: the mean
square is 4^-(m % 3) exactly (every partial sum is a small integer times a power of four; the division by K of K * 4^-j and
1 / sqrt of a power of four are exact in IEEE arithmetic), and a power of two moved from the fp32 scale into the activations
commutes with every rounding on the way (no overflow, nothing near the subnormals: the scales are >= 1).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = (1, 9, 17, 32)
NS = (96, 128, 224)
KS = (512, 1024, 1536)
KS_NX = (1024, 2048)   # the exact norm on the fly takes whole 1024-column pieces only (ssq_parts = K / 16, % 64 == 0)
KMAX = 2176            # 17 K-tiles: the shortest K with an uneven split (test_uneven_split_slabs)
DTYPES = (torch.bfloat16, torch.float16)
DT_IDS = ("bf16", "f16")


def _hip():
    from swiftllm_amd import _hip
    return _hip


def _even_splits(k):
    """The splits every entry takes: a power of two up to 16 that cuts K into equal runs of whole 128-column tiles. (The
    packed entries also take uneven splits of >= 8 tiles each: none exists below 17 tiles — test_uneven_split_slabs.)"""
    return [ks for ks in (1, 2, 4, 8, 16) if k % (128 * ks) == 0]


@pytest.fixture(scope="module")
def data():
    """One seeded x [32, 2176], W [2 * 224, 2176], norm weight and sign pattern per dtype (cases take leading slices)."""
    g = torch.Generator(device="cpu").manual_seed(20)
    out = {}
    for dt in DTYPES:
        x = (torch.randn((32, KMAX), generator=g) * 0.5).to(dt).cuda()
        w = (torch.randn((448, KMAX), generator=g) * 0.05).to(dt).cuda()
        nw = (1.0 + 0.1 * torch.randn((KMAX,), generator=g)).to(dt).cuda()
        sign = (torch.randint(0, 2, (32, KMAX), generator=g) * 2 - 1).to(dt).cuda()
        out[dt] = (x, w, nw, sign)
    return out


def _pack(w):
    from swiftllm_amd.worker.kernels.linear import pack_weight
    w = w.contiguous()
    return w, pack_weight(w)


def _up_gate(w_all, inter, k):
    return _pack(torch.cat([w_all[:inter, :k], w_all[224:224 + inter, :k]]))   # [up ; gate]


def _row_pow2(m, device):
    """2^(m % 3) per token, [M, 1] fp32: the 1/rms the scaled cases are built to have."""
    return torch.tensor([[2.0 ** (i % 3)] for i in range(m)], dtype=torch.float32, device=device)


def _partial(name, x, wt, n, ks):
    h = _hip()
    m, k = x.shape
    ws = torch.full((ks * m * n,), float("nan"), dtype=torch.float32, device=x.device)
    h.call(name, h.ptr(ws), ws.numel() * 4, h.ptr(x), h.ptr(wt), m, n, k, x.stride(0), ks, h.dtype_code(x.dtype), h.stream())
    return ws


def _direct(name, x, wt, n, ks):
    h = _hip()
    m, k = x.shape
    ws = torch.empty((max(ks, 1) * m * n,), dtype=torch.float32, device=x.device)
    out = torch.full((m, n), float("nan"), dtype=x.dtype, device=x.device)
    h.call(name, h.ptr(out), h.ptr(x), h.ptr(wt), h.ptr(ws), ws.numel() * 4, m, n, k, x.stride(0), n, ks,
           h.dtype_code(x.dtype), h.stream())
    return out


def _silu(name, x, wt, inter, pre=()):
    """A SiLU-gate entry: (out, x, *pre, w, M, I, K, strides, dtype, stream); `pre` = what the entry takes between x and w."""
    h = _hip()
    m, k = x.shape
    out = torch.full((m, inter), float("nan"), dtype=x.dtype, device=x.device)
    h.call(name, h.ptr(out), h.ptr(x), *pre, h.ptr(wt), m, inter, k, x.stride(0), inter, h.dtype_code(x.dtype), h.stream())
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_partial_slabs_and_direct_match_row_major(data, n, k, dt):
    x_all, w_all = data[dt][:2]
    w, wp = _pack(w_all[:n, :k])
    for m in MS:
        x = x_all[:m, :k].contiguous()
        for ks in _even_splits(k):
            assert torch.equal(_partial("swl_gemm_skinny_packed_partial", x, wp, n, ks),
                               _partial("swl_gemm_skinny_partial", x, w, n, ks)), f"slabs differ: M={m} N={n} K={k} k_splits={ks}"
            assert torch.equal(_direct("swl_gemm_skinny_packed", x, wp, n, ks),
                               _direct("swl_gemm_skinny", x, w, n, ks)), f"outputs differ: M={m} N={n} K={k} k_splits={ks}"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_splits_that_are_not_taken_are_rejected(data, dt):
    """Three splits (no power of two), and eight splits of twelve K-tiles (uneven, fewer than 8 tiles each): refused by the
    packed entry as by the row-major one."""
    x_all, w_all = data[dt][:2]
    for k, ks in ((1024, 3), (1536, 8)):
        w, wp = _pack(w_all[:128, :k])
        x = x_all[:9, :k].contiguous()
        for name, wt in (("swl_gemm_skinny_packed_partial", wp), ("swl_gemm_skinny_partial", w)):
            with pytest.raises(RuntimeError):
                _partial(name, x, wt, 128, ks)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", (128, 224))
def test_uneven_split_slabs(data, n, dt):
    """K = 17 tiles in two splits of 8 and 9 (packed entries only; four-wave workgroups): slab s is the row-major
    entry's single slab over the split's own columns — the same tiles in the same K order from a zero accumulator."""
    x_all, w_all = data[dt][:2]
    k, cut = KMAX, 8 * 128
    w, wp = _pack(w_all[:n, :k])
    for m in MS:
        x = x_all[:m, :k].contiguous()
        got = _partial("swl_gemm_skinny_packed_partial", x, wp, n, 2).view(2, m, n)
        for s, (lo, hi) in enumerate(((0, cut), (cut, k))):
            want = _partial("swl_gemm_skinny_partial", x[:, lo:hi].contiguous(), w[:, lo:hi].contiguous(), n, 1).view(m, n)
            assert torch.equal(got[s], want), f"slab {s} differs: M={m} N={n}"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("inter", NS)
def test_silu_gate_matches_row_major(data, inter, k, dt):
    x_all, w_all = data[dt][:2]
    w, wp = _up_gate(w_all, inter, k)
    for m in MS:
        x = x_all[:m, :k].contiguous()
        assert torch.equal(_silu("swl_gemm_skinny_packed_silu_gate", x, wp, inter),
                           _silu("swl_gemm_skinny_silu_gate", x, w, inter)), f"M={m} I={inter} K={k}"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("inter", NS)
def test_silu_gate_pending_scale_matches_row_major(data, inter, k, dt):
    """swl_gemm_skinny_packed_silu_gate_rs with row_ssq[0][m] = K * 4^-(m % 3), eps = 0: 1/rms = 2^(m % 3) exactly, applied
    to the fp32 sums — the bits of the row-major entry fed x * 2^(m % 3)."""
    h = _hip()
    x_all, w_all = data[dt][:2]
    w, wp = _up_gate(w_all, inter, k)
    for m in MS:
        x = x_all[:m, :k].contiguous()
        s = _row_pow2(m, x.device)
        ssq = (float(k) / (s * s)).view(1, m).contiguous()
        out = torch.full((m, inter), float("nan"), dtype=dt, device=x.device)
        h.call("swl_gemm_skinny_packed_silu_gate_rs", h.ptr(out), h.ptr(x), h.ptr(wp), h.ptr(ssq), 1, 0.0, m, inter, k,
               x.stride(0), inter, h.dtype_code(dt), h.stream())
        want = _silu("swl_gemm_skinny_silu_gate", (x.float() * s).to(dt), w, inter)
        assert torch.equal(out, want), f"M={m} I={inter} K={k}"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("inter", NS)
def test_silu_gate_norm_on_the_fly_matches_row_major(data, inter, k, dt):
    """swl_gemm_skinny_packed_silu_gate_nf (the up/gate launch of the decode layer; four waves from 9 tokens, two below) on
    residual rows r[m, :] = +-2^-(m % 3), eps = 0: the kernel's own sum of squares is K * 4^-(m % 3), its 1/rms 2^(m % 3), the
    staged activations round(r * w_norm) = +-2^-(m % 3) * w_norm — the bits of the row-major entry fed +-w_norm."""
    h = _hip()
    _, w_all, nw_all, sign = data[dt]
    w, wp = _up_gate(w_all, inter, k)
    nw = nw_all[:k].contiguous()
    for m in MS:
        s = _row_pow2(m, nw.device)
        r = (sign[:m, :k].float() / s).to(dt).contiguous()
        got = _silu("swl_gemm_skinny_packed_silu_gate_nf", r, wp, inter, pre=(h.ptr(nw), 0.0))
        want = _silu("swl_gemm_skinny_silu_gate", (sign[:m, :k].float() * nw.float()).to(dt), w, inter)
        assert torch.equal(got, want), f"M={m} I={inter} K={k}"


def _nx_inputs(x_all, nw_all, m, k, dt):
    """Residual rows, norm weight, per-16-column partials that sum to K * 4^-(m % 3) per row (any partials do: they are an
    input), and what the kernel then stages: round(r * 2^(m % 3) * w_norm)."""
    r = x_all[:m, :k].contiguous()
    nw = nw_all[:k].contiguous()
    s = _row_pow2(m, r.device)
    ssq = (16.0 / (s * s)).expand(m, k // 16).contiguous()
    return r, nw, ssq, (r.float() * s * nw.float()).to(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KS_NX)
@pytest.mark.parametrize("inter", NS)
def test_silu_gate_exact_norm_on_the_fly_matches_row_major(data, inter, k, dt):
    """swl_gemm_skinny_packed_silu_gate_nx: nothing pending after the staging, so the row-major entry on the staged rows."""
    h = _hip()
    x_all, w_all, nw_all, _ = data[dt]
    w, wp = _up_gate(w_all, inter, k)
    for m in MS:
        r, nw, ssq, xn = _nx_inputs(x_all, nw_all, m, k, dt)
        got = _silu("swl_gemm_skinny_packed_silu_gate_nx", r, wp, inter, pre=(h.ptr(nw), 0.0, h.ptr(ssq), ssq.shape[1]))
        assert torch.equal(got, _silu("swl_gemm_skinny_silu_gate", xn, w, inter)), f"M={m} I={inter} K={k}"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KS_NX)
@pytest.mark.parametrize("n", NS)
def test_partial_exact_norm_on_the_fly_matches_row_major(data, n, k, dt):
    """swl_gemm_skinny_packed_partial_nx, every even split: the row-major entry's slabs of the staged rows."""
    h = _hip()
    x_all, w_all, nw_all, _ = data[dt]
    w, wp = _pack(w_all[:n, :k])
    for m in MS:
        r, nw, ssq, xn = _nx_inputs(x_all, nw_all, m, k, dt)
        for ks in _even_splits(k):
            ws = torch.full((ks * m * n,), float("nan"), dtype=torch.float32, device=r.device)
            h.call("swl_gemm_skinny_packed_partial_nx", h.ptr(ws), ws.numel() * 4, h.ptr(r), h.ptr(nw), 0.0, h.ptr(ssq),
                   ssq.shape[1], h.ptr(wp), m, n, k, r.stride(0), ks, h.dtype_code(dt), h.stream())
            assert torch.equal(ws, _partial("swl_gemm_skinny_partial", xn, w, n, ks)), f"M={m} N={n} K={k} k_splits={ks}"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_norm_on_the_fly_slabs_and_ssq(data, n, k, dt):
    """swl_gemm_skinny_packed_partial_nf: the slabs are those of the row-major entry fed round(r * w_norm) — the product of
    two 16-bit floats is exact in fp32, so torch's rounding is the kernel's — and ssq_out[split][m] is the fp32 sum of r^2
    over the split's columns: <= K/ks additions, each within 2^-24 relative of a positive running sum."""
    h = _hip()
    x_all, w_all, nw_all, _ = data[dt]
    w, wp = _pack(w_all[:n, :k])
    nw = nw_all[:k].contiguous()
    for m in MS:
        r = x_all[:m, :k].contiguous()
        xn = (r.float() * nw.float()).to(dt)
        for ks in _even_splits(k):
            ws = torch.full((ks * m * n,), float("nan"), dtype=torch.float32, device=r.device)
            ssq = torch.full((ks, m), float("nan"), dtype=torch.float32, device=r.device)
            h.call("swl_gemm_skinny_packed_partial_nf", h.ptr(ws), ws.numel() * 4, h.ptr(ssq), h.ptr(r), h.ptr(nw), h.ptr(wp),
                   m, n, k, r.stride(0), ks, h.dtype_code(dt), h.stream())
            assert torch.equal(ws, _partial("swl_gemm_skinny_partial", xn, w, n, ks)), f"slabs differ: M={m} N={n} K={k} k_splits={ks}"
            ref = r.double().pow(2).view(m, ks, k // ks).sum(-1).t()
            assert torch.allclose(ssq.double(), ref, rtol=(k // ks) * 2.0 ** -24, atol=0), f"ssq: M={m} N={n} K={k} k_splits={ks}"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_packed_weight_inside_a_larger_allocation(data, dt):
    """The packed copy at a non-zero offset of a bigger buffer, guard words on both sides: pack and stream stay inside."""
    h = _hip()
    x_all, w_all = data[dt][:2]
    n, k, m, guard = 224, 1536, 17, 4096
    w = w_all[:n, :k].contiguous()
    big = torch.full((guard + n * k + guard,), 1.0, dtype=dt, device=w.device)
    big[:guard] = -3.0
    big[guard + n * k:] = -3.0
    wp = big[guard:guard + n * k].view(n, k)
    h.call("swl_gemm_pack_weight", h.ptr(wp), h.ptr(w), n, k, h.dtype_code(dt), h.stream())
    x = x_all[:m, :k].contiguous()
    for ks in _even_splits(k):
        assert torch.equal(_partial("swl_gemm_skinny_packed_partial", x, wp, n, ks), _partial("swl_gemm_skinny_partial", x, w, n, ks))
    assert bool((big[:guard] == -3.0).all()) and bool((big[guard + n * k:] == -3.0).all()), "guard words overwritten"
