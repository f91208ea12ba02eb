"""The decode GEMMs and their split-K consumers at the shapes the Qwen and Mistral checkpoints bring (tests/_family_shapes.py).

The kernel tests were written around Llama-3-8B (4096 / 6144 / 28672 / 14336 / 11008). The launch ladder of
csrc/gemm_skinny.hip keys on N / 32 and K / 128, and the admitted checkpoints land in cells no Llama shape reaches: 16
automatic splits of 2 or 3 K-tiles, the three-wave form on the shallow ring, uneven splits at 9.5 and 57.75 tiles per
split, lm_head widths of 4096 / 4748 / 4752 column tiles, a weight of more than 2 GiB. Every pair below is compared as the
existing tests compare (test_gpu_kernels.py): one rounding of the storage dtype around a high-precision product,
    |out - ref| <= eps |ref| + 1e-3 eps sqrt(K),   eps = 2^-10 (float16) / 2^-7 (bfloat16),
and bit equality between the forms that promise it. Weights and activations are drawn on the device (a CPU randn of 2.4e8
values costs seconds); the reference is the fp64 product on the device. N and K are what select the code path and are kept;
the lm_head widths of the larger checkpoints run at K = 1024, which keeps one split on the deep ring as at 4096 - 8192."""
import types

import pytest
import torch

from oracle import eager_ops as ops
from conftest import ulp_diff_fp16

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}

LM_HEADS = [(151936, 1024),     # Qwen3-0.6B lm_head, the real shape
            (152064, 1024),     # Qwen2.5-72B's width
            (131072, 1024)]     # Mistral-Nemo's / Mistral-Small's width
PAIRS = [(2560, 4096),          # Qwen3-4B o_proj
         (2048, 6144),          # Qwen3-1.7B down
         (6144, 2560),          # Qwen3-4B qkv
         (2560, 9728),          # Qwen3-4B down
         (2048, 11008),         # Qwen2.5-3B down
         (5120, 4096),          # Mistral-Nemo o_proj
         (10240, 5120),         # Qwen3-32B qkv
         (5120, 25600),         # Qwen3-32B down
         (8192, 29568),         # Qwen2.5-72B down
         (1024, 3072),          # Qwen3-0.6B down
         (1024, 2048)] + LM_HEADS    # Qwen3-0.6B o_proj


def _L():
    import importlib        # (the package exports a function of the same name)
    return importlib.import_module("swiftllm_amd.worker.kernels.linear")


def _lib():
    from swiftllm_amd import _hip
    return _hip.load()


def _within(out, ref, k, eps):
    return bool(((out.double() - ref).abs() <= eps * ref.abs() + 1e-3 * eps * (k ** 0.5)).all())


def _device_randn(shape, seed, scale, dtype):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(dtype)


_case = {}      # the inputs of the last (N, K, dtype): one weight resident at a time


def _inputs(n, k, dtype):
    """x [256, K] ~ N(0, 1), W [N, K] ~ 0.05 N(0, 1) with its packed twin attached, ref = the fp64 product [256, N]."""
    key = (n, k, dtype)
    if key not in _case:
        _case.clear()
        torch.cuda.empty_cache()
        x = _device_randn((256, k), 3 * n + k, 1.0, dtype)
        w = _device_randn((n, k), 3 * n + k + 1, 0.05, dtype)
        ref = x.double() @ w.double().T
        _L().pack_weight(w)
        _case[key] = types.SimpleNamespace(x=x, w=w, wp=w._swl_packed, ref=ref)
    return _case[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K", PAIRS)
def test_skinny_gemms_at_the_family_shapes(dtype, N, K):
    """<= 32 tokens: the packed entry through the operators (self-reducing, and slabs then the stand-alone reduce) and the
    row-major entry at the split count the packed one chose — the bound, and the same bits three times."""
    from swiftllm_amd import _hip
    L, lib = _L(), _lib()
    c = _inputs(N, K, dtype)
    ks = int(lib.swl_gemm_skinny_packed_choose_splits(N, K))
    even = K % (128 * ks) == 0
    print(f"\n[family gemm {N} x {K}] packed splits {ks} ({K / 128 / ks:g} K-tiles each{'' if even else ', uneven'}), "
          f"row-major choice {int(lib.swl_gemm_skinny_choose_splits(N, K))}")
    code = _hip.dtype_code(dtype)
    for M in (1, 7, 32):
        x, ref = c.x[:M], c.ref[:M]
        out = L.linear(x, c.w, skinny=True)
        assert out.shape == (M, N) and out.dtype == dtype
        assert _within(out, ref, K, EPS[dtype]), M
        part = L.linear_splitk(x, c.w)
        assert isinstance(part, L.SplitKPartials) == (ks > 1) and (ks == 1 or part.k_splits == ks)
        slabbed = part.materialize() if ks > 1 else part
        assert torch.equal(slabbed, out), M
        ws = torch.empty(max(ks * M * N, 4), dtype=torch.float32, device="cuda")
        rowmajor = torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
        call = lambda: _hip.call("swl_gemm_skinny", rowmajor.data_ptr(), x.data_ptr(), c.w.data_ptr(), ws.data_ptr(),  # noqa: E731
                                 ws.numel() * 4, M, N, K, K, N, ks, code, _hip.stream())
        if even:
            call()
            assert torch.equal(rowmajor, out), M
        else:
            # splits that differ by one K-tile exist on packed weights only: the row-major entry refuses the count
            with pytest.raises(_hip.HipLibraryError):
                call()
            assert bool(torch.isnan(rowmajor).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K", PAIRS)
def test_mid_and_wide_gemms_at_the_family_shapes(dtype, N, K):
    """33..64 tokens (swl_gemm_packed_mid) and 65..256 (swl_gemm_packed_wide) with the library's own choice of waves and
    splits, launched as kernels/linear.py launches them."""
    L, lib = _L(), _lib()
    c = _inputs(N, K, dtype)
    lm_head = (N, K) in LM_HEADS
    for M in ((64,) if lm_head else (48,)):
        x = c.x[:M]
        ks = int(lib.swl_gemm_packed_mid_choose_splits(M, N, K))
        out = L._launch_out("swl_gemm_packed_mid", x, c.wp, N, L._workspace(x.device, ks * M * N * 4 if ks > 1 else 0), ks)
        assert _within(out, c.ref[:M], K, EPS[dtype]), ("mid", M, ks)
    for M in ((256,) if lm_head else (128, 256)):
        x = c.x[:M]
        out = L._launch_wide(x, c.w)
        assert _within(out, c.ref[:M], K, EPS[dtype]), ("wide", M, int(lib.swl_gemm_packed_wide_choose_splits(M, N, K)))


# ---- SiLU-gate entries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("I,Kd", [(9728, 2560),       # Qwen3-4B
                                  (3072, 1024),       # Qwen3-0.6B
                                  (11008, 2048),      # Qwen2.5-3B
                                  (25600, 5120)])     # Qwen3-32B
def test_silu_gate_gemms_at_the_family_shapes(dtype, I, Kd):
    """Fused == the one-split GEMM followed by silu_and_mul, bit for bit, in every tier (<= 32 tokens row-major and packed,
    48 tokens mid, 128 tokens wide), and the bound of test_gemm_silu_gate_fusion_equals_two_ops around the fp64 product:
    three chained roundings (up, silu(gate), product) on projections that may each be 1 ulp off."""
    from swiftllm_amd import _hip
    from swiftllm_amd.worker import kernels as Kn
    L = _L()
    code = _hip.dtype_code(dtype)
    x_all = _device_randn((128, Kd), I + Kd, 1.0, dtype)
    w = _device_randn((2 * I, Kd), I + Kd + 1, 0.03, dtype)
    ref = (x_all.double() @ w.double().T).to(dtype).cpu()
    ops.silu_and_mul_inplace(ref)
    ref = ref[:, :I].float()
    eps = 2.0 ** -7 if dtype == torch.float16 else 2.0 ** -4

    def two_ops(name, x, wt, *tail):
        M = x.shape[0]
        two = torch.empty(M, 2 * I, dtype=dtype, device="cuda")
        _hip.call(name, two.data_ptr(), x.data_ptr(), wt.data_ptr(), 0, 0, M, 2 * I, Kd, Kd, 2 * I, *tail, 1, code,
                  _hip.stream())
        Kn.silu_and_mul_inplace(two)
        return two[:, :I]

    def held(fused, two, x, what):
        assert fused is not None and fused.shape == (x.shape[0], I)
        assert torch.equal(fused, two), what
        assert bool(((fused.cpu().float() - ref[:x.shape[0]]).abs() <= eps * ref[:x.shape[0]].abs() + 2e-3).all()), what
    rowmajor = {M: L.linear_silu_gate(x_all[:M], w) for M in (1, 32)}
    for M in (1, 32):
        held(rowmajor[M], two_ops("swl_gemm_skinny", x_all[:M], w), x_all[:M], ("row-major", M))
    wp = L.pack_weight(w)
    for M in (1, 32):
        x = x_all[:M]
        fused = L.linear_silu_gate(x, w)
        held(fused, two_ops("swl_gemm_skinny_packed", x, wp), x, ("packed", M))
        assert torch.equal(fused, rowmajor[M]), M
    x = x_all[:48]
    held(L._launch_silu("swl_gemm_packed_mid_silu_gate", x, wp), two_ops("swl_gemm_packed_mid", x, wp), x, "mid")
    x = x_all[:128]
    held(L._launch_wide_silu(x, w), two_ops("swl_gemm_packed_wide", x, wp, 0), x, "wide")


# ---- the split-K consumers at the new hidden sizes ----------------------------------------------------------------------
HIDDEN = [1024, 2048, 2560, 5120, 8192]


def _consumer_case(dtype, M, hidden):
    L = _L()
    seed = 5 * hidden + M
    x = _device_randn((M, 2 * hidden), seed, 1.0, dtype)
    w = _device_randn((hidden, 2 * hidden), seed + 1, 0.02, dtype)
    res = _device_randn((M, hidden), seed + 2, 1.0, dtype)
    nw = (1 + _device_randn((hidden,), seed + 3, 0.1, torch.float32)).to(dtype)
    L.pack_weight(w)
    part = L.linear_splitk(x, w)
    assert isinstance(part, L.SplitKPartials) and part.k_splits > 1
    # the families' rms_norm_eps in half of the cases, Llama's in the other
    eps = 1e-6 if (HIDDEN.index(hidden) + (M > 1)) % 2 == 0 else 1e-5
    return part, res, nw, eps


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 32])
@pytest.mark.parametrize("hidden", HIDDEN)
def test_fused_add_rmsnorm_from_splitk_at_the_family_hidden_sizes(dtype, M, hidden):
    from swiftllm_amd.worker import kernels as Kn
    from swiftllm_amd.worker.kernels.rmsnorm import fused_add_rmsnorm_from_splitk
    part, res, nw, eps = _consumer_case(dtype, M, hidden)
    ks = part.k_splits
    slabs = part.slabs[:ks * M * hidden].view(ks, M, hidden).clone()
    # against "materialise, then fused_add_rmsnorm_inplace": bit for bit
    y = part.materialize()
    r1 = res.clone()
    Kn.fused_add_rmsnorm_inplace(y, r1, nw, eps)
    r2 = res.clone()
    y2 = fused_add_rmsnorm_from_splitk(part, r2, nw, eps)
    assert torch.equal(y2, y) and torch.equal(r2, r1)
    # against fp64. The slabs are summed in fp32 in split order (the contract of swl_splitk_reduce) and rounded; the sum with
    # the residual is exact in fp64 and rounded once; the norm of that row in fp64, within 1 ulp.
    total = torch.zeros(M, hidden, dtype=torch.float32, device="cuda")
    for k in range(ks):
        total += slabs[k]
    want_r = (total.to(dtype).double() + res.double()).to(dtype)
    assert torch.equal(r2, want_r)
    r64 = want_r.double()
    want_x = (r64 * torch.rsqrt(r64.pow(2).mean(-1, keepdim=True) + eps) * nw.double()).to(dtype)
    assert ulp_diff_fp16(y2.cpu(), want_x.cpu()) <= 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 32])
@pytest.mark.parametrize("hidden", [h for h in HIDDEN if h % 1024 == 0])
def test_add_scale_from_splitk_at_the_family_hidden_sizes(dtype, M, hidden):
    """The three asserts of test_add_scale_from_splitk: the residual carries the bits fused_add_rmsnorm_from_splitk gives it,
    x_scaled is exactly round(residual * w), the per-1024-column sums of squares add up (fp64 reference)."""
    from swiftllm_amd.worker.kernels.rmsnorm import add_scale_from_splitk, fused_add_rmsnorm_from_splitk
    part, res, nw, eps = _consumer_case(dtype, M, hidden)
    r_exact = res.clone()
    fused_add_rmsnorm_from_splitk(part, r_exact, nw, eps)
    r_def = res.clone()
    pend = add_scale_from_splitk(part, r_def, nw, eps, unsafe_float16_ok=True)
    assert torch.equal(r_def, r_exact)
    assert torch.equal(pend.x, (r_def.float() * nw.float()).to(dtype))
    assert pend.ssq.shape == (hidden // 1024, M) and pend.eps == eps
    want = r_def.double().pow(2).view(M, hidden // 1024, 1024).sum(-1).T
    assert torch.allclose(pend.ssq.double(), want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_scale_from_splitk_refuses_hidden_2560(dtype, monkeypatch):
    from swiftllm_amd import _hip
    from swiftllm_amd.worker.kernels.rmsnorm import add_scale_from_splitk, deferred_norm_ok
    part, res, nw, eps = _consumer_case(dtype, 32, 2560)
    assert not deferred_norm_ok(32, 2560, torch.bfloat16)
    before = res.clone()
    launched = []
    monkeypatch.setattr(_hip, "call", lambda name, *args: launched.append(name))
    with pytest.raises(AssertionError, match="hidden % 1024"):
        add_scale_from_splitk(part, res, nw, eps, unsafe_float16_ok=True)
    assert launched == [] and torch.equal(res, before)


# ---- a weight past 2 GiB ---------------------------------------------------------------------------------------------------
def test_weight_rows_past_2_gib():
    """Qwen2.5-72B's lm_head, 152064 x 8192 bfloat16 = 2.49 GB: the byte offset of row 131072 of the row-major weight is
    2^31. Output columns around that row and at both ends against the fp64 product of those rows, every other column
    against the fp32 product, under the bound of this file."""
    from swiftllm_amd import _hip
    if torch.cuda.mem_get_info()[0] < 12e9:
        pytest.skip("needs 12 GB of free device memory")
    _case.clear()
    torch.cuda.empty_cache()
    L = _L()
    N, K, dtype = 152064, 8192, torch.bfloat16
    eps = EPS[dtype]
    assert N * K * 2 > 2 ** 31 and 131072 * K * 2 == 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(72)
    x = torch.randn(256, K, generator=g, device="cuda").to(dtype)
    w = torch.empty(N, K, dtype=dtype, device="cuda")
    step = 16896        # N / 9
    for r in range(0, N, step):
        w[r:r + step] = (torch.randn(step, K, generator=g, device="cuda") * 0.05).to(dtype)
    wp = L.pack_weight(w)
    xf = x.float()
    ref32 = torch.empty(256, N, dtype=torch.float32, device="cuda")
    for r in range(0, N, step):
        ref32[:, r:r + step] = xf @ w[r:r + step].float().T
    bands = [(0, 128), (131072 - 128, 131072 + 128), (N - 128, N)]
    ref64 = [x.double() @ w[a:b].double().T for a, b in bands]
    code = _hip.dtype_code(dtype)

    def rowmajor(xm):
        out = torch.full((xm.shape[0], N), float("nan"), dtype=dtype, device="cuda")
        _hip.call("swl_gemm_skinny", out.data_ptr(), xm.data_ptr(), w.data_ptr(), 0, 0, xm.shape[0], N, K, K, N, 1, code,
                  _hip.stream())
        return out
    runs = [("packed skinny", 1, lambda xm: L.linear(xm, w, skinny=True)),
            ("packed skinny", 32, lambda xm: L.linear(xm, w, skinny=True)),
            ("row-major skinny", 32, rowmajor),
            ("packed mid", 64, lambda xm: L._launch_out("swl_gemm_packed_mid", xm, wp, N, None, 1)),
            ("packed wide", 256, lambda xm: L._launch_wide(xm, w))]
    assert int(_hip.load().swl_gemm_skinny_packed_choose_splits(N, K)) == 1
    assert int(_hip.load().swl_gemm_packed_mid_choose_splits(64, N, K)) == 1
    for what, M, run in runs:
        out = run(x[:M])
        assert out.shape == (M, N)
        for (a, b), r64 in zip(bands, ref64):
            assert _within(out[:, a:b], r64[:M], K, eps), (what, M, a)
        assert _within(out, ref32[:M].double(), K, eps), (what, M)
        del out
    del w, wp, ref32
    torch.cuda.empty_cache()
