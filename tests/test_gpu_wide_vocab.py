"""Rows wider than the 131072 columns csrc/sampling.hip keeps in registers (16 slots x 1024 threads x 8): everything past
them is re-read on every pass — greedy maximum, top-k counts, top-p mass, the Gumbel draw and its Philox counter — by the
loop that starts at vector 16 * 1024 + tid. Every Qwen checkpoint has 151936 or 152064 columns; Mistral-Nemo sits on the
boundary. The reference is tests/_sampling_ref.py, unchanged, and the comparisons are those of tests/test_gpu_sampling.py.

Inputs of the reference comparison lift the tail (`x[:, 131072:] += lift * scale` before the cast) so that the tokens the
reference draws lie in it: a tail that is skipped, read twice or numbered wrongly then shows as a wrong token, not as a
token that happens to sit in the register-resident part. What the reference must give before the kernel is looked at:
>= 0.9 * 16 rows decided (margin > 1e-3, nucleus equal at p +- 1e-4) and, for the lifted widths, >= 12 of 16 reference
tokens at index >= 131072. Measured on the CPU over the 40 cells below (5 widths x 4 modes x 2 dtypes): 15-16 of 16
decided in every cell; 14-16 of 16 in the tail at 151936 and 152069, 12-16 at 131080, 15-16 at 131075. (The three-column
tail of 131075 is lifted by 6.0: at the 5.0 of the eight-column tail the reference draws only 11 of 16 unfiltered tokens
from it, one short of the condition, which is kept.)"""
import numpy as np
import pytest
import torch

from _sampling_ref import filtered_softmax, kept_set, sample_row
from test_gpu_sampling import _chi2_ok, _rows, _sample, _sp

pytestmark = pytest.mark.gpu

HELD = 131072           # kSampleSlots * kSampleThreads * 8
ROWS = 16
# (n, row stride, lift): the boundary itself (the tail loop must not run), one whole tail vector on the 16-byte path, a
# scalar partial vector (stride % 8: VEC = false), a Qwen vocabulary, a partial last vector on the 16-byte path
WIDTHS = [(HELD, HELD, None), (HELD + 8, HELD + 8, 5.0), (HELD + 3, HELD + 3, 6.0), (151936, 151936, 1.5),
          (152069, 152072, 1.5)]
MODES = [(1.0, 0, 1.0, 2.5), (0.8, 50, 1.0, 2.5), (1.2, 0, 0.9, 8.0), (0.7, 100, 0.8, 6.0)]


def _strided(x: torch.Tensor, stride: int) -> torch.Tensor:
    """x on the device as rows of a [rows, stride] store; the padding between rows would win every comparison."""
    rows, n = x.shape
    if stride == n:
        return x.cuda()
    store = torch.full((rows, stride), 100.0, dtype=x.dtype)
    store[:, :n] = x
    view = store.cuda()[:, :n]
    assert view.stride(0) == stride
    return view


def tail_input(n, lift, scale, dtype):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(ROWS, n, generator=g) * scale
    if lift is not None:
        x[:, HELD:] += lift * scale
    return x.to(dtype)


def reference_shares(x, params, pos, top_p):
    """(reference rows, decided row indices, rows whose reference token lies in the tail)."""
    ref = _rows(x, params, pos, top_p)
    decided = [r for r, (_, ok) in enumerate(ref) if ok]
    in_tail = sum(tok >= HELD for tok, _ in ref)
    return ref, decided, in_tail


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,stride,lift", WIDTHS)
def test_sampler_matches_reference_in_the_tail(dtype, mode, n, stride, lift):
    temp, top_k, top_p, scale = mode
    x = tail_input(n, lift, scale, dtype)
    params = [_sp(temp, top_k, top_p, seed=1000 + r) for r in range(ROWS)]
    pos = [17 + 3 * r for r in range(ROWS)]
    ref, decided, in_tail = reference_shares(x, params, pos, top_p)
    print(f"\n[tail n={n} stride={stride} {dtype} mode={mode}] decided {len(decided)}/{ROWS}  in the tail {in_tail}/{ROWS}")
    assert len(decided) >= 0.9 * ROWS, len(decided)
    if lift is not None:
        assert in_tail >= 12, in_tail
    got = _sample(_strided(x, stride), params, pos)
    assert [got[r] for r in decided] == [ref[r][0] for r in decided]
    for r, f in enumerate(x.double().numpy()):
        assert kept_set(f, temp, top_k, 1.0)[got[r]]                        # inside the top-k set, exactly
        assert kept_set(f, temp, top_k, top_p, 1e-4)[got[r]]                # inside the nucleus of p + 1e-4


# ---- edges across the boundary -----------------------------------------------------------------------------------------
EDGE_SEEDS = 4


def _edge_rows(n, dtype):
    """[(name, row [n] in `dtype`, (temperature, top_k))]: every row is sampled greedily and with EDGE_SEEDS seeds."""
    g = torch.Generator().manual_seed(n)
    last = n - 1
    inf, nan = float("inf"), float("nan")
    out = []

    def base():
        return torch.randn(n, generator=g)
    for p in (HELD - 1, HELD, last):                # the only maximum just before, just after the boundary, at the end
        row = base()
        row[p] = row.max() + 30.0
        out.append((f"max@{p}", row, (1.0, 0)))
    row = base()
    row[[HELD - 1, HELD, last]] = row.max() + 30.0  # three equal maxima: greedy takes the lowest, top_k = 2 keeps all three
    out.append(("three maxima", row, (1.0, 2)))
    # top_k = 50 whose 50th and 51st largest are equal and lie on opposite sides of the boundary: 49 distinct larger
    # values (exact in both dtypes) spread over both sides, then 9.0 twice; T = 4 keeps the draw open among the 51
    row = base().clamp(max=6.0)
    tail = n - HELD
    cols = [HELD - 3 - 2 * i for i in range(25)] + [HELD + (7 * i) % tail for i in range(24)] if tail >= 24 * 7 else \
        [HELD - 3 - 2 * i for i in range(47)] + [HELD, last]
    assert len(set(cols)) == 49
    row[cols] = 10.0 + 0.125 * torch.arange(49, dtype=torch.float32)
    lo, hi = HELD - 2, (HELD + 5 if tail >= 24 * 7 else HELD + 1)
    assert lo not in cols and hi not in cols and hi < n
    row[lo] = row[hi] = 9.0
    out.append(("top-50 tie across", row, (4.0, 50)))
    row = base() * 3
    row[HELD:] += 6.0
    row[HELD::7] = nan                              # NaN on every 7th column of the tail
    out.append(("tail NaN::7", row, (1.0, 0)))
    row = base() * 3
    row[HELD:] = -inf
    out.append(("tail -inf", row, (1.0, 0)))
    row = base() * 3
    row[HELD:] = nan
    out.append(("tail NaN", row, (1.0, 0)))
    row = torch.full((n,), -inf)
    row[HELD + (tail * 2) // 3] = -3.0              # -inf everywhere except one tail column
    out.append(("one finite tail column", row, (1.0, 0)))
    out.append(("all -inf", torch.full((n,), -inf), (1.0, 0)))
    return [(name, r.to(dtype), mode) for name, r, mode in out]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n", [151936, HELD + 3])
def test_sampler_edges_across_the_boundary(dtype, n):
    cases = _edge_rows(n, dtype)
    rows, params, pos, names = [], [], [], []
    for c, (name, row, (temp, top_k)) in enumerate(cases):
        for s in range(EDGE_SEEDS + 1):             # s == 0: the greedy row
            rows.append(row)
            params.append(None if s == 0 else _sp(temp, top_k, 1.0, seed=4000 + 16 * c + s))
            pos.append(3 + 5 * c + s)
            names.append((name, s))
    x = torch.stack(rows)
    got = _sample(x.cuda(), params, pos)             # (n = 131075: an odd row stride, the scalar loads)
    f64 = x.double().numpy()
    for r, (name, s) in enumerate(names):
        f = f64[r]
        sp = params[r]
        if sp is None:
            want, margin = sample_row(f, 0.0, 0, 1.0, 0, 0)
        else:
            want, margin = sample_row(f, sp.temperature, sp.top_k, sp.top_p, sp.seed, pos[r])
            if not np.all(np.isnan(f) | (f == -np.inf)):
                assert kept_set(f, sp.temperature, sp.top_k, 1.0)[got[r]], (name, s, got[r])
        assert margin > 1e-3, (name, s, margin)     # from the reference alone: every edge row is decided
        assert got[r] == want, (name, s, got[r], want)
    by = {name: [got[r] for r, (nm, _) in enumerate(names) if nm == name] for name, _, _ in cases}
    last = n - 1
    for p in (HELD - 1, HELD, last):
        assert by[f"max@{p}"] == [p] * (EDGE_SEEDS + 1)
    assert by["three maxima"][0] == HELD - 1 and set(by["three maxima"][1:]) <= {HELD - 1, HELD, last}
    tie = next(row for name, row, _ in cases if name == "top-50 tie across").double().numpy()
    assert int(kept_set(tie, 4.0, 50, 1.0).sum()) == 51          # ties kept: both 9.0s, one on each side
    assert all(t < HELD for t in by["tail -inf"]) and all(t < HELD for t in by["tail NaN"])
    assert all(t < HELD or (t - HELD) % 7 for t in by["tail NaN::7"])
    assert by["one finite tail column"] == [HELD + ((n - HELD) * 2) // 3] * (EDGE_SEEDS + 1)
    assert by["all -inf"] == [0] * (EDGE_SEEDS + 1)


def test_determinism_and_row_independence_in_the_tail():
    n = 151936
    g = torch.Generator().manual_seed(11)
    x = torch.randn(ROWS, n, generator=g) * 2
    x[:, HELD:] += 3.0
    x = x.to(torch.bfloat16).cuda()
    params = [_sp(1.0, 40 if r % 3 == 0 else 0, 0.9 if r % 2 else 1.0, seed=77 + r) for r in range(ROWS)]
    pos = [100 + r for r in range(ROWS)]
    a, b = _sample(x, params, pos), _sample(x, params, pos)
    assert a == b
    assert _sample(x[5:6].clone(), params[5:6], pos[5:6]) == [a[5]]
    assert sum(t >= HELD for t in a) >= 8 and len(set(a)) > 8      # (draws from the tail, and not one draw 16 times)


def test_distribution_over_a_tail_of_likely_tokens():
    """The chi-square test of test_distribution_matches_filtered_softmax at its 0.999 limit, on a row whose 24 likely
    tokens all lie past the register-resident columns. Seeds are fixed: the outcome is deterministic."""
    from swiftllm_amd.worker.kernels.sampling import SampleArgs, sample_rows
    n, rows, temp = 151936, 8192, 1.0
    g = torch.Generator().manual_seed(3)
    row = torch.randn(n, generator=g).to(torch.bfloat16)
    row[torch.randint(HELD, n, (24,), generator=g)] = torch.linspace(6, 9, 24).to(torch.bfloat16)
    x = row.cuda().unsqueeze(0).expand(rows, -1).contiguous()
    dev = x.device
    seeds = torch.stack((torch.arange(rows, dtype=torch.int32), torch.zeros(rows, dtype=torch.int32)), 1)
    args = SampleArgs(torch.full((rows,), temp, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev),
                      torch.ones(rows, device=dev), seeds.to(dev).contiguous(),
                      torch.full((rows,), 5, dtype=torch.int32, device=dev))
    toks = sample_rows(x, args, None).cpu().numpy()
    probs = filtered_softmax(row.double().numpy(), temp, 0, 1.0)
    stat, limit = _chi2_ok(np.bincount(toks, minlength=n).astype(np.float64), probs)
    print(f"\n[tail distribution] chi2 {stat:.1f} limit {limit:.1f}  draws in the tail {(toks >= HELD).mean():.3f} "
          f"(expected {probs[HELD:].sum():.3f})")
    assert stat < limit, (stat, limit)
