"""The mixture-of-experts kernels (csrc/moe.hip) against the fp64 restatement of tests/_moe_ref.py, float16 and bfloat16.

Every stage is compared with fp64 computed from ITS OWN inputs — the x, ids, weights and stored `act` / `y` the kernels
produced — so no stage's error is charged to the next.

Routing. ids are exact where the logits' k-th gap is at least 2^-6 (by construction: distinct multiples of 2^-5, plus in
fp32 a jitter below 2^-8) and on exactly tied logits (lowest id first); weights within 4 fp32 ulps of the fp64 softmax.

The bound of the GEMM stages, derived, not tuned. Write a(mag) = 2^-18 * mag for the fp32-accumulation allowance on a sum
whose absolute products add to `mag` (the allowance of tests/test_gpu_qk_prep.py), h(v) = half an ulp of T at |v|, and let
up*, gate* be the exact projections, s* = silu(gate*), act* = up* s*.
  up_gate_silu: the kernel rounds up and gate to T (one rounding each), evaluates silu in fp32 (charged 2^-21 |s*|: 4 fp32
    ulps), rounds it to T, multiplies and rounds to T. So
      du = a(up_mag) + h(|up*| + a(up_mag)),   dg = a(gate_mag) + h(|gate*| + a(gate_mag)),
      ds = 1.1 dg + 2^-21 |s*| + h(|s*| + 1.1 dg)                     (|silu'| <= 1.1)
      e  = |up*| ds + |s*| du + du ds,         |act - act*| <= e + h(|act*| + e).
  down: y is the fp32 sum itself, never rounded to T: |y - y*| <= a(y_mag), y* from the STORED act.
  combine: k products and k sums in fp32, then ONE rounding to T: |out - out*| <= a(out_mag) + h(|out*| + a(out_mag)),
    out* from the STORED y and the kernel's own fp32 weights.

Row independence: a token's `out` bits alone (T = 1) equal its bits as any row of T = 33 and under a permutation of the rows.
Memory: the whole chain runs inside tests/_arena.py arenas — nothing outside the declared outputs changes and no fill byte
reaches an output."""
import pytest
import torch

from swiftllm_amd import _hip
from swiftllm_amd.worker.kernels import moe as M

import _moe_ref as R
from _arena import Op, run_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
GEOMETRIES = [(256, 128), (256, 192)]
CASES = {"A": (4, 2, (1, 3, 16, 17, 33)), "B": (8, 2, (1, 3, 16, 17, 33)), "C": (128, 8, (1, 33, 200))}
STEPS = [(name, t) for name, (_, _, ts) in CASES.items() for t in ts]


def gapped_logits(g, T, E, dtype):
    """[T, E]: per row a permutation of E distinct multiples of 2^-5 around 0 (every gap >= 2^-5, exact in bfloat16 for
    E <= 128); in fp32 plus a jitter below 2^-8, which leaves every gap above 2^-6."""
    base = (torch.arange(E, dtype=torch.float32) - E // 2) / 32.0
    rows = torch.stack([base[torch.randperm(E, generator=g)] for _ in range(T)])
    if dtype == torch.float32:
        rows = rows + (torch.rand((T, E), generator=g) - 0.5) * 2.0 ** -8
    out = rows.to(dtype)
    srt = out.double().sort(dim=1).values
    assert E == 1 or float((srt[:, 1:] - srt[:, :-1]).min()) >= 2.0 ** -6
    return out


def check_route(logits, k, norm):
    ids, w = M.moe_route(logits.to(DEV), k, norm)
    ids, w = ids.cpu(), w.cpu()
    want_ids, want_w = R.route_ref(logits.cpu(), k, norm)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32
    assert torch.equal(ids.long(), want_ids), (ids[:4], want_ids[:4])
    err = (w.double() - want_w).abs()
    worst = float((err / R.ulp_of(want_w, torch.float32)).max())
    assert worst <= 4.0, worst
    return ids, w, worst


# ---- routing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", list(CASES))
def test_route_ids_are_exact_and_weights_within_4_ulps(case, ldtype):
    E, k, ts = CASES[case]
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for T in ts:
        logits = gapped_logits(g, T, E, ldtype)
        assert float(R.kth_gap(logits, k).min()) >= 2.0 ** -6
        for norm in (True, False):
            ids, w, u = check_route(logits, k, norm)
            worst = max(worst, u)
            assert bool((w[:, :-1] >= w[:, 1:]).all())                      # slots in descending probability
            if norm:
                assert float((w.double().sum(1) - 1).abs().max()) <= 2.0 ** -22
    print(f"\n[route {case} {ldtype}] worst weight error {worst:.2f} fp32 ulps")


def test_route_ties_go_to_the_lowest_id_and_k_may_equal_e():
    g = torch.Generator().manual_seed(12)
    for E, k in ((4, 2), (8, 2), (128, 8), (4, 4), (8, 8), (16, 16), (256, 16), (100, 3)):
        tied = torch.zeros((3, E))
        ids, w, _ = check_route(tied, k, True)
        assert ids.tolist() == [list(range(k))] * 3
        assert torch.equal(w, torch.full((3, k), 1.0 / k))
        few = torch.randint(0, 3, (19, E), generator=g).float()            # three distinct values: ties everywhere
        check_route(few, k, True)
        check_route(few.to(torch.bfloat16), k, False)
        check_route(gapped_logits(g, 5, E, torch.float32) * 8.0, k, True)   # a peaked softmax: tiny tail weights
    # a row stride wider than E
    wide = torch.randn((7, 40), generator=g).to(DEV)
    ids, w = M.moe_route(wide[:, :8], 2, True)
    want_ids, want_w = R.route_ref(wide[:, :8].cpu(), 2, True)
    assert torch.equal(ids.cpu().long(), want_ids) and float((w.cpu().double() - want_w).abs().max()) <= 2.0 ** -23


def test_route_rows_that_are_not_finite_get_ids_0_to_k_and_weight_0():
    g = torch.Generator().manual_seed(13)
    E, k = 128, 8
    logits = gapped_logits(g, 9, E, torch.float32)
    logits[1, 5] = float("nan")
    logits[3, 127] = float("inf")
    logits[4, 0] = float("-inf")
    logits[7] = float("nan")
    for ldtype in (torch.float32, torch.float16, torch.bfloat16):
        ids, w, _ = check_route(logits.to(ldtype), k, True)
        for t in (1, 3, 4, 7):
            assert ids[t].tolist() == list(range(k)) and not bool(w[t].any())
        assert bool((w[[0, 2, 5, 6, 8]] > 0).all())


# ---- alignment -----------------------------------------------------------------------------------------------------------
def check_align(ids, E):
    """The properties of the tile tables for topk_ids [T, k] (CPU int32); returns (tile_rows, tile_experts)."""
    T, k = ids.shape
    rows, experts = M.moe_align(ids.to(DEV), E)
    rows, experts = rows.cpu(), experts.cpu()
    tiles = (T * k + 15) // 16 + min(E, T * k)
    assert experts.numel() == tiles == M.max_tiles(T, k, E) and rows.numel() == tiles * 16
    flat = ids.reshape(-1)
    valid = ((flat >= 0) & (flat < E)).nonzero().flatten()
    placed = rows[rows >= 0]
    assert sorted(placed.tolist()) == valid.tolist()                         # every pair exactly once
    assert bool(((rows >= -1) & (rows < T * k)).all())
    used = 0
    for t in range(tiles):
        r = rows[t * 16:(t + 1) * 16]
        live = r[r >= 0]
        if int(experts[t]) < 0:
            assert int(experts[t]) == -1 and live.numel() == 0                # unused tiles: -1, all padding
            continue
        used += 1
        assert 0 <= int(experts[t]) < E and live.numel() >= 1
        assert bool((flat[live.long()] == experts[t]).all())                 # rows of ONE expert
        assert bool((r[:live.numel()] >= 0).all()) and live.tolist() == sorted(live.tolist())   # packed, stable
    counts = torch.bincount(flat[valid].long(), minlength=E)
    assert used == int(((counts + 15) // 16).sum())
    live_experts = experts[experts >= 0]
    assert live_experts.tolist() == sorted(live_experts.tolist()) and bool((experts[used:] == -1).all())
    return rows, experts


@pytest.mark.parametrize("case, T", STEPS)
def test_align_places_every_pair_once_in_tiles_of_one_expert(case, T):
    E, k, _ = CASES[case]
    g = torch.Generator().manual_seed(14)
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).int()
    a = check_align(ids, E)
    b = check_align(ids, E)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])               # a function of topk_ids alone


def test_align_edge_cases():
    # all_to_one: one expert has several tiles, every other none
    ids = torch.tensor([[5, 2]] * 33).int()
    rows, experts = check_align(ids, 8)
    assert experts[experts >= 0].tolist() == [2, 2, 2, 5, 5, 5]
    # empty_expert: expert 3 of 4 is never chosen; T k = 34 is no multiple of 16
    ids = torch.tensor([[0, 1], [2, 0], [1, 2]] * 5 + [[0, 2], [2, 1]]).int()
    assert ids.numel() == 34 and 3 not in ids
    check_align(ids, 4)
    # one pair; k == E; the largest step one call takes; ids outside [0, E) are in no tile
    check_align(torch.tensor([[6]]).int(), 8)
    check_align(torch.arange(4).repeat(17, 1).int(), 4)
    g = torch.Generator().manual_seed(15)
    check_align(torch.stack([torch.randperm(128, generator=g)[:8] for _ in range(512)]).int(), 128)
    check_align(torch.zeros((256, 16), dtype=torch.int32), 256)
    check_align(torch.tensor([[0, 9], [-1, 3], [8, 2], [7, 128]]).int(), 8)


# ---- GEMM stages ---------------------------------------------------------------------------------------------------------
def a_of(mag):
    return mag * 2.0 ** -18


def chain(g, T, E, k, H, I, dtype, norm=True, x=None, logits=None, weights=None, w_scale=0.05):
    """Run the five launches; return every intermediate on the CPU."""
    if weights is None:
        gd = torch.Generator(device=DEV).manual_seed(int(torch.randint(0, 2 ** 31, (1,), generator=g)))
        weights = ((torch.randn((E, 2 * I, H), generator=gd, device=DEV) * w_scale).to(dtype),
                   (torch.randn((E, H, I), generator=gd, device=DEV) * w_scale).to(dtype))
    if x is None:
        x = torch.randn((T, H), generator=g).to(dtype)
    if logits is None:
        logits = gapped_logits(g, T, E, torch.float32)
    ug, dn = weights
    xd = x.to(DEV)
    ids, w = M.moe_route(logits.to(DEV), k, norm)
    rows, experts = M.moe_align(ids, E)
    act = M.moe_up_gate_silu(xd, ug, rows, experts, k)
    y = M.moe_down(act, dn, rows, experts, k)
    out = M.moe_combine(y, w, torch.empty_like(xd))
    torch.cuda.synchronize()
    return dict(x=x, logits=logits, weights=weights, ids=ids.cpu(), w=w.cpu(), act=act.cpu(), y=y.cpu(), out=out.cpu())


def hold_stages(tag, r, dtype):
    ug, dn = r["weights"]
    ids = r["ids"].long()
    T, k = ids.shape
    h = lambda v: 0.5 * R.ulp_of(v, dtype)      # noqa: E731
    ref = R.up_gate_silu_ref(r["x"], ug.cpu() if ug.numel() < 1 << 24 else ug, ids)
    up, gate = ref["up"], ref["gate"]
    du = a_of(ref["up_mag"]) + h(up.abs() + a_of(ref["up_mag"]))
    dg = a_of(ref["gate_mag"]) + h(gate.abs() + a_of(ref["gate_mag"]))
    s = R.silu(gate)
    ds = 1.1 * dg + 2.0 ** -21 * s.abs() + h(s.abs() + 1.1 * dg)
    e = up.abs() * ds + s.abs() * du + du * ds
    want = up * s
    bound = e + h(want.abs() + e)
    err = (r["act"].double() - want).abs()
    r_act = float((err / bound).max())
    y_ref, y_mag = R.down_ref(r["act"], dn.cpu() if dn.numel() < 1 << 24 else dn, ids)
    r_y = float(((r["y"].double() - y_ref).abs() / a_of(y_mag).clamp(min=1e-300)).max())
    o_ref, o_mag = R.combine_ref(r["y"], r["w"])
    o_bound = a_of(o_mag) + h(o_ref.abs() + a_of(o_mag))
    r_out = float(((r["out"].double() - o_ref).abs() / o_bound).max())
    print(f"\n[{tag} {dtype}] error / bound: act {r_act:.3f}  y {r_y:.3f}  out {r_out:.3f}  "
          f"(max |act| {float(r['act'].abs().max()):.3g}, max |out| {float(r['out'].abs().max()):.3g})")
    assert float(r["act"].abs().max()) > 0 and float(r["out"].abs().max()) > 0
    assert r_act <= 1.0, (tag, "act", r_act)
    assert r_y <= 1.0, (tag, "y", r_y)
    assert r_out <= 1.0, (tag, "out", r_out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H, I", GEOMETRIES)
@pytest.mark.parametrize("case, T", STEPS)
def test_stages_meet_the_derived_bound(case, T, H, I, dtype):
    E, k, _ = CASES[case]
    g = torch.Generator().manual_seed(100 + T + H + I)
    r = chain(g, T, E, k, H, I, dtype, norm=(T % 2 == 1))
    assert torch.equal(r["ids"].long(), R.route_ref(r["logits"], k, T % 2 == 1)[0])
    hold_stages(f"{case} T={T} H={H} I={I}", r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_block_at_a_real_width(dtype):
    g = torch.Generator().manual_seed(21)
    r = chain(g, 8, 128, 8, 2048, 768, dtype, w_scale=0.02)
    hold_stages("Qwen3-30B-A3B T=8", r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pattern", ["all_to_one", "empty_expert"])
def test_stages_on_lopsided_routing(pattern, dtype):
    g = torch.Generator().manual_seed(22)
    T, E, k, H, I = 33, 8, 2, 256, 192
    logits = gapped_logits(g, T, E, torch.float32).clamp(max=0.0) - 1.0
    if pattern == "all_to_one":
        logits[:, 5], logits[:, 2] = 3.0, 2.0                # every token: experts 5 then 2 — three tiles each, six empty
    else:
        logits[:, 3] = -9.0                                  # expert 3 has no row
    r = chain(g, T, E, k, H, I, dtype, logits=logits)
    if pattern == "all_to_one":
        assert r["ids"].tolist() == [[5, 2]] * T
    else:
        assert 3 not in r["ids"]
    hold_stages(pattern, r, dtype)


# ---- row independence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E, k, H, I", [(8, 2, 256, 128), (128, 8, 256, 192), (4, 2, 256, 192)])
def test_a_token_s_bits_do_not_depend_on_its_neighbours(E, k, H, I, dtype):
    g = torch.Generator().manual_seed(23)
    T = 33
    full = chain(g, T, E, k, H, I, dtype)
    x, logits, weights = full["x"], full["logits"], full["weights"]
    perm = torch.randperm(T, generator=g)
    mixed = chain(g, T, E, k, H, I, dtype, x=x[perm], logits=logits[perm], weights=weights)
    assert torch.equal(mixed["out"].view(torch.int16), full["out"][perm].view(torch.int16))
    assert torch.equal(mixed["ids"], full["ids"][perm])
    for t in (0, 7, 15, 16, 32):
        alone = chain(g, 1, E, k, H, I, dtype, x=x[t:t + 1], logits=logits[t:t + 1], weights=weights)
        assert torch.equal(alone["out"].view(torch.int16), full["out"][t:t + 1].view(torch.int16)), t
        assert torch.equal(alone["w"], full["w"][t:t + 1])
    # ... nor on which tokens share its tile: the same rows inside a batch that sends everything else to its experts
    crowd = logits.clone()
    crowd[1:] = logits[0]
    crowded = chain(g, T, E, k, H, I, dtype, x=x, logits=crowd, weights=weights)
    assert torch.equal(crowded["out"][0].view(torch.int16), full["out"][0].view(torch.int16))


def test_moe_ffn_walks_a_long_step_in_token_blocks():
    """600 tokens x top-8 is more than one call takes: moe_ffn gives the bits of the five launches on each block of rows."""
    from swiftllm_amd.worker.kernels.linear import linear
    g = torch.Generator().manual_seed(24)
    T, E, k, H, I = 600, 128, 8, 256, 128
    dtype = torch.bfloat16
    x = torch.randn((T, H), generator=g).to(dtype).to(DEV)
    router = (torch.randn((E, H), generator=g) * 0.3).to(dtype).to(DEV)
    weights = ((torch.randn((E, 2 * I, H), generator=g) * 0.05).to(dtype).to(DEV),
               (torch.randn((E, H, I), generator=g) * 0.05).to(dtype).to(DEV))
    assert T * k > M.max_pairs()
    tap = []
    out = M.moe_ffn(x, router, *weights, k, True, tap=tap, layer_id=3)
    assert len(tap) == 1 and tap[0][0] == 3 and tuple(tap[0][1].shape) == (T, k) and tuple(tap[0][2].shape) == (T, k)
    logits = linear(x, router, False)
    block = M.max_pairs() // k
    assert 0 < block < T
    for t0 in range(0, T, block):
        part = chain(g, min(block, T - t0), E, k, H, I, dtype, x=x[t0:t0 + block].cpu(), logits=logits[t0:t0 + block].cpu(),
                     weights=weights)
        assert torch.equal(part["out"].view(torch.int16), out[t0:t0 + block].cpu().view(torch.int16)), t0
        assert torch.equal(part["ids"], tap[0][1][t0:t0 + block]) and torch.equal(part["w"], tap[0][2][t0:t0 + block])
    assert float(out.float().abs().max()) > 0 and M.moe_ffn(x[:0], router, *weights, k, True).shape == (0, H)
    with pytest.raises(_hip.HipLibraryError):
        M.moe_align(torch.zeros((T, k), dtype=torch.int32, device=DEV), E)


# ---- memory ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T, E, k, H, I", [(17, 8, 2, 256, 192), (33, 128, 8, 256, 128), (1, 4, 2, 256, 128)])
def test_nothing_is_read_or_written_outside_the_buffers(T, E, k, H, I, dtype):
    g = torch.Generator().manual_seed(25)
    tiles = M.max_tiles(T, k, E)
    code = _hip.dtype_code(dtype)
    ops = dict(
        x=Op(torch.randn((T, H), generator=g).to(dtype), stride=H + 8),
        logits=Op(gapped_logits(g, T, E, torch.float32), skew=4, stride=E + 3),
        up_gate=Op((torch.randn((E, 2 * I, H), generator=g) * 0.05).to(dtype)),
        down=Op((torch.randn((E, H, I), generator=g) * 0.05).to(dtype)),
        ids=Op(torch.zeros((T, k), dtype=torch.int32), skew=4, out=True),
        w=Op(torch.zeros((T, k), dtype=torch.float32), skew=4, out=True),
        tile_rows=Op(torch.zeros((tiles * 16,), dtype=torch.int32), skew=4, out=True),
        tile_experts=Op(torch.zeros((tiles,), dtype=torch.int32), skew=4, out=True),
        act=Op(torch.zeros((T * k, I), dtype=dtype), out=True),
        y=Op(torch.zeros((T * k, H), dtype=torch.float32), out=True),
        out=Op(torch.zeros((T, H), dtype=dtype), stride=H + 8, out=True),
    )

    def call(v):
        p, s = _hip.ptr, _hip.stream()
        _hip.call("swl_moe_route", p(v["ids"]), p(v["w"]), p(v["logits"]), T, E, k, 1, E + 3, M.LOGITS_F32, s)
        _hip.call("swl_moe_align", p(v["tile_rows"]), p(v["tile_experts"]), p(v["ids"]), T, k, E, tiles, s)
        _hip.call("swl_moe_up_gate_silu", p(v["act"]), p(v["x"]), p(v["up_gate"]), p(v["tile_rows"]), p(v["tile_experts"]),
                  tiles, T, k, H, I, E, H + 8, code, s)
        _hip.call("swl_moe_down", p(v["y"]), p(v["act"]), p(v["down"]), p(v["tile_rows"]), p(v["tile_experts"]), tiles, T, k,
                  H, I, E, code, s)
        _hip.call("swl_moe_combine", p(v["out"]), p(v["y"]), p(v["w"]), T, k, H, H + 8, code, s)

    want = run_case(ops, call, DEV, sync=torch.cuda.synchronize)
    assert bool(torch.isfinite(want["out"].float()).all()) and float(want["out"].float().abs().max()) > 0
    assert sorted(want["tile_rows"][want["tile_rows"] >= 0].tolist()) == list(range(T * k))
