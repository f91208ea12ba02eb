"""The row-tile form of the expert GEMMs (csrc/moe_wide.hip), float16 and bfloat16, on the SAME routing and tile tables as
the 16-row kernels: `act` / `y` meet the derived bounds of tests/test_gpu_moe_kernels.py (`hold_stages`) and equal the 16-row
outputs bit for bit. H 256 is one k step per wave, H 320 / I 192 uneven k steps (and waves with none); the steps give runs of
4, 3 and 1 tiles, empty experts, one-tile experts with unused tiles behind, 64 tiles per expert, and a single pair."""
import pytest
import torch

from swiftllm_amd import _hip
from swiftllm_amd.worker.kernels import moe as M
from _arena import Op, run_case
from test_gpu_moe_kernels import gapped_logits, hold_stages

pytestmark = pytest.mark.gpu

DEV, DTYPES, FORMS = "cuda", [torch.float16, torch.bfloat16], M.WIDE_ROW_TILES
STEPS = {"seven_tiles": (4, 2, 200), "lopsided": (8, 2, 33), "one_tile_experts": (128, 8, 40), "largest": (4, 2, 2048),
         "one_pair": (4, 2, 1)}
bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)      # noqa: E731


def step_logits(g, name, T, E):
    logits = gapped_logits(g, T, E, torch.float32)
    if name == "lopsided":                                  # every token: experts 5 then 2 — three tiles each, six empty
        logits = logits.clamp(max=0.0) - 1.0
        logits[:, 5], logits[:, 2] = 3.0, 2.0
    return logits


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H, I", [(256, 128), (320, 192)])
@pytest.mark.parametrize("name", list(STEPS))
def test_wide_stages_meet_the_bound_and_equal_the_16_row_bits(name, H, I, dtype):
    E, k, T = STEPS[name]
    g = torch.Generator().manual_seed(300 + T + H)
    x = torch.randn((T, H), generator=g).to(dtype)
    ug = (torch.randn((E, 2 * I, H), generator=g) * 0.05).to(dtype).to(DEV)
    dn = (torch.randn((E, H, I), generator=g) * 0.05).to(dtype).to(DEV)
    ids, w = M.moe_route(step_logits(g, name, T, E).to(DEV), k, True)
    rows, experts = M.moe_align(ids, E)
    got = {}
    for rt in (0,) + FORMS:
        act = M.moe_up_gate_silu(x.to(DEV), ug, rows, experts, k, row_tiles=rt)
        y = M.moe_down(act, dn, rows, experts, k, row_tiles=rt)
        out = M.moe_combine(y, w, torch.empty((T, H), dtype=dtype, device=DEV))
        got[rt] = dict(x=x, weights=(ug, dn), ids=ids.cpu(), w=w.cpu(), act=act.cpu(), y=y.cpu(), out=out.cpu())
    for rt in FORMS:
        hold_stages(f"wide {rt} {name} H={H} I={I}", got[rt], dtype)
        assert torch.equal(bits(got[rt]["act"]), bits(got[0]["act"])), rt
        assert torch.equal(bits(got[rt]["y"]), bits(got[0]["y"])), rt


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_route_boundary_keeps_a_token_s_bits(dtype):
    g = torch.Generator().manual_seed(31)
    T, E, k, H, I = 600, 8, 2, 256, 128
    x = torch.randn((T, H), generator=g).to(dtype).to(DEV)
    router = (torch.randn((E, H), generator=g) * 0.3).to(dtype).to(DEV)
    ug = (torch.randn((E, 2 * I, H), generator=g) * 0.05).to(dtype).to(DEV)
    dn = (torch.randn((E, H, I), generator=g) * 0.05).to(dtype).to(DEV)
    base = M.moe_ffn(x, router, ug, dn, k, True, wide_tiles=0)
    assert float(base.float().abs().max()) > 0 and M.wide_row_tiles(T, k, E, H, I) in FORMS
    for wt in FORMS + (-1,):
        assert torch.equal(bits(M.moe_ffn(x, router, ug, dn, k, True, wide_tiles=wt)), bits(base)), wt
    assert M.wide_row_tiles(1, k, E, H, I) == 0             # alone, the chooser takes the 16-row form
    for t in (0, 16, 599):
        assert torch.equal(bits(M.moe_ffn(x[t:t + 1], router, ug, dn, k, True)), bits(base[t:t + 1])), t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", FORMS)
@pytest.mark.parametrize("name, T", [("lopsided", 33), ("seven_tiles", 100)])
def test_nothing_is_read_or_written_outside_the_buffers(name, T, rt, dtype):
    g = torch.Generator().manual_seed(32)
    E, k, H, I = STEPS[name][0], 2, 256, 128
    ids, _ = M.moe_route(step_logits(g, name, T, E).to(DEV), k, True)
    rows, experts = M.moe_align(ids, E)
    tiles, code, p = experts.numel(), _hip.dtype_code(dtype), _hip.ptr
    ops = dict(
        x=Op(torch.randn((T, H), generator=g).to(dtype), stride=H + 8),
        up_gate=Op((torch.randn((E, 2 * I, H), generator=g) * 0.05).to(dtype)),
        down=Op((torch.randn((E, H, I), generator=g) * 0.05).to(dtype)),
        tile_rows=Op(rows.cpu(), skew=4), tile_experts=Op(experts.cpu(), skew=4),
        act=Op(torch.zeros((T * k, I), dtype=dtype), out=True),
        y=Op(torch.zeros((T * k, H), dtype=torch.float32), out=True),
    )

    def call(v):
        _hip.call("swl_moe_up_gate_silu_wide", p(v["act"]), p(v["x"]), p(v["up_gate"]), p(v["tile_rows"]),
                  p(v["tile_experts"]), tiles, T, k, H, I, E, H + 8, rt, code, _hip.stream())
        _hip.call("swl_moe_down_wide", p(v["y"]), p(v["act"]), p(v["down"]), p(v["tile_rows"]), p(v["tile_experts"]), tiles,
                  T, k, H, I, E, rt, code, _hip.stream())

    want = run_case(ops, call, DEV, sync=torch.cuda.synchronize)
    assert bool(torch.isfinite(want["y"]).all()) and bool((want["y"].abs().amax(1) > 0).all())


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_a_model_serves_the_same_tokens_and_logits_in_both_forms(dtype, tmp_path):
    from test_gpu_moe_model import R, TORCH_DTYPE, _generate, _load
    R.make_moe_checkpoint(str(tmp_path), "mixtral", TORCH_DTYPE[dtype], 1)
    prompt = torch.randint(3, 512, (200,), generator=torch.Generator().manual_seed(33)).tolist()
    got = []
    for wt in (0, 4):
        model = _load(str(tmp_path), dtype, moe_wide_tiles=wt)
        got.append(_generate(model, [prompt], steps=4))
        del model
    assert got[0][0] == got[1][0] and torch.equal(bits(got[0][1][-1]), bits(got[1][1][-1]))
