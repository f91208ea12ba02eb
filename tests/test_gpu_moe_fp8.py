"""FP8 (e4m3) expert weights (csrc/moe_fp8.h, moe_fp8.hip, moe_fp8_wide.hip), float16 and bfloat16.

Expert GEMMs: every stage against fp64 on the DEQUANTISED stacks (code * scale, exact in fp64) with `hold_stages` of
tests/test_gpu_moe_kernels.py, its fp32 allowance widened by the one extra fp32 multiply (the row scale): a(mag) = (2^-18 +
2^-24) mag. K (H for up/gate, I for down) takes the three kinds of value the walk has — 8 waves x 64-wide steps x 4 in flight
= 2048 a pipelined pass: fewer than 8 steps (128, 192, 256), a pass plus a remainder (2112), a last round that ends mid-way
(576). Row magnitudes are spread over 2^6. Model: HF's fp32 eager forward holding the dequantised expert values, routers forced
to our choices, gate 1.5 x the distance of HF's own 16-bit forward."""
import pytest
import torch

from swiftllm_amd.worker.kernels import moe as M

import _moe_ref as R
import test_gpu_moe_kernels as K16
from test_gpu_model_families import TORCH_DTYPE, _generate, _prompts, _serve
from test_gpu_moe_model import KINDS, SEED, _load

pytestmark = pytest.mark.gpu

DEV, DTYPES = "cuda", [torch.float16, torch.bfloat16]
GEOMETRIES = [(256, 128), (2112, 192), (576, 2112)]
bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)      # noqa: E731
_STACKS = {}


def quantised(w):                                           # [rows, K] -> (codes, scale) the way the loader makes them
    scale, inv = M.row_scales(w)
    return M.quantise_rows(w, inv, torch.empty(w.shape, dtype=M.FP8, device=DEV)), scale


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantiser_codes_equal_the_host_twin(dtype):
    g = torch.Generator().manual_seed(41)
    rows, k = 37, 64 * 16 + 48                              # a wave strides a row by 1024 elements: one partial stride
    w = torch.randn((rows, k), generator=g) * torch.exp2(torch.randint(-8, 4, (rows, 1), generator=g).float())
    w[3] = 0.0                                              # a zero row: scale 1
    w[5, 7], w[6, 9] = -9.0 * float(w[5].abs().max()), 9.0 * float(w[6].abs().max())       # the row maximum: -448 / +448
    w[8] = torch.randn(k, generator=g) * 2.0 ** -12
    w[8, 0] = 16.0                                          # the rest of the row lands in the e4m3 subnormals (< 2^-6)
    w = w.to(dtype)
    codes, scale = quantised(w.to(DEV))
    host_scale, host_inv = M.row_scales(w)
    assert torch.equal(scale.cpu(), host_scale) and float(host_scale[3]) == 1.0
    want = w.float().mul(host_inv[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    got = codes.cpu().view(torch.uint8)
    assert torch.equal(got, want)
    assert not bool(got[3].any()) and int(got[5, 7]) == 0xFE and int(got[6, 9]) == 0x7E
    assert bool((((got[8] & 0x78) == 0) & ((got[8] & 7) != 0)).any())


def stacks(E, H, I, dtype):
    """FP8 stacks + scales of a geometry (device) and their dequantised fp64 values: made once, shared by its cases."""
    key = (E, H, I, dtype)
    if key not in _STACKS:
        _STACKS.clear()
        g = torch.Generator(device=DEV).manual_seed(42 + E + H + I)
        out = []
        for rows, k in ((2 * I, H), (H, I)):
            w = torch.randn((E * rows, k), generator=g, device=DEV) * 0.02
            w *= torch.exp2(torch.randint(-3, 4, (E * rows, 1), generator=g, device=DEV).float())
            codes, scale = quantised(w.to(dtype))
            codes, scale = codes.view(E, rows, k), scale.view(E, rows)
            out.append((codes, scale, codes.float().double() * scale.double()[..., None]))
        _STACKS[key] = out
    return _STACKS[key]


def chain(E, k, H, I, dtype, x, logits, forms=(0,)):
    """The launches on FP8 stacks, once per form; every intermediate on the CPU, in hold_stages' layout."""
    (ug, ug_s, ug_d), (dn, dn_s, dn_d) = stacks(E, H, I, dtype)
    ids, w = M.moe_route(logits.to(DEV), k, True)
    rows, experts = M.moe_align(ids, E)
    got = []
    for rt in forms:
        act = M.moe_up_gate_silu(x.to(DEV), ug, rows, experts, k, row_tiles=rt, up_gate_scale=ug_s)
        y = M.moe_down(act, dn, rows, experts, k, row_tiles=rt, down_scale=dn_s)
        out = M.moe_combine(y, w, torch.empty(x.shape, dtype=dtype, device=DEV))
        got.append(dict(x=x, weights=(ug_d, dn_d), ids=ids.cpu(), w=w.cpu(), act=act.cpu(), y=y.cpu(), out=out.cpu()))
    return got


def step_logits(g, T, E, pattern):
    logits = K16.gapped_logits(g, T, E, torch.float32)
    if pattern == "all_to_one":                             # every token: experts 3 then 1; the others have no row
        logits = logits.clamp(max=0.0) - 1.0
        logits[:, 3], logits[:, 1] = 3.0, 2.0
    elif pattern == "empty_expert":
        logits[:, 2] = -9.0
    return logits


@pytest.mark.parametrize("T", [1, 17, 33])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H, I", GEOMETRIES)
@pytest.mark.parametrize("E, k", [(4, 2), (128, 8)])
def test_fp8_stages_meet_the_derived_bound(E, k, H, I, dtype, T, monkeypatch):
    monkeypatch.setattr(K16, "a_of", lambda mag: mag * (2.0 ** -18 + 2.0 ** -24))
    g = torch.Generator().manual_seed(400 + T + H)
    pattern = {33: "all_to_one", 17: "empty_expert"}.get(T, "free") if E == 4 else "free"
    x = torch.randn((T, H), generator=g).to(dtype)
    r, = chain(E, k, H, I, dtype, x, step_logits(g, T, E, pattern))
    if pattern == "all_to_one":
        assert r["ids"].tolist() == [[3, 1]] * T
    K16.hold_stages(f"fp8 {pattern} E={E} T={T} H={H} I={I}", r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E, k, T, H, I, pattern", [(4, 2, 200, 256, 128, "free"), (4, 2, 33, 576, 192, "all_to_one")],
                         ids=["100_rows_an_expert", "ragged_last_tile"])
def test_the_wide_form_writes_the_bits_of_the_16_row_form(E, k, T, H, I, pattern, dtype):
    g = torch.Generator().manual_seed(43)
    x = torch.randn((T, H), generator=g).to(dtype)
    base, *wide = chain(E, k, H, I, dtype, x, step_logits(g, T, E, pattern), forms=(0,) + M.WIDE_ROW_TILES)
    assert int(torch.bincount(base["ids"].flatten()).max()) >= (64 if pattern == "free" else 33)
    for r in wide:
        assert torch.equal(bits(r["act"]), bits(base["act"])) and torch.equal(bits(r["y"]), bits(base["y"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_s_bits_do_not_depend_on_its_step(dtype):
    g = torch.Generator().manual_seed(44)
    T, E, k, H, I = 33, 128, 8, 576, 192
    x, logits = torch.randn((T, H), generator=g).to(dtype), step_logits(g, T, E, "free")
    full, = chain(E, k, H, I, dtype, x, logits)
    for t in (0, 16, 32):
        alone, = chain(E, k, H, I, dtype, x[t:t + 1], logits[t:t + 1])
        assert torch.equal(bits(alone["out"]), bits(full["out"][t:t + 1])), t
        assert torch.equal(bits(alone["y"]), bits(full["y"][t * k:(t + 1) * k])), t


STEPS, _MODELS = 4, {}


@pytest.fixture
def served(tmp_path_factory):
    """(path, HF fp32 model with the DEQUANTISED expert values, prompts, streams, logits, tapped ids per prompt and layer) of
    a kind and dtype with FP8 expert weights: one tapped (eager) run, once per module."""
    def get(kind, dtype):
        if (kind, dtype) not in _MODELS:
            path = str(tmp_path_factory.mktemp(f"fp8_{kind}_{dtype}"))
            hf = R.make_moe_checkpoint(path, kind, TORCH_DTYPE[dtype], SEED[kind])
            prompts = _prompts(SEED[kind], hf.config.vocab_size)
            model = _load(path, dtype, moe_weight_dtype="fp8_e4m3")
            inter = model.model_config.moe_inter_dim
            for lw, (gate_up, down) in zip(model.weight.layers, R.experts_of(hf)):
                assert lw.expert_up_gate.dtype == lw.expert_down.dtype == torch.float8_e4m3fn       # one byte an element
                assert lw.expert_up_gate_scale.shape == gate_up.shape[:2] and lw.expert_down_scale.shape == down.shape[:2]
                ug = (lw.expert_up_gate.float() * lw.expert_up_gate_scale[..., None]).cpu()
                gate_up.copy_(torch.cat((ug[:, inter:], ug[:, :inter]), dim=1))         # HF keeps [gate ; up]
                down.copy_((lw.expert_down.float() * lw.expert_down_scale[..., None]).cpu())
            model.moe_tap = tap = []
            streams, logits = _generate(model, prompts, steps=STEPS)
            layers, starts = model.model_config.num_layers, [sum(len(p) for p in prompts[:i]) for i in range(len(prompts))]
            assert len(tap) == (STEPS + 1) * layers
            ids = [[torch.cat([tap[layer][1][s:s + len(p)]] + [tap[st * layers + layer][1][i:i + 1]
                                                               for st in range(1, STEPS + 1)]).long()
                    for layer in range(layers)] for i, (p, s) in enumerate(zip(prompts, starts))]
            del model
            _MODELS[(kind, dtype)] = (path, hf, prompts, streams, logits, ids)
        return _MODELS[(kind, dtype)]
    return get


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("kind", KINDS)
def test_fp8_model_logits_stay_within_the_gate(served, kind, dtype):
    _, hf, prompts, streams, logits, ids = served(kind, dtype)
    rows = [p + s[:-1] for p, s in zip(prompts, streams)]
    at = lambda ref: torch.stack([r[0][len(p) - 1:] for r, p in zip(ref, prompts)], dim=1)     # noqa: E731
    lg32 = at(R.forced_logits(hf, rows, torch.float32, ids))
    lg16 = at(R.forced_logits(hf, rows, TORCH_DTYPE[dtype], ids))
    d_ours, d_ref16 = (logits - lg32).abs().max().item(), (lg16 - lg32).abs().max().item()
    print(f"\n[fp8 {kind} {dtype}] d_ours {d_ours:.3e}  d_ref16 {d_ref16:.3e}  ratio {d_ours / d_ref16:.2f}")
    assert lg32.shape == logits.shape and d_ours <= 1.5 * d_ref16, (kind, d_ours, d_ref16)


@pytest.mark.parametrize("kind, dtype", [("qwen3_moe", "bfloat16"), ("mixtral", "float16")])
def test_fp8_model_replays_and_chunks_to_the_same_streams(served, kind, dtype):
    path, _, prompts, base_streams, base_logits, _ = served(kind, dtype)
    replay = _load(path, dtype, moe_weight_dtype="fp8_e4m3")          # no tap: decode steps replay their hipGraph
    streams, logits = _generate(replay, prompts, steps=STEPS)
    assert replay.replay.captures >= 1 and streams == base_streams and torch.equal(logits, base_logits)
    chunked = _load(path, dtype, moe_weight_dtype="fp8_e4m3", max_prefill_chunk=16)
    _, (got,) = _serve(chunked, [prompts], STEPS + 1)
    assert [(err, toks) for err, toks in got] == [(None, s) for s in base_streams]
