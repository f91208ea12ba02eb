"""Block-scaled FP8 checkpoints (csrc/moe_fp8_block.h, moe_fp8_block.hip, moe_fp8_block_wide.hip), float16 and bfloat16.

Expert GEMMs: every stage against fp64 on the DEQUANTISED stacks (code * block scale, exact in fp64) with `hold_stages` of
tests/test_gpu_moe_kernels.py. Its fp32 allowance grows by the folds: each rounds the running sum once, by at most 2^-24 of
the sum of absolute products, and an element is folded ceil(K / 64) times — a(mag) = (2^-18 + ceil(max(H, I) / 64) 2^-24) mag
(DESIGN.md section 4.21). Neighbouring blocks differ by 2^6 in magnitude in both directions, so a wrong row-block or k-block
index is 64 x off. Geometries: one block each way (256, 128); partial last blocks, a pipelined pass plus a remainder and a
gate half that starts at a non-multiple of 128 (2112, 192), (576, 2112). Loader: a tiny checkpoint of each kind rewritten into
the published layout. Model: HF's fp32 eager forward holding the dequantised values, routers forced to our choices, gate 1.5 x
the distance of HF's own 16-bit forward. Every test fails on a tree that cannot load such a directory
or has no block entries."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file, save_file

from swiftllm_amd.model_config import LlamaModelConfig
from swiftllm_amd.worker.kernels import moe as M
from swiftllm_amd.worker.weight import dequantise_blocks, load_weights

import _moe_ref as R
import test_gpu_moe_kernels as K16
from test_gpu_model_families import TORCH_DTYPE, _generate, _prompts, _serve
from test_gpu_moe_fp8 import bits, step_logits
from test_gpu_moe_model import KINDS, SEED, _load

pytestmark = pytest.mark.gpu

DEV, DTYPES, B = "cuda", [torch.float16, torch.bfloat16], 128
GEOMETRIES = [(256, 128), (2112, 192), (576, 2112)]
QUANT = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [B, B]}
_STACKS = {}


def expand(scale, rows, cols):                              # [..., rb, kb] -> [..., rows, cols]
    return scale.repeat_interleave(B, -2)[..., :rows, :].repeat_interleave(B, -1)[..., :cols]


def block_quantise(w):
    """[..., rows, k] fp32 -> (codes, scale [..., ceil(rows / 128), ceil(k / 128)]): scale = amax / 448 per block."""
    r, c = w.shape[-2:]
    rb, cb = -(-r // B), -(-c // B)
    p = w.new_zeros(*w.shape[:-2], rb * B, cb * B)
    p[..., :r, :c] = w
    scale = p.view(*w.shape[:-2], rb, B, cb, B).abs().amax(dim=(-3, -1)) / 448.0
    return (w / expand(scale, r, c)).to(M.FP8).contiguous(), scale


def stacks(E, H, I):
    """Block-scaled stacks of a geometry (device), in the kernels' layout, and their dequantised fp64 values."""
    if (E, H, I) not in _STACKS:
        _STACKS.clear()
        g = torch.Generator(device=DEV).manual_seed(52 + E + H + I)
        out = []
        for halves, rows, k in ((2, I, H), (1, H, I)):
            w = torch.randn((E, halves, rows, k), generator=g, device=DEV) * 0.02
            rb, kb = M.block_scales_shape(rows, k)
            board = (torch.arange(rb, device=DEV)[:, None] + torch.arange(kb, device=DEV)[None, :]) % 2
            codes, scale = block_quantise(w * expand(torch.exp2(6.0 * board - 3.0), rows, k))
            deq = (codes.double() * expand(scale.double(), rows, k)).view(E, halves * rows, k)
            out.append((codes.view(E, halves * rows, k), scale.view(E, halves * rb, kb).contiguous(), deq))
        _STACKS[(E, H, I)] = out
    return _STACKS[(E, H, I)]


def chain(E, k, H, I, dtype, x, logits, forms=(0,)):
    """The launches on block-scaled stacks, once per form; every intermediate on the CPU, in hold_stages' layout."""
    (ug, ug_s, ug_d), (dn, dn_s, dn_d) = stacks(E, H, I)
    ids, w = M.moe_route(logits.to(DEV), k, True)
    rows, experts = M.moe_align(ids, E)
    got = []
    for rt in forms:
        act = M.moe_up_gate_silu(x.to(DEV), ug, rows, experts, k, row_tiles=rt, up_gate_bscale=ug_s)
        y = M.moe_down(act, dn, rows, experts, k, row_tiles=rt, down_bscale=dn_s)
        out = M.moe_combine(y, w, torch.empty(x.shape, dtype=dtype, device=DEV))
        got.append(dict(x=x, weights=(ug_d, dn_d), ids=ids.cpu(), w=w.cpu(), act=act.cpu(), y=y.cpu(), out=out.cpu()))
    return got


@pytest.mark.parametrize("T", [1, 17, 33])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H, I", GEOMETRIES)
@pytest.mark.parametrize("E, k", [(4, 2), (128, 8)])
def test_block_stages_meet_the_derived_bound(E, k, H, I, dtype, T, monkeypatch):
    folds = -(-max(H, I) // 64)
    monkeypatch.setattr(K16, "a_of", lambda mag: mag * (2.0 ** -18 + folds * 2.0 ** -24))
    g = torch.Generator().manual_seed(500 + T + H)
    pattern = {33: "all_to_one", 17: "empty_expert"}.get(T, "free") if E == 4 else "free"
    x = torch.randn((T, H), generator=g).to(dtype)
    r, = chain(E, k, H, I, dtype, x, step_logits(g, T, E, pattern))
    if pattern == "all_to_one":
        assert r["ids"].tolist() == [[3, 1]] * T
    K16.hold_stages(f"fp8 block {pattern} E={E} T={T} H={H} I={I}", r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E, k, T, H, I, pattern", [(4, 2, 200, 256, 128, "free"), (4, 2, 33, 576, 192, "all_to_one")],
                         ids=["100_rows_an_expert", "ragged_last_tile"])
def test_the_wide_forms_write_the_bits_of_the_16_row_form(E, k, T, H, I, pattern, dtype):
    g = torch.Generator().manual_seed(53)
    x = torch.randn((T, H), generator=g).to(dtype)
    base, *wide = chain(E, k, H, I, dtype, x, step_logits(g, T, E, pattern), forms=(0,) + M.WIDE_ROW_TILES)
    assert int(torch.bincount(base["ids"].flatten()).max()) >= (64 if pattern == "free" else 33)
    for r in wide:                                          # (a row_tiles of 4 is served by the 2-tile kernels)
        assert torch.equal(bits(r["act"]), bits(base["act"])) and torch.equal(bits(r["y"]), bits(base["y"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_s_bits_do_not_depend_on_its_step(dtype):
    g = torch.Generator().manual_seed(54)
    T, E, k, H, I = 33, 128, 8, 576, 192
    x, logits = torch.randn((T, H), generator=g).to(dtype), step_logits(g, T, E, "free")
    full, = chain(E, k, H, I, dtype, x, logits)
    for t in (0, 16, 32):
        alone, = chain(E, k, H, I, dtype, x[t:t + 1], logits[t:t + 1])
        assert torch.equal(bits(alone["out"]), bits(full["out"][t:t + 1])), t
        assert torch.equal(bits(alone["y"]), bits(full["y"][t * k:(t + 1) * k])), t


def to_block_fp8(path):
    """Rewrite a 16-bit checkpoint into the published layout: codes + weight_scale_inv for q/k/v/o_proj and every expert
    projection, quantization_config in config.json. Returns the file's tensors."""
    file = os.path.join(path, "model.safetensors")
    out = {}
    for key, w in load_file(file).items():
        if key.endswith("_proj.weight") or (".experts." in key and key.endswith(".weight")):
            out[key], out[key + "_scale_inv"] = block_quantise(w.float())
        else:
            out[key] = w
    save_file(out, file, metadata={"format": "pt"})
    with open(os.path.join(path, "config.json"), encoding="utf-8") as f:
        config = dict(json.load(f), quantization_config=QUANT)
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(config, f)
    return out


@pytest.mark.parametrize("streaming", [True, False], ids=["streaming", "per_tensor"])
@pytest.mark.parametrize("kind, dtype", [("qwen3_moe", "bfloat16"), ("mixtral", "float16")])
def test_the_loader_keeps_codes_and_scales_and_dequantises_the_rest(tmp_path, kind, dtype, streaming):
    R.make_moe_checkpoint(str(tmp_path), kind, TORCH_DTYPE[dtype], SEED[kind])
    file = to_block_fp8(str(tmp_path))
    cfg = LlamaModelConfig.load_from_model_path(str(tmp_path))
    weight = load_weights(cfg, TORCH_DTYPE[dtype], str(tmp_path), device=DEV, fuse_qkv=streaming, streaming=streaming)
    mod, up, gate, down = {"qwen3_moe": ("mlp.", "up_proj", "gate_proj", "down_proj"),
                           "mixtral": ("block_sparse_moe.", "w3", "w1", "w2")}[kind]
    inter, (rb_i, _) = cfg.moe_inter_dim, M.block_scales_shape(cfg.moe_inter_dim, cfg.hidden_size)
    raw = lambda t: t.cpu().view(torch.uint8)               # noqa: E731
    for li, lw in enumerate(weight.layers):
        assert lw.expert_up_gate.dtype == lw.expert_down.dtype == M.FP8 and lw.expert_up_gate_scale is None
        for e in range(cfg.num_experts):
            name = lambda proj, what: f"model.layers.{li}.{mod}experts.{e}.{proj}.{what}"     # noqa: E731
            for proj, stack, rows, bscale, brows in ((up, lw.expert_up_gate, slice(0, inter), lw.expert_up_gate_bscale, slice(0, rb_i)),
                                                     (gate, lw.expert_up_gate, slice(inter, 2 * inter), lw.expert_up_gate_bscale, slice(rb_i, 2 * rb_i)),
                                                     (down, lw.expert_down, slice(None), lw.expert_down_bscale, slice(None))):
                assert torch.equal(raw(stack[e, rows]), raw(file[name(proj, "weight")])), (li, e, proj)
                assert torch.equal(bscale[e, brows].cpu(), file[name(proj, "weight_scale_inv")]), (li, e, proj)
        attn = f"model.layers.{li}.self_attn."
        want = {p: dequantise_blocks(file[attn + p + ".weight"], file[attn + p + ".weight_scale_inv"], TORCH_DTYPE[dtype])
                for p in ("q_proj", "o_proj")}
        q = lw.qkv_proj[:cfg.q_size] if streaming else lw.q_proj
        assert torch.equal(bits(q.cpu()), bits(want["q_proj"])) and torch.equal(bits(lw.o_proj.cpu()), bits(want["o_proj"]))


STEPS, _MODELS = 4, {}


@pytest.fixture
def served(tmp_path_factory):
    """(path, HF fp32 model holding the DEQUANTISED values, prompts, streams, logits, tapped ids per prompt and layer) of a
    kind and dtype from a block-scaled FP8 checkpoint: one tapped (eager) run, once per module."""
    def get(kind, dtype):
        if (kind, dtype) not in _MODELS:
            path = str(tmp_path_factory.mktemp(f"fp8_block_{kind}_{dtype}"))
            hf = R.make_moe_checkpoint(path, kind, TORCH_DTYPE[dtype], SEED[kind])
            file = to_block_fp8(path)
            prompts = _prompts(SEED[kind], hf.config.vocab_size)
            model = _load(path, dtype)                      # moe_weight_dtype "auto"
            cfg = model.model_config
            h, inter = cfg.hidden_size, cfg.moe_inter_dim
            for li, (lw, (gate_up, down)) in enumerate(zip(model.weight.layers, R.experts_of(hf))):
                ug = (lw.expert_up_gate.float().view(-1, 2, inter, h) *
                      expand(lw.expert_up_gate_bscale.view(-1, 2, *M.block_scales_shape(inter, h)), inter, h)).cpu()
                gate_up.copy_(torch.cat((ug[:, 1], ug[:, 0]), dim=1))                   # HF keeps [gate ; up]
                down.copy_((lw.expert_down.float() * expand(lw.expert_down_bscale, h, inter)).cpu())
                for p in ("q_proj", "k_proj", "v_proj", "o_proj"):
                    key = f"model.layers.{li}.self_attn.{p}.weight"
                    getattr(hf.model.layers[li].self_attn, p).weight.data.copy_(
                        dequantise_blocks(file[key], file[key + "_scale_inv"], TORCH_DTYPE[dtype]).float())
            model.moe_tap = tap = []
            streams, logits = _generate(model, prompts, steps=STEPS)
            layers, starts = cfg.num_layers, [sum(len(p) for p in prompts[:i]) for i in range(len(prompts))]
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
def test_block_model_logits_stay_within_the_gate(served, kind, dtype):
    _, hf, prompts, streams, logits, ids = served(kind, dtype)
    rows = [p + s[:-1] for p, s in zip(prompts, streams)]
    at = lambda ref: torch.stack([r[0][len(p) - 1:] for r, p in zip(ref, prompts)], dim=1)     # noqa: E731
    lg32 = at(R.forced_logits(hf, rows, torch.float32, ids))
    lg16 = at(R.forced_logits(hf, rows, TORCH_DTYPE[dtype], ids))
    d_ours, d_ref16 = (logits - lg32).abs().max().item(), (lg16 - lg32).abs().max().item()
    print(f"\n[fp8 block {kind} {dtype}] d_ours {d_ours:.3e}  d_ref16 {d_ref16:.3e}  ratio {d_ours / d_ref16:.2f}")
    assert lg32.shape == logits.shape and d_ours <= 1.5 * d_ref16, (kind, d_ours, d_ref16)


@pytest.mark.parametrize("kind, dtype", [("qwen3_moe", "bfloat16"), ("mixtral", "float16")])
def test_block_model_replays_and_chunks_to_the_same_streams(served, kind, dtype):
    path, _, prompts, base_streams, base_logits, _ = served(kind, dtype)
    replay = _load(path, dtype, moe_weight_dtype="fp8_e4m3")          # no tap: decode steps replay their hipGraph
    assert replay.weight.layers[0].expert_up_gate_bscale is not None  # (either option serves the checkpoint's own codes)
    streams, logits = _generate(replay, prompts, steps=STEPS)
    assert replay.replay.captures >= 1 and streams == base_streams and torch.equal(logits, base_logits)
    chunked = _load(path, dtype, max_prefill_chunk=16)
    _, (got,) = _serve(chunked, [prompts], STEPS + 1)
    assert [(err, toks) for err, toks in got] == [(None, s) for s in base_streams]
