"""Dense block-scaled FP8 projections (csrc/gemm_fp8_block.h, gemm_fp8_block.hip, kernels/linear_fp8.py), float16 and bfloat16.

Kernels: every element against fp64 on the DEQUANTISED weights (code * block scale, exact in fp64). The bound is the one of
tests/test_gpu_moe_kernels.py and tests/test_gpu_moe_fp8_block.py, |got - ref| <= h(|ref| + a) + a with h half an ulp of T and
a = (2^-18 + F 2^-24) sum |x_k w_k|, where F counts the fp32 roundings behind the MFMAs in the chain the header documents: one
fold per 128-wide k block and one add per further k slice, F = ceil(K / 128) + k_splits - 1 for the split the launch ran (the
forced one, else the chooser's for that form's output columns); steps of more than 64 rows go through the library GEMM, which
has neither: F = 0. The SiLU-gate form takes the up_gate_silu bound of tests/test_gpu_moe_kernels.py with this a. Neighbouring blocks differ by 2^6 in
magnitude in both directions and across segments, so a wrong row-block, k-block or segment index is 64 x off. Model: tiny
checkpoints rewritten into the published layout (the Llama case is the Mistral maker at Llama's shape with model_type
"llama": the same tensors and the same function), HF's fp32 eager forward holding the dequantised values, gate 1.5 x the
distance of HF's own 16-bit forward. Every test fails on a tree without the entries or the option."""
import json
import os

import pytest
import torch

from swiftllm_amd.model_config import LlamaModelConfig
from swiftllm_amd.worker.kernels import linear_fp8 as L
from swiftllm_amd.worker.weight import dequantise_blocks

import _moe_ref as R
from _families_ref import make_hf_checkpoint
from test_gpu_model_families import TORCH_DTYPE, _generate, _hf_at_our_positions, _load, _prompts
from test_gpu_moe_fp8 import bits
from test_gpu_moe_fp8_block import block_quantise, expand, to_block_fp8

pytestmark = pytest.mark.gpu

DEV, DTYPES = "cuda", [torch.float16, torch.bfloat16]
# (the issue's four, and one whose 15 column tiles are no multiple of a workgroup's 4: its last workgroup has a spare wave)
GEOMETRIES = [((256,), 128), ((192, 64, 64), 576), ((2112,), 192), ((192, 192), 2112), ((208, 16, 16), 192)]
_WEIGHTS = {}


def weights(segments, K):
    """(codes [N, K], bscale, dequantised fp64 [N, K] on the CPU) of a geometry: a 2^+-3 checkerboard over the scale rows."""
    if (segments, K) not in _WEIGHTS:
        g = torch.Generator(device=DEV).manual_seed(60 + sum(segments) + K)
        codes, scales, deq, first = [], [], [], 0
        for rows in segments:
            rb, kb = L.blocks(rows), L.blocks(K)
            board = (first + torch.arange(rb, device=DEV)[:, None] + torch.arange(kb, device=DEV)[None, :]) % 2
            c, s = block_quantise(torch.randn((rows, K), generator=g, device=DEV) * 0.02 * expand(torch.exp2(6.0 * board - 3.0), rows, K))
            codes.append(c), scales.append(s), deq.append((c.double() * expand(s.double(), rows, K)).cpu())
            first += rb
        _WEIGHTS[(segments, K)] = (torch.cat(codes).contiguous(), torch.cat(scales).contiguous(), torch.cat(deq))
    return _WEIGHTS[(segments, K)]


def a_of(mag, K, ks, n_out):
    """ks: the forced split, 0 for the chooser's at (n_out, K), None for the library GEMM (no folds, no slices)."""
    F = 0 if ks is None else L.blocks(K) + (ks or L.choose_splits(n_out, K)) - 1
    return mag * (2.0 ** -18 + F * 2.0 ** -24)


def splits_of(segments, K):
    return (0, 1, L.max_splits(K)) if K == 2112 else (0,)


@pytest.mark.parametrize("M", [1, 17, 33, 64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("segments, K", GEOMETRIES)
def test_every_element_meets_the_derived_bound(segments, K, dtype, M):
    codes, bscale, deq = weights(segments, K)
    x = torch.randn((M, K), generator=torch.Generator().manual_seed(600 + M + K)).to(dtype)
    xd, h = x.double(), lambda v: 0.5 * R.ulp_of(v, dtype)      # noqa: E731
    ref, mag = xd @ deq.T, xd.abs() @ deq.abs().T
    for ks in splits_of(segments, K):
        a = a_of(mag, K, ks, sum(segments))
        got = L.linear_fp8_block(x.to(DEV), codes, bscale, segments, k_splits=ks).cpu().double()
        worst = float(((got - ref).abs() / (h(ref.abs() + a) + a)).max())
        print(f"\n[gemm {segments} K={K} M={M} ks={ks} {dtype}] error / bound {worst:.3f}")
        assert float(got.abs().max()) > 0 and worst <= 1.0, (segments, K, M, ks, worst)
        if len(segments) != 2:
            continue
        inter, a = segments[0], a_of(mag, K, ks, segments[0])
        act = L.linear_silu_gate_fp8_block(x.to(DEV), codes, bscale, inter, k_splits=ks).cpu().double()
        (up, gate), (au, ag) = (ref[:, :inter], ref[:, inter:]), (a[:, :inter], a[:, inter:])
        du, dg, s = au + h(up.abs() + au), ag + h(gate.abs() + ag), R.silu(gate)
        ds = 1.1 * dg + 2.0 ** -21 * s.abs() + h(s.abs() + 1.1 * dg)
        e = up.abs() * ds + s.abs() * du + du * ds
        worst = float(((act - up * s).abs() / (e + h((up * s).abs() + e))).max())
        print(f"[silu_gate ks={ks}] error / bound {worst:.3f}")
        assert float(act.abs().max()) > 0 and worst <= 1.0, (segments, K, M, ks, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("segments, K", GEOMETRIES[1:4])
def test_a_row_s_bits_depend_on_that_row_only_and_launches_repeat(segments, K, dtype):
    codes, bscale, _ = weights(segments, K)
    x = torch.randn((64, K), generator=torch.Generator().manual_seed(61)).to(dtype).to(DEV)
    forms = [lambda v, ks: L.linear_fp8_block(v, codes, bscale, segments, k_splits=ks)]
    if len(segments) == 2:
        forms.append(lambda v, ks: L.linear_silu_gate_fp8_block(v, codes, bscale, segments[0], k_splits=ks))
    for form in forms:
        for ks in splits_of(segments, K):
            full = form(x, ks)
            assert torch.equal(bits(full), bits(form(x, ks)))
            for t in (0, 16, 63):
                assert torch.equal(bits(form(x[t:t + 1], ks)), bits(full[t:t + 1])), (ks, t)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantise_writes_the_loader_s_bits_and_serves_steps_beyond_64_rows(dtype):
    segments, K = GEOMETRIES[1]
    codes, bscale, deq = weights(segments, K)
    got = L.dequantise_fp8_block(codes, bscale, segments, torch.empty(codes.shape, dtype=dtype, device=DEV))
    first, row = 0, 0
    for rows in segments:                                   # the loader's dequantiser, a segment (= a checkpoint tensor) at a time
        want = dequantise_blocks(codes[row:row + rows], bscale[first:first + L.blocks(rows)], dtype)
        assert torch.equal(bits(got[row:row + rows]), bits(want))
        first, row = first + L.blocks(rows), row + rows
    x = torch.randn((65, K), generator=torch.Generator().manual_seed(62)).to(dtype)
    y = L.linear_fp8_block(x.to(DEV), codes, bscale, segments).cpu().double()
    w16 = got.cpu().double()                                # (the 16-bit image: the library GEMM's own operand)
    ref, a = x.double() @ w16.T, a_of(x.double().abs() @ w16.abs().T, K, None, sum(segments))
    assert float(((y - ref).abs() / (0.5 * R.ulp_of(ref.abs() + a, dtype) + a)).max()) <= 1.0


# ---- model ---------------------------------------------------------------------------------------------------------------
KINDS = {"llama": ("mistral", dict(head_dim=64, num_key_value_heads=2), 4), "qwen3": ("qwen3_d128", {}, 1)}
STEPS, _MODELS = 4, {}


@pytest.fixture
def served(tmp_path_factory):
    """(path, HF fp32 model holding the DEQUANTISED projections, prompts, streams, logits) of a kind and dtype, loaded with
    dense_weight_dtype "fp8_block": once per module. The last prompt is 80 tokens: its prefill step takes the dequantising
    route (more than 64 rows), the decode steps the FP8 kernels."""
    def get(kind, dtype):
        if (kind, dtype) not in _MODELS:
            name, overrides, seed = KINDS[kind]
            path = str(tmp_path_factory.mktemp(f"dense_fp8_{kind}_{dtype}"))
            hf = make_hf_checkpoint(path, name, TORCH_DTYPE[dtype], seed, **overrides)
            file = to_block_fp8(path)
            if kind == "llama":
                with open(os.path.join(path, "config.json"), encoding="utf-8") as f:
                    config = dict(json.load(f), model_type="llama", architectures=["LlamaForCausalLM"])
                with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
                    json.dump(config, f)
            for key, p in hf.named_parameters():
                if key + "_scale_inv" in file:
                    p.data.copy_(dequantise_blocks(file[key], file[key + "_scale_inv"], TORCH_DTYPE[dtype]).float())
            prompts = _prompts(seed, hf.config.vocab_size)
            prompts[-1] = (prompts[-1] * 2)[:80]
            L._scratch.clear()
            model = _load(path, dtype, dense_weight_dtype="fp8_block")
            (scratch,) = L._scratch.values()                # reserved at load: the largest projection
            assert scratch.numel() == max(t.numel() for t in vars(model.weight.layers[0]).values()
                                          if isinstance(t, torch.Tensor) and t.dtype == L.FP8)
            assert model.weight.layers[0].qkv_proj.dtype == L.FP8 and model.weight.layers[0].down_bscale is not None
            streams, logits = _generate(model, prompts, steps=STEPS)
            assert model.replay.captures >= 1
            assert list(L._scratch.values())[0] is scratch and len(L._scratch) == 1     # the 118-row prefill used it
            del model
            _MODELS[(kind, dtype)] = (path, hf, prompts, streams, logits)
        return _MODELS[(kind, dtype)]
    return get


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_dense_fp8_model_logits_stay_within_the_gate(served, kind, dtype):
    path, hf, prompts, streams, logits = served(kind, dtype)
    lg32 = _hf_at_our_positions(hf, prompts, streams, torch.float32)
    lg16 = _hf_at_our_positions(hf, prompts, streams, TORCH_DTYPE[dtype])
    d_ours, d_ref16 = (logits - lg32).abs().max().item(), (lg16 - lg32).abs().max().item()
    print(f"\n[dense fp8 {kind} {dtype}] d_ours {d_ours:.3e}  d_ref16 {d_ref16:.3e}  ratio {d_ours / d_ref16:.2f}")
    assert lg32.shape == logits.shape and d_ours <= 1.5 * d_ref16, (kind, d_ours, d_ref16)
    with pytest.raises(ValueError, match="quantised dense model"):      # the same directory, the option off
        LlamaModelConfig.load_from_model_path(path)


@pytest.mark.parametrize("kind, dtype", [("llama", "bfloat16"), ("qwen3", "float16")])
def test_graph_replay_gives_the_bits_of_eager_launches(served, kind, dtype):
    path, _, prompts, base_streams, base_logits = served(kind, dtype)
    eager = _load(path, dtype, dense_weight_dtype="fp8_block", use_hip_graph=False)
    streams, logits = _generate(eager, prompts, steps=STEPS)
    assert eager.replay.captures == 0 and streams == base_streams and torch.equal(logits, base_logits)
