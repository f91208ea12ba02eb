"""A 16-bit dense checkpoint served with dense_weight_dtype "fp8_e4m3" (csrc/gemm_fp8_row.h): tiny 2-layer Llama and dense
Qwen3 checkpoints, built as tests/test_gpu_gemm_fp8_block.py builds its own but left in 16 bits. Three prompts, one of 80
tokens (its prefill step takes the dequantising route), then 8 decode steps on the FP8 kernels. Gate: the distance of our
logits to HF's fp32 eager forward holding the DEQUANTISED projections is at most 1.5 x the distance of HF's own 16-bit forward
of those values; graph replay writes the bits of eager launches."""
import json
import os

import pytest
import torch

from swiftllm_amd.worker.kernels import linear_fp8 as LB
from swiftllm_amd.worker.kernels import linear_fp8_row as L
from swiftllm_amd.worker.kernels.moe import row_scales

from _families_ref import make_hf_checkpoint
from test_gpu_gemm_fp8_block import KINDS
from test_gpu_model_families import TORCH_DTYPE, _generate, _hf_at_our_positions, _load, _prompts

pytestmark = pytest.mark.gpu

STEPS, _MODELS = 8, {}


@pytest.fixture
def served(tmp_path_factory):
    """(path, HF fp32 model holding the dequantised projections, prompts, streams, logits) of a kind and dtype: once a module."""
    def get(kind, dtype):
        if (kind, dtype) not in _MODELS:
            name, overrides, seed = KINDS[kind]
            path = str(tmp_path_factory.mktemp(f"dense_fp8_row_{kind}_{dtype}"))
            hf = make_hf_checkpoint(path, name, TORCH_DTYPE[dtype], seed, **overrides)
            if kind == "llama":
                with open(os.path.join(path, "config.json"), encoding="utf-8") as f:
                    config = dict(json.load(f), model_type="llama", architectures=["LlamaForCausalLM"])
                with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
                    json.dump(config, f)
            for key, p in hf.named_parameters():            # the contract's torch twin, per checkpoint tensor
                if key.endswith("_proj.weight"):
                    w = p.data.to("cuda", TORCH_DTYPE[dtype])
                    scale, inv = row_scales(w)
                    code = w.float().mul(inv[:, None]).clamp(-448, 448).to(L.FP8).float()
                    p.data.copy_((code * scale[:, None]).to(TORCH_DTYPE[dtype]).float().cpu())
            prompts = _prompts(seed, hf.config.vocab_size)
            prompts[-1] = (prompts[-1] * 2)[:80]
            LB._scratch.clear()
            model = _load(path, dtype, dense_weight_dtype="fp8_e4m3")
            lw = model.weight.layers[0]
            assert lw.qkv_proj.dtype == L.FP8 and lw.down_scale.shape == (lw.down_proj.shape[0],) and lw.o_bscale is None
            assert getattr(lw.qkv_proj, "_swl_packed", None) is None and model.weight.lm_head.dtype == TORCH_DTYPE[dtype]
            (scratch,) = LB._scratch.values()               # reserved at load: the largest projection
            assert scratch.numel() == max(t.numel() for t in vars(lw).values() if isinstance(t, torch.Tensor) and t.dtype == L.FP8)
            streams, logits = _generate(model, prompts, steps=STEPS)
            assert model.replay.captures >= 1
            del model
            _MODELS[(kind, dtype)] = (path, hf, prompts, streams, logits)
        return _MODELS[(kind, dtype)]
    return get


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_logits_stay_within_the_gate(served, kind, dtype):
    path, hf, prompts, streams, logits = served(kind, dtype)
    lg32 = _hf_at_our_positions(hf, prompts, streams, torch.float32)
    lg16 = _hf_at_our_positions(hf, prompts, streams, TORCH_DTYPE[dtype])
    d_ours, d_ref16 = (logits - lg32).abs().max().item(), (lg16 - lg32).abs().max().item()
    print(f"\n[dense fp8 row {kind} {dtype}] d_ours {d_ours:.3e}  d_ref16 {d_ref16:.3e}  ratio {d_ours / d_ref16:.2f}")
    assert lg32.shape == logits.shape and d_ours <= 1.5 * d_ref16, (kind, d_ours, d_ref16)


@pytest.mark.parametrize("kind, dtype", [("llama", "bfloat16"), ("qwen3", "float16")])
def test_graph_replay_gives_the_bits_of_eager_launches(served, kind, dtype):
    path, _, prompts, base_streams, base_logits = served(kind, dtype)
    eager = _load(path, dtype, dense_weight_dtype="fp8_e4m3", use_hip_graph=False)
    streams, logits = _generate(eager, prompts, steps=STEPS)
    assert eager.replay.captures == 0 and streams == base_streams and torch.equal(logits, base_logits)
