"""A 16-bit dense checkpoint served with dense_weight_dtype "mxfp4" (csrc/gemm_mxfp4.h): the tiny 2-layer Llama and dense
Qwen3 checkpoints of tests/test_gpu_dense_fp8_row_model.py (hidden 256, intermediate 512), bfloat16. Three prompts, one of 80
tokens (the dequantising route), then 8 decode steps on the MXFP4 kernels. Gate: our logits lie within 1.5 x the distance of
HF's own bfloat16 forward from HF's fp32 eager forward, both holding the DEQUANTISED projections;
graph replay writes the bits of eager launches; the layers hold codes and scales only."""
import json
import os

import pytest
import torch

from swiftllm_amd.worker.kernels import linear_fp8 as LB
from swiftllm_amd.worker.kernels import linear_mxfp4 as L

from _families_ref import make_hf_checkpoint
from test_gpu_gemm_fp8_block import KINDS
from test_gpu_gemm_mxfp4 import twin
from test_gpu_model_families import _generate, _hf_at_our_positions, _load, _prompts

pytestmark = pytest.mark.gpu

STEPS, DTYPE, _MODELS = 8, "bfloat16", {}


@pytest.fixture
def served(tmp_path_factory):
    """(path, HF fp32 model holding the dequantised projections, prompts, streams, logits) of a kind: once a module."""
    def get(kind):
        if kind not in _MODELS:
            name, overrides, seed = KINDS[kind]
            path = str(tmp_path_factory.mktemp(f"dense_mxfp4_{kind}"))
            hf = make_hf_checkpoint(path, name, torch.bfloat16, seed, **overrides)
            if kind == "llama":
                with open(os.path.join(path, "config.json"), encoding="utf-8") as f:
                    config = dict(json.load(f), model_type="llama", architectures=["LlamaForCausalLM"])
                with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
                    json.dump(config, f)
            for key, p in hf.named_parameters():            # the contract's torch twin, per checkpoint tensor
                if key.endswith("_proj.weight"):
                    p.data.copy_(twin(p.data.to(torch.bfloat16))[0])
            prompts = _prompts(seed, hf.config.vocab_size)
            prompts[-1] = (prompts[-1] * 2)[:80]
            LB._scratch.clear()
            model = _load(path, DTYPE, dense_weight_dtype="mxfp4")
            lw, held = model.weight.layers[0], 0
            for attr in ("qkv", "o", "up_gate", "down"):    # codes and scales only: N K / 2 + one byte per 32 k (padded groups)
                codes, scales = getattr(lw, attr + "_proj"), getattr(lw, attr + "_scale")
                n, k = codes.shape[0], 2 * codes.shape[1]
                assert codes.dtype == scales.dtype == torch.uint8 and getattr(codes, "_swl_packed", None) is None
                held += codes.numel() + scales.numel()
            sixteen = [t for t in vars(lw).values() if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16]
            # one byte per 32 k, in groups of four k tiles: K = 256 pads two tiles to four, K = 512 is exact
            want = sum(n * k // 2 + n // 16 * 256 * -(-k // 512) for n, k in _shapes(model))
            assert all(t.dim() == 1 for t in sixteen) and held == want
            assert model.weight.lm_head.dtype == torch.bfloat16
            (scratch,) = LB._scratch.values()               # reserved at load: the largest projection's 16-bit image
            assert scratch.numel() == 2 * max(getattr(lw, a + "_proj").numel() for a in ("qkv", "o", "up_gate", "down"))
            streams, logits = _generate(model, prompts, steps=STEPS)
            assert model.replay.captures >= 1
            del model
            _MODELS[kind] = (path, hf, prompts, streams, logits)
        return _MODELS[kind]
    return get


def _shapes(model):
    c = model.model_config
    h, q, kv, i = c.hidden_size, c.q_size, c.num_kv_heads * c.head_dim, c.ffn_inter_dim
    return [(q + 2 * kv, h), (h, q), (2 * i, h), (h, i)]


@pytest.mark.parametrize("kind", list(KINDS))
def test_logits_stay_within_the_gate(served, kind):
    path, hf, prompts, streams, logits = served(kind)
    lg32 = _hf_at_our_positions(hf, prompts, streams, torch.float32)
    lg16 = _hf_at_our_positions(hf, prompts, streams, torch.bfloat16)
    d_ours, d_ref16 = (logits - lg32).abs().max().item(), (lg16 - lg32).abs().max().item()
    print(f"\n[dense mxfp4 {kind}] d_ours {d_ours:.3e}  d_ref16 {d_ref16:.3e}  ratio {d_ours / d_ref16:.2f}")
    assert lg32.shape == logits.shape and d_ours <= 1.5 * d_ref16, (kind, d_ours, d_ref16)


@pytest.mark.parametrize("kind", list(KINDS))
def test_graph_replay_gives_the_bits_of_eager_launches(served, kind):
    path, _, prompts, base_streams, base_logits = served(kind)
    eager = _load(path, DTYPE, dense_weight_dtype="mxfp4", use_hip_graph=False)
    streams, logits = _generate(eager, prompts, steps=STEPS)
    assert eager.replay.captures == 0 and streams == base_streams and torch.equal(logits, base_logits)
