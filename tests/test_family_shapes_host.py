"""tests/_family_shapes.py held to the code that reads a checkpoint's config (no GPU): every admitted geometry parses
through LlamaModelConfig to the (N, K) pairs the table's function gives, every pair is a shape the weight-streaming
GEMMs take, and the layer route of the new hidden sizes defers the RMSNorm only where the deferred kernel's chunking
(1024 columns per workgroup) divides the row."""
import pytest
import torch

from swiftllm_amd import EngineConfig, LlamaModelConfig, _hip
from swiftllm_amd.worker.layers import transformer_layer as T
from swiftllm_amd.worker.kernels.rmsnorm import deferred_norm_ok

from _family_shapes import GEOMETRIES, config_json, geometry, projection_shapes

CHECKPOINTS = ["Llama-3-8B", "Qwen3-0.6B", "Qwen3-1.7B", "Qwen3-4B", "Qwen3-8B", "Qwen3-32B", "Qwen2.5-3B", "Qwen2.5-72B",
               "Mistral-7B", "Mistral-Nemo", "Mistral-Small-24B"]


def test_the_table_lists_the_admitted_checkpoints():
    assert list(GEOMETRIES) == CHECKPOINTS


@pytest.mark.parametrize("name", CHECKPOINTS)
def test_geometry_parses_and_yields_the_projection_shapes(name):
    g = geometry(name)
    c = LlamaModelConfig(config_json(name))
    assert (c.model_type, c.hidden_size, c.num_q_heads, c.num_kv_heads, c.head_dim, c.ffn_inter_dim, c.vocab_size) == \
        tuple(g[f] for f in ("family", "hidden", "q_heads", "kv_heads", "head_dim", "intermediate", "vocab"))
    assert c.q_size == g["q_heads"] * g["head_dim"]
    assert (c.qk_norm, c.qkv_bias) == (g["family"] == "qwen3", g["family"] == "qwen2")
    kv_size = c.num_kv_heads * c.head_dim
    want = dict(qkv=(c.q_size + 2 * kv_size, c.hidden_size), o=(c.hidden_size, c.q_size),
                up_gate=(2 * c.ffn_inter_dim, c.hidden_size), down=(c.hidden_size, c.ffn_inter_dim),
                lm_head=(c.vocab_size, c.hidden_size))
    assert projection_shapes(name) == want
    for proj, (n, k) in want.items():
        # kernels/linear.py `packable`'s shape rule: whole 32-row and 128-column tiles
        assert n % 32 == 0 and k % 128 == 0, (name, proj, n, k)
    assert want["up_gate"][0] % 64 == 0          # the SiLU-gate entries pair up and gate rows


def test_the_gpu_test_pairs_are_the_table_s():
    """The (N, K) list of tests/test_gpu_family_shapes.py names its sources: each is what the table gives."""
    s = projection_shapes
    assert s("Qwen3-4B")["o"] == (2560, 4096) and s("Qwen3-1.7B")["down"] == (2048, 6144)
    assert s("Qwen3-4B")["qkv"] == (6144, 2560) and s("Qwen3-4B")["down"] == (2560, 9728)
    assert s("Qwen2.5-3B")["down"] == (2048, 11008) and s("Mistral-Nemo")["o"] == (5120, 4096)
    assert s("Qwen3-32B")["qkv"] == (10240, 5120) and s("Qwen3-32B")["down"] == (5120, 25600)
    assert s("Qwen2.5-72B")["down"] == (8192, 29568) and s("Qwen2.5-72B")["lm_head"] == (152064, 8192)
    assert s("Qwen3-0.6B")["down"] == (1024, 3072) and s("Qwen3-0.6B")["o"] == (1024, 2048)
    assert s("Qwen3-0.6B")["lm_head"] == (151936, 1024) and s("Mistral-Nemo")["lm_head"][0] == 131072


def _facts(name, dtype):
    g = geometry(name)
    shapes = {p: nk for p, nk in projection_shapes(name).items() if p != "lm_head"}
    ecfg = EngineConfig(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                        max_seqs_in_block_table=64, max_blocks_per_seq=32, max_batch_size=256, max_tokens_in_batch=4096)
    plain = g["family"] in ("qwen2", "qwen3") or g["q_heads"] * g["head_dim"] != g["hidden"]
    return T.layer_facts(ecfg, dtype, g["hidden"], g["q_heads"], g["head_dim"], shapes, frozenset(shapes), _hip.load(),
                         plain_qkv=plain)


def _step(m, kind=T.Input.TENSOR):
    return T.StepFacts(input=kind, prefill=False, m=m, ignore_kvcache=False, positions=True, split=False, verify=False,
                       chunked=False, lora=False)


def test_hidden_2560_never_defers_the_norm(monkeypatch):
    def forbidden(name, *args):
        raise AssertionError(f"the route decision launched {name}")
    monkeypatch.setattr(_hip, "call", forbidden)
    assert not any(deferred_norm_ok(m, 2560, torch.bfloat16) for m in range(1, 33))
    for dtype in (torch.bfloat16, torch.float16):
        f = _facts("Qwen3-4B", dtype)
        assert f.hidden == 2560 and f.plain_qkv and f.o_splits > 1 and f.fly_ffn
        for m in range(1, 257):
            for kind in (T.Input.TENSOR, T.Input.SLABS):
                r = T.decide_route(f, _step(m, kind))
                assert r.o_ffn is T.OFfn.SPLITK_FUSED and r.attn_norm is T.AttnNorm.FUSED, (dtype, m, kind)
                assert r.down is T.Down.SPLITK and r.qkv is T.QKV.ROTARY_THEN_STORE


@pytest.mark.parametrize("name", ["Qwen3-0.6B", "Qwen3-1.7B", "Qwen2.5-3B", "Qwen3-32B", "Mistral-Nemo", "Mistral-Small-24B"])
def test_hidden_1024_2048_5120_defer_at_bfloat16_up_to_32_rows(name, monkeypatch):
    def forbidden(entry, *args):
        raise AssertionError(f"the route decision launched {entry}")
    monkeypatch.setattr(_hip, "call", forbidden)
    bf16, f16 = _facts(name, torch.bfloat16), _facts(name, torch.float16)
    assert bf16.hidden in (1024, 2048, 5120) and bf16.plain_qkv and bf16.o_splits > 1 and bf16.fly_ffn
    for m in range(1, 257):
        for kind in (T.Input.TENSOR, T.Input.SLABS):
            r = T.decide_route(bf16, _step(m, kind))
            assert r.o_ffn is (T.OFfn.SPLITK_DEFERRED if m <= 32 else T.OFfn.SPLITK_FUSED), (name, m, kind)
            assert r.down is T.Down.SPLITK
            assert T.decide_route(f16, _step(m, kind)).o_ffn is T.OFfn.SPLITK_FUSED     # float16 keeps the exact roundings
