"""Mixture-of-experts models without a device: config parsing and refusals, both weight loaders against HuggingFace's fused
expert parameters, the layer route, and the routing-forced reference of tests/_moe_ref.py against unhooked HF."""
import itertools

import pytest
import torch

from swiftllm_amd import EngineConfig, _hip
from swiftllm_amd.model_config import LlamaModelConfig
from swiftllm_amd.worker import weight as W
from swiftllm_amd.worker.layers import transformer_layer as T

import _moe_ref as R

# the published config.json files, reduced to the fields that are read
QWEN3_30B_A3B = dict(model_type="qwen3_moe", hidden_act="silu", hidden_size=2048, intermediate_size=6144,
                     moe_intermediate_size=768, num_hidden_layers=48, num_attention_heads=32, num_key_value_heads=4,
                     head_dim=128, num_experts=128, num_experts_per_tok=8, norm_topk_prob=True, decoder_sparse_step=1,
                     mlp_only_layers=[], vocab_size=151936, max_position_embeddings=40960, rms_norm_eps=1e-6,
                     rope_theta=1000000.0, rope_scaling=None, sliding_window=None, use_sliding_window=False,
                     tie_word_embeddings=False, attention_bias=False)
MIXTRAL_8X7B = dict(model_type="mixtral", hidden_act="silu", hidden_size=4096, intermediate_size=14336, num_hidden_layers=32,
                    num_attention_heads=32, num_key_value_heads=8, num_local_experts=8, num_experts_per_tok=2,
                    vocab_size=32000, max_position_embeddings=32768, rms_norm_eps=1e-5, rope_theta=1000000.0,
                    sliding_window=None, tie_word_embeddings=False)
LLAMA = dict(model_type="llama", hidden_act="silu", hidden_size=4096, intermediate_size=14336, num_hidden_layers=32,
             num_attention_heads=32, num_key_value_heads=8, vocab_size=128256, max_position_embeddings=8192, rms_norm_eps=1e-5)


def test_published_configs_parse():
    q = LlamaModelConfig(QWEN3_30B_A3B)
    assert (q.num_experts, q.num_experts_per_tok, q.moe_inter_dim, q.norm_topk_prob) == (128, 8, 768, True)
    assert q.is_moe and q.qk_norm and not q.qkv_bias and q.head_dim == 128 and q.q_size == 4096 and q.hidden_size == 2048
    assert (q.num_q_heads, q.num_kv_heads, q.num_layers, q.rope_theta) == (32, 4, 48, 1000000.0)
    assert LlamaModelConfig(dict(QWEN3_30B_A3B, norm_topk_prob=False)).norm_topk_prob is False
    # transformers 5 writes the count of either family as num_local_experts
    renamed = dict({k: v for k, v in QWEN3_30B_A3B.items() if k != "num_experts"}, num_local_experts=128)
    assert LlamaModelConfig(renamed).num_experts == 128
    m = LlamaModelConfig(MIXTRAL_8X7B)
    assert (m.num_experts, m.num_experts_per_tok, m.moe_inter_dim, m.norm_topk_prob) == (8, 2, 14336, True)
    assert m.is_moe and not m.qk_norm and not m.qkv_bias and m.head_dim == 128 and m.q_size == 4096
    assert _hip.load().swl_moe_supported(2048, 768, 128, 8, _hip.SWL_BF16) == 1
    assert _hip.load().swl_moe_supported(4096, 14336, 8, 2, _hip.SWL_F16) == 1


def test_dense_configs_parse_as_before():
    c = LlamaModelConfig(LLAMA)
    assert (c.num_experts, c.num_experts_per_tok, c.moe_inter_dim, c.norm_topk_prob, c.is_moe) == (0, 0, 0, False, False)
    assert c.ffn_inter_dim == 14336 and c.head_dim == 128 and c.model_type == "llama"
    d = LlamaModelConfig(dict(LLAMA, model_type="mistral", sliding_window=None))
    assert not d.is_moe and d.ffn_inter_dim == 14336
    with pytest.raises(KeyError):
        LlamaModelConfig({k: v for k, v in LLAMA.items() if k != "intermediate_size"})


@pytest.mark.parametrize("change, reason", [
    (dict(model_type="qwen2_moe"), "shared expert"),
    (dict(mlp_only_layers=[0, 3]), "mlp_only_layers"),
    (dict(decoder_sparse_step=2), "decoder_sparse_step"),
    (dict(num_experts_per_tok=129), "exceeds the 128 experts"),
    (dict(num_experts=512), "at most 256 experts"),
    (dict(num_experts_per_tok=17), "top-16"),
    (dict(hidden_size=2080), "hidden_size % 64"),
    (dict(moe_intermediate_size=760), "intermediate size % 32"),
    (dict(num_experts=None), "mixture-of-experts config without"),
    (dict(num_experts_per_tok=0), "mixture-of-experts config without"),
    (dict(moe_intermediate_size=None), "mixture-of-experts config without"),
    (dict(rope_scaling=dict(rope_type="yarn", factor=4.0)), "rope_type"),      # dense Qwen3's refusals are inherited
])
def test_refusals_give_their_reason(change, reason):
    with pytest.raises(ValueError, match=reason):
        LlamaModelConfig(dict(QWEN3_30B_A3B, **change))


def test_mixtral_refusals():
    with pytest.raises(ValueError, match="mixture-of-experts config without"):
        LlamaModelConfig({k: v for k, v in MIXTRAL_8X7B.items() if k != "num_local_experts"})
    with pytest.raises(ValueError, match="exceeds the 8 experts"):
        LlamaModelConfig(dict(MIXTRAL_8X7B, num_experts_per_tok=9))
    with pytest.raises(ValueError, match="intermediate size % 32"):
        LlamaModelConfig(dict(MIXTRAL_8X7B, intermediate_size=14352))


# ---- loaders -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["qwen3_moe", "mixtral"])
def test_both_loaders_assemble_the_expert_stacks(kind, tmp_path):
    import json
    import os
    import safetensors
    path = str(tmp_path)
    hf = R.make_moe_checkpoint(path, kind, torch.bfloat16, 3)
    cfg = LlamaModelConfig.load_from_model_path(path)
    assert cfg.is_moe and cfg.model_type == kind
    with safetensors.safe_open(os.path.join(path, "model.safetensors"), framework="pt") as f:
        keys = set(f.keys())
    mod, up, gate, down = W._moe_names(cfg)
    for name in (f"model.layers.1.{mod}gate.weight", f"model.layers.1.{mod}experts.{cfg.num_experts - 1}.{up}.weight",
                 f"model.layers.0.{mod}experts.0.{gate}.weight", f"model.layers.0.{mod}experts.1.{down}.weight"):
        assert name in keys, (name, sorted(keys)[:12])        # the per-expert names of the published checkpoints
    assert json.load(open(os.path.join(path, "config.json")))["model_type"] == kind
    inter = cfg.moe_inter_dim
    loaded = [W.load_weights(cfg, torch.bfloat16, path, device="cpu", fuse_qkv=True, streaming=s) for s in (True, False)]
    for weight in loaded:
        assert weight.projection_tensors() and all(t.dim() == 2 for t in weight.projection_tensors())   # experts: not packed
        for layer, (gate_up, down_proj), router in zip(weight.layers, R.experts_of(hf), R.routers(hf)):
            assert not hasattr(layer, "up_gate_proj") and not hasattr(layer, "down_proj")
            assert tuple(layer.expert_up_gate.shape) == (cfg.num_experts, 2 * inter, cfg.hidden_size)
            assert tuple(layer.expert_down.shape) == (cfg.num_experts, cfg.hidden_size, inter)
            assert layer.expert_up_gate.is_contiguous() and layer.expert_down.is_contiguous()
            assert torch.equal(layer.expert_up_gate[:, :inter].float(), gate_up[:, inter:])      # ours [up ; gate], HF [gate ; up]
            assert torch.equal(layer.expert_up_gate[:, inter:].float(), gate_up[:, :inter])
            assert torch.equal(layer.expert_down.float(), down_proj)
            assert torch.equal(layer.router.float(), router.weight.detach())
            assert layer.qkv_proj is not None and (layer.q_norm is not None) == (kind == "qwen3_moe")
    for a, b in zip(loaded[0].layers, loaded[1].layers):
        assert torch.equal(a.expert_up_gate, b.expert_up_gate) and torch.equal(a.qkv_proj, b.qkv_proj)
    dummy = W.load_weights(cfg, torch.float16, path, use_dummy=True, device="cpu")
    assert tuple(dummy.layers[0].expert_down.shape) == (cfg.num_experts, cfg.hidden_size, inter)
    assert float(dummy.layers[1].expert_up_gate.abs().max()) <= 2.0 ** -9 and dummy.layers[0].router is not None


# ---- route ---------------------------------------------------------------------------------------------------------------
SHAPES = dict(qkv=(5120, 2048), o=(2048, 4096), up_gate=(2 * 768, 2048), down=(2048, 768))     # Qwen3-30B-A3B


def _facts(dtype, packed=True, shapes=SHAPES, hidden=2048, **kw):
    engine = {k: kw.pop(k) for k in list(kw) if k in ("kv_cache_dtype", "tuning", "use_skinny_gemm")}
    ecfg = EngineConfig(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                        max_seqs_in_block_table=64, max_blocks_per_seq=32, max_batch_size=256, max_tokens_in_batch=4096,
                        **engine)
    names = frozenset(n for n in shapes if n in ("qkv", "o") or not kw.get("moe")) if packed else frozenset()
    return T.layer_facts(ecfg, dtype, hidden, 32, 128, shapes, names, _hip.load(), **kw)


def _steps():
    for m, kind, split, (prefill, chunked, verify), lora in itertools.product(
            (1, 2, 8, 16, 17, 32, 33, 256), T.Input, (False, True),
            ((False, False, False), (True, False, False), (True, True, False), (True, False, True)), (False, True)):
        yield T.StepFacts(input=kind, prefill=prefill, m=m, ignore_kvcache=False, positions=True, split=split, verify=verify,
                          chunked=chunked, lora=lora)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_a_moe_layer_ends_its_norm_in_a_tensor_and_returns_one(dtype, monkeypatch):
    def forbidden(name, *args):
        raise AssertionError(f"the route decision launched {name}")
    monkeypatch.setattr(_hip, "call", forbidden)
    seen = set()
    for f in (_facts(dtype, plain_qkv=True, moe=True), _facts(dtype, packed=False, plain_qkv=True, moe=True),
              _facts(dtype, plain_qkv=True, moe=True, kv_cache_dtype="fp8_e4m3"), _facts(dtype, moe=True),
              _facts(dtype, moe=True, use_skinny_gemm=False)):
        assert f.moe is True
        for s in _steps():
            if s.input is not T.Input.TENSOR:
                continue                                    # a MoE layer hands a tensor on: no other input reaches the next
            r = T.decide_route(f, s)
            assert r.down is T.Down.MOE and r.attn_norm is T.AttnNorm.FUSED and not r.merge, (s, r)
            assert r.o_ffn in (T.OFfn.SPLITK_FUSED, T.OFfn.PLAIN), (s, r)
            if s.prefill or s.lora or not f.skinny:
                assert r.o_ffn is T.OFfn.PLAIN, (s, r)
            seen.add(r.o_ffn)
    assert seen == {T.OFfn.SPLITK_FUSED, T.OFfn.PLAIN}


def test_without_the_field_every_route_is_what_it_was():
    dense = dict(qkv=(6144, 4096), o=(4096, 4096), up_gate=(2 * 14336, 4096), down=(4096, 14336))      # Llama-3-8B
    for dtype, fp8, plain in itertools.product((torch.bfloat16, torch.float16), (False, True), (False, True)):
        kw = dict(kv_cache_dtype="fp8_e4m3") if fp8 else {}
        old = _facts(dtype, shapes=dense, hidden=4096, plain_qkv=plain, **kw)
        new = _facts(dtype, shapes=dense, hidden=4096, plain_qkv=plain, moe=False, **kw)
        assert old == new and old.moe is False
        assert T.LayerFacts(*old[:-1]) == old               # the field has a default: positional construction without it
        routes = set()
        for s in _steps():
            try:
                want = T.decide_route(old, s)
            except AssertionError:
                with pytest.raises(AssertionError):
                    T.decide_route(new, s)
                continue
            assert T.decide_route(new, s) == want and want.down is not T.Down.MOE
            routes.add((want.o_ffn, want.down))
        if not (fp8 or plain) and dtype == torch.bfloat16:  # the dense forms are all still reachable
            assert {(T.OFfn.ROWS_NF, T.Down.ROWS), (T.OFfn.TINY, T.Down.SPLITK), (T.OFfn.PLAIN, T.Down.PLAIN)} <= routes


# ---- the routing-forced reference against unhooked HF -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["qwen3_moe", "mixtral"])
def test_forced_with_its_own_choices_the_reference_is_hf(kind, tmp_path):
    hf = R.make_moe_checkpoint(str(tmp_path), kind, torch.bfloat16, 1)
    g = torch.Generator().manual_seed(7)
    rows = [torch.randint(3, 512, (n,), generator=g).tolist() for n in (5, 17, 29)]
    with torch.no_grad():
        plain = [hf(torch.tensor([row])).logits[0].float() for row in rows]
    free = R.forced_logits(hf, rows)
    k = hf.config.num_experts_per_tok
    for (lg, router_logits, ids), want, row in zip(free, plain, rows):
        assert router_logits.shape[:2] == (2, len(row)) and tuple(ids.shape) == (2, len(row), k)
        assert float((lg - want).abs().max()) <= 1e-5        # the hook alone changes nothing
    forced = R.forced_logits(hf, rows, forced=[[ids[layer] for layer in range(2)] for _, _, ids in free])
    for (lg, _, ids), want, (_, _, free_ids) in zip(forced, plain, free):
        assert float((lg - want).abs().max()) <= 1e-5
        assert torch.equal(ids, free_ids)
    # ... and a forced set that is not the free one moves the logits: the hook acts
    other = [[(ids[layer] + 1) % hf.config.get_text_config().to_dict().get("num_experts", 4) for layer in range(2)]
             for _, _, ids in free]
    moved = R.forced_logits(hf, rows, forced=other)
    assert any(float((lg - want).abs().max()) > 1e-4 for (lg, _, _), want in zip(moved, plain))


def test_a_dense_layer_keeps_the_order_of_its_tensors():
    """Callers re-initialise dummy weights by walking vars(layer) with ONE seeded generator (the benchmark does): the order of
    a dense layer's tensor attributes is part of what they compute, so it stays what it was before the MoE attributes."""
    cfg = LlamaModelConfig(dict(LLAMA, hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4,
                                num_key_value_heads=2, vocab_size=512))
    for fuse, want in ((True, ["qkv_proj", "attn_norm", "o_proj", "ffn_norm", "down_proj", "up_gate_proj"]),
                       (False, ["attn_norm", "q_proj", "k_proj", "v_proj", "o_proj", "ffn_norm", "down_proj", "up_gate_proj"])):
        weight = W.load_weights(cfg, torch.float16, "", use_dummy=True, device="cpu", fuse_qkv=fuse)
        got = [name for name, t in vars(weight.layers[0]).items() if isinstance(t, torch.Tensor)]
        assert got == want, got
