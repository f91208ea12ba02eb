"""Host side of the model families beyond Llama (Mistral, Qwen2 / Qwen2.5, dense Qwen3): config parsing and refusals,
both weight loaders on the CPU, and the layer routes of a `plain_qkv` model. No device."""
import itertools
import json
import os

import pytest
import torch

from swiftllm_amd import EngineConfig, LlamaModelConfig, _hip
from swiftllm_amd.worker import weight as W
from swiftllm_amd.worker.layers import transformer_layer as T

from _families_ref import make_hf_checkpoint

# ---- published configs (the fields this project reads, with the published values) -------------------------------------
QWEN3_8B = dict(model_type="qwen3", hidden_act="silu", num_hidden_layers=36, hidden_size=4096, num_attention_heads=32,
                num_key_value_heads=8, head_dim=128, intermediate_size=12288, vocab_size=151936, rope_theta=1000000,
                rms_norm_eps=1e-6, max_position_embeddings=40960, attention_bias=False, tie_word_embeddings=False,
                rope_scaling=None, sliding_window=None, use_sliding_window=False, max_window_layers=36)
QWEN3_4B = dict(QWEN3_8B, hidden_size=2560, intermediate_size=9728, tie_word_embeddings=True)
QWEN25_3B = dict(model_type="qwen2", hidden_act="silu", num_hidden_layers=36, hidden_size=2048, num_attention_heads=16,
                 num_key_value_heads=2, intermediate_size=11008, vocab_size=151936, rope_theta=1000000.0, rms_norm_eps=1e-6,
                 max_position_embeddings=32768, tie_word_embeddings=True, sliding_window=32768, use_sliding_window=False,
                 max_window_layers=70)
MISTRAL_7B = dict(model_type="mistral", hidden_act="silu", num_hidden_layers=32, hidden_size=4096, num_attention_heads=32,
                  num_key_value_heads=8, intermediate_size=14336, vocab_size=32000, rope_theta=10000.0, rms_norm_eps=1e-5,
                  max_position_embeddings=32768, sliding_window=4096, tie_word_embeddings=False)
MISTRAL_NEMO = dict(MISTRAL_7B, num_hidden_layers=40, hidden_size=5120, head_dim=128, vocab_size=131072, rope_theta=1000000.0,
                    max_position_embeddings=131072, sliding_window=None)
LLAMA = dict(model_type="llama", hidden_act="silu", num_hidden_layers=2, hidden_size=128, num_attention_heads=4,
             num_key_value_heads=2, intermediate_size=256, vocab_size=512, rms_norm_eps=1e-5, max_position_embeddings=512)


def test_published_configs_parse():
    c = LlamaModelConfig(QWEN3_8B)
    assert (c.model_type, c.num_layers, c.hidden_size, c.num_q_heads, c.num_kv_heads, c.head_dim, c.q_size) == \
        ("qwen3", 36, 4096, 32, 8, 128, 4096)
    assert (c.ffn_inter_dim, c.vocab_size, c.rope_theta, c.rms_norm_eps, c.max_position_embeddings) == \
        (12288, 151936, 1000000, 1e-6, 40960)
    assert (c.qk_norm, c.qkv_bias, c.tie_word_embeddings, c.rope_scaling, c.sliding_window) == (True, False, False, 1.0, None)
    c = LlamaModelConfig(QWEN3_4B)
    assert (c.hidden_size, c.head_dim, c.q_size, c.ffn_inter_dim, c.qk_norm, c.tie_word_embeddings) == \
        (2560, 128, 4096, 9728, True, True)
    c = LlamaModelConfig(QWEN25_3B)
    assert (c.hidden_size, c.num_q_heads, c.num_kv_heads, c.head_dim, c.q_size, c.ffn_inter_dim) == (2048, 16, 2, 128, 2048, 11008)
    assert (c.qkv_bias, c.qk_norm, c.tie_word_embeddings, c.max_position_embeddings, c.sliding_window) == \
        (True, False, True, 32768, None)        # use_sliding_window false: the window does not apply
    c = LlamaModelConfig(MISTRAL_NEMO)
    assert (c.hidden_size, c.num_q_heads, c.num_kv_heads, c.head_dim, c.q_size) == (5120, 32, 8, 128, 4096)
    assert (c.qkv_bias, c.qk_norm, c.tie_word_embeddings, c.max_position_embeddings) == (False, False, False, 131072)
    assert c.get_kvslot_size(torch.float16) == 2 * 40 * 8 * 128 * 2


def test_a_window_that_applies_caps_the_positions(capsys):
    c = LlamaModelConfig(MISTRAL_7B)
    assert (c.head_dim, c.q_size, c.max_position_embeddings, c.sliding_window) == (128, 4096, 4096, 4096)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "sliding_window 4096" in out
    assert LlamaModelConfig(dict(QWEN25_3B, use_sliding_window=True, sliding_window=1024)).max_position_embeddings == 1024
    assert LlamaModelConfig(dict(QWEN3_8B, use_sliding_window=False, sliding_window=1024)).max_position_embeddings == 40960
    capsys.readouterr()
    assert LlamaModelConfig(dict(MISTRAL_7B, sliding_window=None)).max_position_embeddings == 32768
    assert capsys.readouterr().out == ""


def test_llama_parses_as_before():
    c = LlamaModelConfig(dict(LLAMA, rope_scaling=dict(factor=8.0, rope_type="llama3"), attention_bias=True, head_dim=7))
    assert (c.model_type, c.head_dim, c.q_size, c.qkv_bias, c.qk_norm, c.tie_word_embeddings) == ("llama", 32, 128, False, False, False)
    assert c.rope_scaling == dict(factor=8.0, rope_type="llama3") and c.rope_theta == 10000 and c.sliding_window is None


@pytest.mark.parametrize("base,change,words", [
    (QWEN3_8B, dict(attention_bias=True), "o_proj"),
    (MISTRAL_7B, dict(attention_bias=True), "o_proj"),
    (QWEN3_8B, dict(mlp_bias=True), "mlp_bias"),
    (QWEN25_3B, dict(mlp_bias=True), "mlp_bias"),
    (QWEN3_8B, dict(rope_scaling=dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=32768)), "yarn"),
    (QWEN25_3B, dict(rope_scaling=dict(type="yarn", factor=4.0)), "yarn"),
    (MISTRAL_7B, dict(rope_parameters=dict(rope_type="linear", factor=2.0, rope_theta=1e4)), "linear"),
    (QWEN25_3B, dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4), "ratio of 7"),        # Qwen2.5-7B
    (QWEN25_3B, dict(hidden_size=1536, num_attention_heads=12, num_key_value_heads=2), "ratio of 6"),        # Qwen2.5-1.5B
    (QWEN3_8B, dict(hidden_size=5120, num_attention_heads=40, num_key_value_heads=8), "ratio of 5"),         # Qwen3-14B
    (QWEN3_8B, dict(head_dim=256), "head_dim 256"),
    (MISTRAL_7B, dict(head_dim=96), "head_dim 96"),
    (QWEN3_8B, dict(model_type="qwen3_moe"), "mixture-of-experts"),
])
def test_what_is_not_built_is_refused_with_its_reason(base, change, words):
    with pytest.raises(ValueError, match=words):
        LlamaModelConfig(dict(base, **change))


def test_other_model_types_keep_their_assertion():
    for kind in ("gpt2", "gemma2", "phi3"):
        with pytest.raises(AssertionError):
            LlamaModelConfig(dict(LLAMA, model_type=kind))
    with pytest.raises(AssertionError):
        LlamaModelConfig(dict(QWEN3_8B, hidden_act="gelu"))


# ---- checkpoints written by save_pretrained -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    out = {}
    for name in ("qwen3_d128", "qwen2", "qwen3_d64_tied"):
        path = str(tmp_path_factory.mktemp(name))
        out[name] = (path, make_hf_checkpoint(path, name, torch.bfloat16, seed=3))
    return out


def test_a_config_as_save_pretrained_writes_it_parses(dirs):
    path, _ = dirs["qwen3_d128"]
    raw = json.load(open(os.path.join(path, "config.json"), encoding="utf-8"))
    assert "rope_theta" not in raw and raw["rope_parameters"]["rope_type"] == "default"     # what this test is about
    c = LlamaModelConfig.load_from_model_path(path)
    assert (c.model_type, c.head_dim, c.q_size, c.hidden_size, c.qk_norm, c.rope_theta) == ("qwen3", 128, 512, 256, True, 10000.0)
    assert LlamaModelConfig(dict(raw, rope_parameters=dict(rope_type="default", rope_theta=1e6))).rope_theta == 1e6
    c = LlamaModelConfig.load_from_model_path(dirs["qwen2"][0])
    assert (c.model_type, c.head_dim, c.q_size, c.qkv_bias, c.qk_norm) == ("qwen2", 64, 256, True, False)


def _tensors(weight):
    out = {}
    for owner, prefix in [(weight, "")] + [(lw, f"{i}.") for i, lw in enumerate(weight.layers)]:
        for attr, t in vars(owner).items():
            if isinstance(t, torch.Tensor):
                out[prefix + attr] = t
    return out


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("name", ["qwen3_d128", "qwen2"])
def test_both_loaders_agree_bit_for_bit_on_the_cpu(dirs, name, fuse):
    path, hf = dirs[name]
    cfg = LlamaModelConfig.load_from_model_path(path)
    a = W.load_weights(cfg, torch.bfloat16, path, device="cpu", fuse_qkv=fuse, streaming=True)
    b = W.load_weights(cfg, torch.bfloat16, path, device="cpu", fuse_qkv=fuse, streaming=False)
    ta, tb = _tensors(a), _tensors(b)
    assert set(ta) == set(tb)
    for key in ta:
        assert ta[key].dtype == torch.bfloat16 and torch.equal(ta[key], tb[key]), key
    sd = {k: v.to(torch.bfloat16) for k, v in hf.state_dict().items()}
    qs, kv, h = cfg.q_size, cfg.num_kv_heads * cfg.head_dim, cfg.hidden_size
    for i, lw in enumerate(a.layers):
        pre = f"model.layers.{i}.self_attn."
        q, k, v = (sd[pre + f"{n}_proj.weight"] for n in "qkv")
        assert tuple(q.shape) == (qs, h) and tuple(lw.o_proj.shape) == (h, qs)
        assert torch.equal(lw.o_proj, sd[pre + "o_proj.weight"])
        if fuse:
            assert tuple(lw.qkv_proj.shape) == (qs + 2 * kv, h) and torch.equal(lw.qkv_proj, torch.cat((q, k, v)))
            assert not hasattr(lw, "q_proj")
        else:
            assert lw.qkv_proj is None and torch.equal(lw.q_proj, q) and torch.equal(lw.k_proj, k) and torch.equal(lw.v_proj, v)
        if cfg.qk_norm:
            assert torch.equal(lw.q_norm, sd[pre + "q_norm.weight"]) and torch.equal(lw.k_norm, sd[pre + "k_norm.weight"])
            assert tuple(lw.q_norm.shape) == (cfg.head_dim,) and lw.q_bias is None and lw.qkv_bias is None
        else:
            qb, kb, vb = (sd[pre + f"{n}_proj.bias"] for n in "qkv")
            assert lw.q_norm is None and lw.k_norm is None
            assert torch.equal(lw.q_bias, qb) and torch.equal(lw.k_bias, kb) and torch.equal(lw.v_bias, vb)
            if fuse:        # three slices of one assembled vector
                assert torch.equal(lw.qkv_bias, torch.cat((qb, kb, vb)))
                base = lw.qkv_bias.data_ptr()
                assert [t.data_ptr() - base for t in (lw.q_bias, lw.k_bias, lw.v_bias)] == [0, 2 * qs, 2 * (qs + kv)]
            else:
                assert lw.qkv_bias is None
    assert a.lm_head is not a.wte and torch.equal(a.lm_head, sd["lm_head.weight"])
    # the vectors are not projections: never packed
    proj = {t.data_ptr() for t in a.projection_tensors()}
    for lw in a.layers:
        for t in (lw.q_norm, lw.k_norm, lw.q_bias, lw.k_bias, lw.v_bias, lw.qkv_bias):
            assert t is None or t.data_ptr() not in proj
    assert len(a.projection_tensors()) == 1 + cfg.num_layers * (4 if fuse else 6)


@pytest.mark.parametrize("streaming", [True, False])
def test_a_tied_lm_head_is_the_embedding_object(dirs, streaming):
    path, hf = dirs["qwen3_d64_tied"]
    cfg = LlamaModelConfig.load_from_model_path(path)
    assert cfg.tie_word_embeddings and cfg.q_size == cfg.hidden_size == 256
    w = W.load_weights(cfg, torch.bfloat16, path, device="cpu", fuse_qkv=True, streaming=streaming)
    assert w.lm_head is w.wte and torch.equal(w.wte, hf.state_dict()["model.embed_tokens.weight"].to(torch.bfloat16))


# ---- routes ---------------------------------------------------------------------------------------------------------------
SHAPES = {  # Qwen3-8B and a Qwen3-4B-like layer whose q_size differs from hidden
    "qwen3_8b": (4096, 32, 128, dict(qkv=(6144, 4096), o=(4096, 4096), up_gate=(2 * 12288, 4096), down=(4096, 12288))),
    "qwen3_4b": (2560, 32, 128, dict(qkv=(6144, 2560), o=(2560, 4096), up_gate=(2 * 9728, 2560), down=(2560, 9728))),
}


def _facts(shape, dtype, packed=True, **kw):
    hidden, heads, d, shapes = SHAPES[shape]
    engine = {k: kw.pop(k) for k in list(kw) if k in ("kv_cache_dtype", "tuning", "use_skinny_gemm")}
    ecfg = EngineConfig(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                        max_seqs_in_block_table=64, max_blocks_per_seq=32, max_batch_size=256, max_tokens_in_batch=4096,
                        **engine)
    return T.layer_facts(ecfg, dtype, hidden, heads, d, shapes, frozenset(shapes) if packed else frozenset(), _hip.load(), **kw)


def _steps():
    for m, kind, split, (prefill, chunked, verify), lora in itertools.product(
            (1, 2, 8, 16, 17, 32, 33, 256), T.Input, (False, True),
            ((False, False, False), (True, False, False), (True, True, False), (True, False, True)), (False, True)):
        yield T.StepFacts(input=kind, prefill=prefill, m=m, ignore_kvcache=False, positions=True, split=split, verify=verify,
                          chunked=chunked, lora=lora)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_plain_qkv_layer_takes_none_of_the_fused_qkv_forms(shape, dtype, monkeypatch):
    def forbidden(name, *args):
        raise AssertionError(f"the route decision launched {name}")
    monkeypatch.setattr(_hip, "call", forbidden)
    seen = set()
    for f in (_facts(shape, dtype, plain_qkv=True), _facts(shape, dtype, packed=False, plain_qkv=True),
              _facts(shape, dtype, plain_qkv=True, kv_cache_dtype="fp8_e4m3")):
        assert f.plain_qkv is True
        for s in _steps():
            if s.input in (T.Input.RAW, T.Input.RAW_SSQ):
                with pytest.raises(AssertionError):     # no layer of such a model hands a RawResidual on
                    T.decide_route(f, s)
                continue
            r = T.decide_route(f, s)
            assert r.qkv is T.QKV.ROTARY_THEN_STORE, (s, r)
            assert r.attn_norm is T.AttnNorm.FUSED and not r.merge, (s, r)
            assert r.o_ffn in (T.OFfn.SPLITK_FUSED, T.OFfn.SPLITK_DEFERRED, T.OFfn.PLAIN), (s, r)
            assert r.down in (T.Down.SPLITK, T.Down.PLAIN), (s, r)
            if s.prefill or s.lora:
                assert (r.o_ffn, r.down) == (T.OFfn.PLAIN, T.Down.PLAIN), (s, r)
            seen.add((r.o_ffn, r.down))
        r = T.decide_route(f, T.StepFacts(T.Input.TENSOR, True, 0, True, True, False, False, False, False))
        assert r.qkv is T.QKV.ROTARY_ONLY                # the profile run stores nothing
    assert (T.OFfn.PLAIN, T.Down.PLAIN) in seen and any(d is T.Down.SPLITK for _, d in seen)   # the split-K projections serve it


def test_without_the_field_every_route_is_what_it_was():
    for dtype, fp8 in itertools.product((torch.bfloat16, torch.float16), (False, True)):
        kw = dict(kv_cache_dtype="fp8_e4m3") if fp8 else {}
        old, new = _facts("qwen3_8b", dtype, **kw), _facts("qwen3_8b", dtype, plain_qkv=False, **kw)
        assert old == new and old.plain_qkv is False
        assert T.LayerFacts(*old[:-1]) == old            # the field has a default: positional construction without it
        for s in _steps():
            try:
                want = T.decide_route(old, s)
            except AssertionError:
                with pytest.raises(AssertionError):
                    T.decide_route(new, s)
                continue
            assert T.decide_route(new, s) == want
    # ... and a plain_qkv layer routes exactly as the same layer does with FP8 pools (minus what FP8 alone refuses)
    f16, f8 = _facts("qwen3_8b", torch.bfloat16, plain_qkv=True), _facts("qwen3_8b", torch.bfloat16, kv_cache_dtype="fp8_e4m3")
    for s in _steps():
        if s.input in (T.Input.TENSOR, T.Input.SLABS):
            assert T.decide_route(f16, s) == T.decide_route(f8, s), s
