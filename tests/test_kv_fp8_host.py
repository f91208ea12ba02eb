"""FP8 (e4m3fn) KV cache, the parts that need no GPU: the engine option, the sizing arithmetic, the C-ABI surface and
its argument validation, the torch reference of the storage contract (tests/_fp8_ref.py), the server flag."""
import argparse
import ctypes
import os

import pytest
import torch

import _fp8_ref as R
from swiftllm_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("swl_store_kv_prefill_at_fp8", "swl_store_kv_decode_fp8", "swl_paged_attn_phase1_fp8",
       "swl_paged_attn_decode_fp8", "swl_prefill_attn_paged_fp8")


def _cfg(**kw):
    from swiftllm_amd import EngineConfig
    base = dict(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                max_seqs_in_block_table=16, max_blocks_per_seq=32, max_batch_size=8, max_tokens_in_batch=256)
    base.update(kw)
    return EngineConfig(**base)


def test_engine_config_accepts_auto_and_fp8_and_nothing_else():
    assert _cfg().kv_cache_dtype == "auto"
    assert _cfg(kv_cache_dtype="auto").kv_cache_dtype == "auto"
    assert _cfg(kv_cache_dtype="fp8_e4m3").kv_cache_dtype == "fp8_e4m3"
    for bad in ("fp8", "fp8_e5m2", "float16", "", None, 8):
        with pytest.raises(ValueError):
            _cfg(kv_cache_dtype=bad)
    with pytest.raises(ValueError, match="decode_engine"):
        _cfg(kv_cache_dtype="fp8_e4m3", tuning=dict(decode_engine=True))
    assert _cfg(kv_cache_dtype="auto", tuning=dict(decode_engine=True)).decode_engine is True


def test_kvslot_size_and_block_count_use_the_pool_element_size():
    from swiftllm_amd import LlamaModelConfig
    from swiftllm_amd.worker.model import LlamaModel
    cfg = LlamaModelConfig(dict(model_type="llama", hidden_act="silu", num_hidden_layers=32, num_attention_heads=32,
                                num_key_value_heads=8, hidden_size=4096, vocab_size=128256,
                                max_position_embeddings=8192, intermediate_size=14336, rms_norm_eps=1e-5))
    s16, s8 = cfg.get_kvslot_size(torch.bfloat16), cfg.get_kvslot_size(torch.float8_e4m3fn)
    assert s16 == 2 * 32 * 8 * 128 * 2 and s8 * 2 == s16 and cfg.get_kvslot_size() == s16
    for budget in (0.0, 1.0, 16 * s16 - 1, 16 * s16, 250e9, 250e9 + 12345.0):
        n16_half = LlamaModel.blocks_that_fit(budget, (16 * s16) // 2)
        assert LlamaModel.blocks_that_fit(budget, 16 * s8) == n16_half
        assert 2 * LlamaModel.blocks_that_fit(budget, 16 * s16) <= n16_half <= 2 * LlamaModel.blocks_that_fit(budget, 16 * s16) + 1
    assert LlamaModel.blocks_that_fit(-5.0, 16 * s8) == 0


def test_new_symbols_are_in_the_header_the_ctypes_table_and_the_library():
    header = open(os.path.join(ROOT, "include", "swiftllm_hip.h"), encoding="utf-8").read()
    lib = _hip.load()
    for name in NEW:
        assert name + "(" in header and name in _hip.SIGNATURES and hasattr(lib, name)
    assert "#define SWL_ABI_VERSION 2" in header and _hip.ABI_VERSION == 2 and lib.swl_abi_version() == 2


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 32)
    return buf, ctypes.addressof(buf) // 16 * 16 + 16


def test_fp8_entry_points_validate_before_any_launch():
    lib = _hip.load()
    keep, p = _aligned()

    def store_at(kc=p, k=p, inv=p, n=1, mx=4, layer=0, D=128, dt=_hip.SWL_F16):
        return lib.swl_store_kv_prefill_at_fp8(kc, p, k, p, inv, p, p, p, p, None, n, mx, layer, 2, 8, 16, D, 8, 1024,
                                               1024, dt, None)

    def store_dec(kc=p, inv=p, n=1, D=128, dt=_hip.SWL_BF16):
        return lib.swl_store_kv_decode_fp8(kc, p, p, p, inv, p, p, p, n, 0, 2, 8, 16, D, 8, 1024, 1024, dt, None)

    def phase1(q=p, sc=p, n=1, D=128, dt=_hip.SWL_F16, nsb=1, H=32):
        return lib.swl_paged_attn_phase1_fp8(p, q, p, p, sc, p, p, p, None, None, 0.088, n, H, 8, D, 2, 16, 0, 8, 64,
                                             nsb, 4096, 4096, dt, None)

    def decode(o=p, sc=p, n=1, D=128, dt=_hip.SWL_F16, nsb=1, scratch=None):
        return lib.swl_paged_attn_decode_fp8(o, p, p, p, sc, p, p, p, scratch, 0.088, n, 32, 8, D, 2, 16, 0, 8, 64, nsb,
                                             4096, 4096, dt, None)

    def prefill(o=p, sc=p, n=1, D=128, dt=_hip.SWL_F16, mbps=8, total=64):
        return lib.swl_prefill_attn_paged_fp8(o, p, p, p, sc, p, p, p, p, n, 64, total, 32, 8, D, 2, 16, 0, mbps,
                                              0.088, 4096, 4096, dt, None)

    # empty batches are legal and launch nothing
    assert store_at(n=0) == 0 and store_at(mx=0) == 0 and store_dec(n=0) == 0
    assert phase1(n=0) == 0 and decode(n=0) == 0 and decode(nsb=0) == 0 and prefill(n=0) == 0
    # null pointers, a bad head dim, a bad dtype code: SWL_ERR_BAD_ARG, no launch (there is no GPU here)
    assert store_at(kc=None) == -1 and store_at(inv=None) == -1 and store_at(k=p + 2) == -1 and store_at(n=-1) == -1
    assert store_at(D=24) == -1 and store_at(dt=7) == -1 and store_at(layer=2) == -1
    assert store_dec(kc=None) == -1 and store_dec(inv=None) == -1 and store_dec(D=24) == -1 and store_dec(dt=7) == -1
    assert phase1(q=None) == -1 and phase1(sc=None) == -1 and phase1(D=48) == -1 and phase1(D=256) == -1
    assert phase1(dt=7) == -1 and phase1(H=30) == -1 and phase1(nsb=2) == -1      # split without partial buffers
    assert decode(o=None) == -1 and decode(sc=None) == -1 and decode(D=48) == -1 and decode(dt=7) == -1
    assert decode(nsb=2, scratch=None) == -1
    assert prefill(o=None) == -1 and prefill(sc=None) == -1 and prefill(D=48) == -1 and prefill(dt=7) == -1
    assert prefill(total=200, mbps=8) == -1         # a table row cannot hold the longest sequence
    del keep


def _all_codes():
    return torch.arange(256, dtype=torch.uint8).view(R.FP8)


def test_every_finite_code_is_exact_in_float16_and_bfloat16():
    x8 = _all_codes()
    f32 = x8.to(torch.float32)
    finite = torch.isfinite(f32)
    assert int(finite.sum()) == 254 and not finite[0x7f] and not finite[0xff]
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(x8.to(dt)[finite].to(torch.float32), f32[finite])
        assert torch.equal(R.dequantise(x8, dt)[finite].double(), f32[finite].double())
    assert f32[finite].abs().max().item() == 448.0
    assert f32[1].item() == 2.0 ** -9 and f32[8].item() == 2.0 ** -6      # smallest subnormal, smallest normal
    # and the round trip of every finite code is the identity
    assert torch.equal(R.codes(R.quantise(f32[finite], 1.0)), R.codes(x8)[finite])


def test_reference_saturates_rounds_to_nearest_even_and_keeps_subnormals():
    q = lambda *v, inv=1.0: R.quantise(torch.tensor(v, dtype=torch.float32), inv).to(torch.float32).tolist()  # noqa: E731
    assert q(448.0, 449.0, 1e6, float("inf"), -500.0, -float("inf")) == [448.0, 448.0, 448.0, 448.0, -448.0, -448.0]
    assert q(464.0, 480.0) == [448.0, 448.0]                    # beyond the last rounding boundary: clamped, not NaN
    assert q(432.0, 400.0, 21.0, 23.0, 1.0625, 1.1875) == [448.0, 384.0, 20.0, 24.0, 1.0, 1.25]     # ties to even
    assert q(17.0, 19.0) == [16.0, 20.0]
    sub = 2.0 ** -9
    assert q(sub, 0.5 * sub, 1.5 * sub, 2.5 * sub, 0.49 * sub, 7.5 * sub) == [sub, 0.0, 2 * sub, 2 * sub, 0.0, 8 * sub]
    assert R.codes(R.quantise(torch.tensor([-0.0, -1e-9]), 1.0)).tolist() == [0x80, 0x80]
    # the scale goes in as ONE fp32 multiplication by fp32(1 / scale)
    s = torch.tensor(0.3, dtype=torch.float32)
    x = torch.tensor([1.0, -37.5, 1000.0], dtype=torch.float16)
    want = (x.float() * (1.0 / s)).clamp(-448, 448).to(R.FP8)
    assert torch.equal(R.codes(R.quantise(x, R.inv_scale(s))), R.codes(want))
    assert R.stored(x, s).tolist() == (want.to(torch.float32).double() * s.double()).tolist()
    # fp16 / bf16 inputs: the product is taken in fp32
    for dt in (torch.float16, torch.bfloat16):
        x = (torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 50).to(dt)
        assert torch.equal(R.codes(R.quantise(x, 0.7)), R.codes((x.float() * torch.tensor(0.7)).clamp(-448, 448).to(R.FP8)))
        assert torch.equal(R.fake_quant(x), R.quantise(x, 1.0).to(dt))


def test_server_cli_parses_the_flag():
    from swiftllm_amd import EngineConfig
    ap = argparse.ArgumentParser()
    EngineConfig.add_cli_args(ap)
    a = ap.parse_args(["--model-path", "/m", "--kv-cache-dtype", "fp8_e4m3"])
    assert a.kv_cache_dtype == "fp8_e4m3"
    assert ap.parse_args(["--model-path", "/m"]).kv_cache_dtype == "auto"
    with pytest.raises(SystemExit):
        ap.parse_args(["--model-path", "/m", "--kv-cache-dtype", "int4"])
    import dataclasses
    fields = {f.name for f in dataclasses.fields(EngineConfig)}
    assert "kv_cache_dtype" in fields       # api_server builds EngineConfig from the parsed fields
    cfg = EngineConfig(**{k: v for k, v in vars(a).items() if k in fields})
    assert cfg.kv_cache_dtype == "fp8_e4m3"
