"""Block-scaled FP8 checkpoints without a device: the refusals of quantization_config, and the ABI rows of
csrc/moe_fp8_block.hip / csrc/moe_fp8_block_wide.hip (header <-> _hip._SPECIAL <-> library, validation observed as
tests/test_moe_fp8_host.py does)."""
import os
import re

import pytest

from swiftllm_amd import _hip
from swiftllm_amd.model_config import LlamaModelConfig
from test_moe_abi import BAD, BASE as TWIN, LAUNCH, OK, ORDERS as TWIN_ORDERS, P, UNSUPPORTED, no_device

ORDERS = {"swl_moe_fp8_block_supported": TWIN_ORDERS["swl_moe_supported"]}
BASE = {}
for _twin, _stack, _scale, _blocks in (("swl_moe_up_gate_silu", "expert_up_gate", "up_gate_bscale", (6, 16)),
                                       ("swl_moe_down", "expert_down", "down_bscale", (16, 6))):    # H 2048, I 768
    _order = list(TWIN_ORDERS[_twin])                       # the twin's arguments, scales and block counts behind the stack
    _at = _order.index(_stack) + 1
    _order[_at:_at] = [_scale, "row_blocks", "k_blocks"]
    _extra = {_scale: P, "row_blocks": _blocks[0], "k_blocks": _blocks[1]}
    ORDERS[_twin + "_fp8_block"], BASE[_twin + "_fp8_block"] = tuple(_order), dict(TWIN[_twin], **_extra)
    _order.insert(_order.index("dtype"), "row_tiles")       # ... and row_tiles before dtype
    ORDERS[_twin + "_fp8_block_wide"], BASE[_twin + "_fp8_block_wide"] = tuple(_order), dict(TWIN[_twin], row_tiles=2, **_extra)

QUANT = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}
MODEL = dict(hidden_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
             rms_norm_eps=1e-6, max_position_embeddings=1024, hidden_act="silu", rope_theta=10000.0)
MOE = dict(MODEL, model_type="mixtral", intermediate_size=128, num_local_experts=4, num_experts_per_tok=2)


def run(name, **change):
    args = dict(BASE[name], **change)
    return getattr(_hip.load(), name)(*[args[k] for k in ORDERS[name]])


def test_entries_are_in_the_header_and_special_only_and_the_abi_version_stays():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swiftllm_hip.h"),
                  encoding="utf-8").read()
    assert "csrc/moe_fp8_block.h" in header and re.search(r"#define\s+SWL_ABI_VERSION\s+2\b", header)
    assert _hip.ABI_VERSION == 2 and _hip.load().swl_abi_version() == 2
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, order in ORDERS.items():
        argtypes, restype = _hip._SPECIAL[name]
        assert name not in _hip.SIGNATURES and len(order) == len(argtypes) and restype is _hip._I32, name
        params = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).split(",")
        assert tuple(p.split()[-1].lstrip("*") for p in params) == order, name
        for p, ctype in zip(params, argtypes):
            assert ctype is (_hip._P if "*" in p or "swl_stream_t" in p else _hip._I64 if "int64_t" in p else _hip._I32), (name, p)


def test_supported_shapes_and_empty_batches_are_host_arithmetic():
    ok = _hip.load().swl_moe_fp8_block_supported
    assert ok(2048, 768, 128, 8, _hip.SWL_BF16) == 1 and ok(4096, 14336, 8, 2, _hip.SWL_F16) == 1 and ok(576, 192, 8, 2, 0) == 1
    assert ok(256, 96, 8, 2, 0) == 0 and ok(288, 128, 8, 2, 0) == 0 and ok(256, 128, 257, 2, 0) == 0 and ok(256, 128, 8, 2, 2) == 0
    for name in BASE:                                       # an empty batch is OK and launches nothing
        nulls = {k: None for k, v in BASE[name].items() if v == P}
        assert run(name, num_tokens=0, **nulls) == OK and run(name, max_tiles=0) == OK


@no_device
@pytest.mark.parametrize("name", list(BASE))
def test_validation(name):
    assert run(name) == LAUNCH and run(name, dtype=_hip.SWL_F16) == LAUNCH
    for field, v in BASE[name].items():                     # null operands, the scales among them
        if v == P:
            assert run(name, **{field: None}) == BAD, field
    for field in ("x", "expert_up_gate") if "x" in BASE[name] else ("act", "expert_down"):
        assert run(name, **{field: P + 8}) == BAD, field
    for change, want in ((dict(num_tokens=-1), BAD), (dict(top_k=0), BAD), (dict(dtype=2), BAD), (dict(max_tiles=-1), BAD),
                         (dict(num_experts=257), UNSUPPORTED), (dict(num_tokens=513), UNSUPPORTED),
                         (dict(inter=800), UNSUPPORTED),    # 800 % 32 == 0, % 64 != 0
                         (dict(row_blocks=BASE[name]["row_blocks"] + 1), BAD), (dict(k_blocks=BASE[name]["k_blocks"] - 1), BAD),
                         (dict(inter=832, **{"row_blocks" if "x" in BASE[name] else "k_blocks": 7}), LAUNCH)):  # a partial block
        assert run(name, **change) == want, change
    if name.endswith("_wide"):                              # 2 tiles only: four do not fit a wave's registers
        assert (run(name, row_tiles=0), run(name, row_tiles=3), run(name, row_tiles=4)) == (BAD, UNSUPPORTED, UNSUPPORTED)


@pytest.mark.parametrize("config, reason", [
    (dict(MOE, quantization_config=dict(QUANT, quant_method="compressed-tensors")), "quant_method 'compressed-tensors'"),
    (dict(MOE, quantization_config=dict(QUANT, fmt="e5m2")), "fmt 'e5m2'"),
    (dict(MOE, quantization_config=dict(QUANT, weight_block_size=[64, 64])), r"weight_block_size \[64, 64\]"),
    (dict(MOE, quantization_config=dict(QUANT, weight_block_size=None)), "weight_block_size None"),
    (dict(MOE, quantization_config=dict(QUANT, activation_scheme="static")), "activation_scheme 'static'"),
    (dict(MODEL, model_type="llama", intermediate_size=512, quantization_config=QUANT), "quantised dense model"),
    (dict(MOE, intermediate_size=96, quantization_config=QUANT), "multiples of 64"),
], ids=["method", "fmt", "block_size", "per_tensor", "static", "dense", "geometry"])
def test_refusals_name_their_reason(config, reason):
    with pytest.raises(ValueError, match=reason):
        LlamaModelConfig(config)
    assert not LlamaModelConfig({k: v for k, v in config.items() if k != "quantization_config"}).fp8_block


def test_a_block_scaled_config_is_taken():
    assert LlamaModelConfig(dict(MOE, quantization_config=QUANT)).fp8_block
