"""FP8 expert weights without a device: the option and its refusals, the CLI flags, and the ABI rows of csrc/moe_fp8.hip /
csrc/moe_fp8_wide.hip (header <-> _hip._SPECIAL <-> library, validation observed as tests/test_moe_wide_abi.py does)."""
import argparse
import dataclasses
import json
import os
import re

import pytest

from swiftllm_amd import EngineConfig, _hip
from test_moe_abi import BAD, BASE as TWIN, LAUNCH, OK, ORDERS as TWIN_ORDERS, P, UNSUPPORTED, no_device

ORDERS = {"swl_moe_fp8_supported": TWIN_ORDERS["swl_moe_supported"],
          "swl_moe_quantise_rows": ("codes", "rows", "inv", "num_rows", "row_len", "dtype", "stream")}
BASE = {"swl_moe_quantise_rows": dict(codes=P, rows=P, inv=P, num_rows=768, row_len=2048, dtype=_hip.SWL_BF16, stream=None)}
for _twin, _stack, _scale in (("swl_moe_up_gate_silu", "expert_up_gate", "up_gate_scale"),
                              ("swl_moe_down", "expert_down", "down_scale")):
    _order = list(TWIN_ORDERS[_twin])                       # the twin's arguments, the scales behind the stack ...
    _order.insert(_order.index(_stack) + 1, _scale)
    ORDERS[_twin + "_fp8"], BASE[_twin + "_fp8"] = tuple(_order), dict(TWIN[_twin], **{_scale: P})
    _order.insert(_order.index("dtype"), "row_tiles")       # ... and row_tiles before dtype
    ORDERS[_twin + "_fp8_wide"], BASE[_twin + "_fp8_wide"] = tuple(_order), dict(TWIN[_twin], row_tiles=4, **{_scale: P})

def config(path="/m", **kw):
    return EngineConfig(model_path=path, use_dummy=False, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=8,
                        max_seqs_in_block_table=16, max_blocks_per_seq=16, max_batch_size=8, max_tokens_in_batch=256, **kw)


def run(name, **change):
    args = dict(BASE[name], **change)
    return getattr(_hip.load(), name)(*[args[k] for k in ORDERS[name]])


def test_entries_are_registered_with_their_types_and_match_the_header():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swiftllm_hip.h"),
                  encoding="utf-8").read()
    assert "csrc/moe_fp8.h" in header                       # the storage contract is cited
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, order in ORDERS.items():
        argtypes, restype = _hip._SPECIAL[name]
        assert len(order) == len(argtypes) and restype is _hip._I32 and hasattr(_hip.load(), name), name
        params = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).split(",")
        assert tuple(p.split()[-1].lstrip("*") for p in params) == order, name
        for p, ctype in zip(params, argtypes):
            want = (_hip._P if "*" in p or "swl_stream_t" in p else _hip._I64 if "int64_t" in p else _hip._I32)
            assert ctype is want, (name, p)


def test_supported_shapes_and_empty_batches_are_host_arithmetic():
    ok = _hip.load().swl_moe_fp8_supported
    assert ok(2048, 768, 128, 8, _hip.SWL_BF16) == 1 and ok(4096, 14336, 8, 2, _hip.SWL_F16) == 1 and ok(256, 128, 8, 2, 0) == 1
    assert ok(256, 96, 8, 2, 0) == 0 and ok(288, 128, 8, 2, 0) == 0       # a k step is 64 codes: both % 64
    assert ok(256, 128, 257, 2, 0) == 0 and ok(256, 128, 8, 17, 0) == 0 and ok(256, 128, 2, 3, 0) == 0 and ok(256, 128, 8, 2, 2) == 0
    for name in BASE:                                       # an empty batch is OK and launches nothing
        nulls = {k: None for k, v in BASE[name].items() if v == P}
        empty = dict(num_rows=0) if name == "swl_moe_quantise_rows" else dict(num_tokens=0)
        assert run(name, **empty, **nulls) == OK and (empty == dict(num_rows=0) or run(name, max_tiles=0) == OK)


@no_device
@pytest.mark.parametrize("name", list(BASE))
def test_validation(name):
    assert run(name) == LAUNCH and run(name, dtype=_hip.SWL_F16) == LAUNCH
    for field, v in BASE[name].items():                     # null operands
        if v == P:
            assert run(name, **{field: None}) == BAD, field
    if name == "swl_moe_quantise_rows":
        assert run(name, row_len=2056) == UNSUPPORTED and run(name, row_len=0) == BAD and run(name, num_rows=-1) == BAD
        assert run(name, codes=P + 8) == BAD and run(name, rows=P + 8) == BAD and run(name, dtype=2) == BAD
        return
    for field in ("x", "expert_up_gate") if "x" in BASE[name] else ("act", "expert_down"):
        assert run(name, **{field: P + 8}) == BAD, field
    for change, want in ((dict(num_tokens=-1), BAD), (dict(top_k=0), BAD), (dict(top_k=3, num_experts=2), BAD),
                         (dict(dtype=2), BAD), (dict(max_tiles=-1), BAD), (dict(num_experts=257), UNSUPPORTED),
                         (dict(num_tokens=513), UNSUPPORTED), (dict(inter=800), UNSUPPORTED)):     # 800 % 32 == 0, % 64 != 0
        assert run(name, **change) == want, change
    assert not name.endswith("_wide") or (run(name, row_tiles=2), run(name, row_tiles=0), run(name, row_tiles=3)) == (LAUNCH, BAD, UNSUPPORTED)


def test_the_option_is_validated_and_reaches_engine_config_from_every_cli():
    assert config().moe_weight_dtype == "auto"
    with pytest.raises(ValueError, match="moe_weight_dtype must be one of"):
        config(moe_weight_dtype="int4")
    ap = argparse.ArgumentParser()
    EngineConfig.add_cli_args(ap)                           # api_server builds EngineConfig from the parsed fields
    a = ap.parse_args(["--model-path", "/m", "--moe-weight-dtype", "fp8_e4m3"])
    assert ap.parse_args(["--model-path", "/m"]).moe_weight_dtype == "auto"
    with pytest.raises(SystemExit):
        ap.parse_args(["--model-path", "/m", "--moe-weight-dtype", "int4"])
    fields = {f.name for f in dataclasses.fields(EngineConfig)}
    assert EngineConfig(**{k: v for k, v in vars(a).items() if k in fields}).moe_weight_dtype == "fp8_e4m3"
    from swiftllm_amd.server.router import moe_passthrough
    assert moe_passthrough("fp8_e4m3") == ["--moe-weight-dtype", "fp8_e4m3"] and moe_passthrough(None) == []


def test_refusals_at_load_name_their_reason(tmp_path):
    from swiftllm_amd import LlamaModel
    base = dict(hidden_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
                rms_norm_eps=1e-6, max_position_embeddings=1024, hidden_act="silu", rope_theta=10000.0)
    cases = {"dense": (dict(base, model_type="llama", intermediate_size=512), "no mixture-of-experts layers"),
             "narrow": (dict(base, model_type="mixtral", intermediate_size=96, num_local_experts=4, num_experts_per_tok=2),
                        "multiples of 64")}
    for name, (cfg, reason) in cases.items():
        os.makedirs(tmp_path / name)
        with open(tmp_path / name / "config.json", "w") as f:
            json.dump(cfg, f)
        LlamaModel(config(str(tmp_path / name), dtype="bfloat16"))                         # "auto" takes both
        with pytest.raises(ValueError, match=reason):
            LlamaModel(config(str(tmp_path / name), dtype="bfloat16", moe_weight_dtype="fp8_e4m3"))
