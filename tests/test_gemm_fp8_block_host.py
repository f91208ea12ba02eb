"""Dense block-scaled FP8 projections without a device: the ABI rows of csrc/gemm_fp8_block.hip (header <-> _hip._SPECIAL <->
library, validation observed as tests/test_moe_fp8_block_host.py does), the host arithmetic, and the config's opt-in."""
import re

import pytest

from swiftllm_amd import _hip
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.model_config import LlamaModelConfig
from test_abi import HEADER
from test_moe_abi import BAD, LAUNCH, OK, P, UNSUPPORTED, no_device
from test_moe_fp8_block_host import MODEL, MOE, QUANT

ORDERS = {
    "swl_gemm_fp8_block_supported": ("n", "k", "dtype"),
    "swl_gemm_fp8_block_choose_splits": ("n", "k"),
    "swl_gemm_fp8_block": ("y", "x", "codes", "bscale", "workspace", "workspace_bytes", "num_tokens", "seg0", "seg1", "seg2", "k",
                           "scale_rows", "k_blocks", "x_row_stride", "k_splits", "dtype", "stream"),
    "swl_gemm_fp8_block_silu_gate": ("act", "x", "codes", "bscale", "workspace", "workspace_bytes", "num_tokens", "inter", "k",
                                     "scale_rows", "k_blocks", "x_row_stride", "k_splits", "dtype", "stream"),
    "swl_fp8_block_dequant": ("out", "codes", "bscale", "seg0", "seg1", "seg2", "k", "scale_rows", "k_blocks", "dtype", "stream"),
}
# qkv of a GQA model: segments 192 / 64 / 64 (2 + 1 + 1 scale rows), K = 576 (5 k blocks); [up ; gate] of inter 192
BASE = {
    "swl_gemm_fp8_block": dict(y=P, x=P, codes=P, bscale=P, workspace=P, workspace_bytes=1 << 20, num_tokens=17, seg0=192, seg1=64,
                               seg2=64, k=576, scale_rows=4, k_blocks=5, x_row_stride=576, k_splits=0, dtype=_hip.SWL_BF16,
                               stream=None),
    "swl_gemm_fp8_block_silu_gate": dict(act=P, x=P, codes=P, bscale=P, workspace=P, workspace_bytes=1 << 20, num_tokens=17,
                                         inter=192, k=576, scale_rows=4, k_blocks=5, x_row_stride=576, k_splits=0,
                                         dtype=_hip.SWL_BF16, stream=None),
    "swl_fp8_block_dequant": dict(out=P, codes=P, bscale=P, seg0=192, seg1=64, seg2=64, k=576, scale_rows=4, k_blocks=5,
                                  dtype=_hip.SWL_BF16, stream=None),
}
DENSE = dict(MODEL, model_type="llama", intermediate_size=512, quantization_config=QUANT)
ENGINE = dict(model_path="x", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=0, max_seqs_in_block_table=8,
              max_blocks_per_seq=8, max_batch_size=8, max_tokens_in_batch=128)


def run(name, **change):
    args = dict(BASE[name], **change)
    return getattr(_hip.load(), name)(*[args[k] for k in ORDERS[name]])


def test_entries_are_in_the_header_and_special_only_and_the_abi_version_stays():
    header = open(HEADER, encoding="utf-8").read()
    assert "csrc/gemm_fp8_block.h" in header and re.search(r"#define\s+SWL_ABI_VERSION\s+2\b", header)
    assert _hip.ABI_VERSION == 2 and _hip.load().swl_abi_version() == 2
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, order in ORDERS.items():
        argtypes, restype = _hip._SPECIAL[name]
        assert name not in _hip.SIGNATURES and len(order) == len(argtypes) and restype is _hip._I32, name
        params = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).split(",")
        assert tuple(p.split()[-1].lstrip("*") for p in params) == order, name
        for p, ctype in zip(params, argtypes):
            assert ctype is (_hip._P if "*" in p or "swl_stream_t" in p else _hip._I64 if "int64_t" in p else _hip._I32), (name, p)


def test_supported_shapes_splits_and_empty_batches_are_host_arithmetic():
    lib = _hip.load()
    ok, splits = lib.swl_gemm_fp8_block_supported, lib.swl_gemm_fp8_block_choose_splits
    assert ok(6144, 4096, _hip.SWL_BF16) == 1 and ok(320, 576, _hip.SWL_F16) == 1 and ok(16, 64, 0) == 1
    assert ok(6152, 4096, 0) == 0 and ok(4096, 4128, 0) == 0 and ok(4096, 4096, 2) == 0 and ok(0, 64, 0) == 0
    # a function of (N, K) alone: a power of two, <= 8, <= the k blocks, 1 where the tiles fill the card already
    assert splits(28672, 4096) == 1 and splits(14336, 4096) == 2 and splits(4096, 4096) == 4 and splits(4096, 14336) == 4 and splits(6144, 4096) == 4
    assert splits(1024, 4096) == 8 and splits(192, 2112) == 8 and splits(256, 128) == 1 and splits(2112, 192) == 1
    assert splits(100, 4096) == 0 and splits(4096, 100) == 0
    for name in BASE:                                       # an empty batch is OK and launches nothing
        if "num_tokens" in BASE[name]:
            assert run(name, num_tokens=0, **{k: None for k, v in BASE[name].items() if v == P}) == OK


@no_device
@pytest.mark.parametrize("name", list(BASE))
def test_validation(name):
    gemm = "num_tokens" in BASE[name]
    assert run(name) == LAUNCH and run(name, dtype=_hip.SWL_F16) == LAUNCH
    for field, v in BASE[name].items():                     # null operands, the scales among them
        if v == P and field != "workspace":
            assert run(name, **{field: None}) == BAD, field
    for field in ("x", "codes") if gemm else ("out", "codes"):
        assert run(name, **{field: P + 8}) == BAD, field
    seg = "inter" if "inter" in BASE[name] else "seg1"
    for change, want in ((dict(dtype=2), BAD), (dict(k=608, k_blocks=5), UNSUPPORTED),      # 608 % 32 == 0, % 64 != 0
                         ({seg: 72}, UNSUPPORTED),          # a segment that is no multiple of 16
                         (dict(scale_rows=5), BAD), (dict(k_blocks=4), BAD),
                         (dict(k=640, **({"x_row_stride": 640} if gemm else {})), LAUNCH)):     # a partial last k block
        assert run(name, **change) == want, change
    if gemm:
        for change, want in ((dict(num_tokens=-1), BAD), (dict(num_tokens=65), UNSUPPORTED), (dict(num_tokens=64), LAUNCH),
                             (dict(x_row_stride=568), BAD), (dict(k_splits=3), BAD), (dict(k_splits=8), BAD),   # 8 > 5 k blocks
                             (dict(k_splits=4), LAUNCH), (dict(k_splits=4, workspace=None), BAD),
                             (dict(k_splits=4, workspace_bytes=4 * 17 * 320 * 4 - 1), BAD),
                             (dict(k_splits=1, workspace=None, workspace_bytes=0), LAUNCH)):
            assert run(name, **change) == want, change
    else:
        assert run(name, seg1=0) == UNSUPPORTED             # an empty segment before a used one


def test_a_dense_block_scaled_config_is_taken_with_the_option_only():
    with pytest.raises(ValueError, match="quantised dense model.*dense_weight_dtype"):
        LlamaModelConfig(DENSE)
    cfg = LlamaModelConfig(DENSE, dense_fp8=True)
    assert cfg.fp8_block and cfg.dense_fp8 and not LlamaModelConfig(dict(MOE, quantization_config=QUANT)).dense_fp8
    assert EngineConfig(**ENGINE).dense_weight_dtype == "auto"


@pytest.mark.parametrize("config, reason", [
    (dict(DENSE, intermediate_size=480), "multiples of 64"),
    (dict(DENSE, hidden_size=288, num_attention_heads=9, num_key_value_heads=9), "multiples of 64"),
    (dict(DENSE, model_type="mistral", head_dim=32, num_attention_heads=3, num_key_value_heads=3), "q_size 96"),
    (dict(DENSE, hidden_size=64, num_attention_heads=8, num_key_value_heads=1), "multiples of 16"),    # q_size 64, kv 8
    (dict(DENSE, quantization_config=dict(QUANT, fmt="e5m2")), "fmt 'e5m2'"),
    ({k: v for k, v in DENSE.items() if k != "quantization_config"}, "no quantization_config"),
    (dict(MOE, quantization_config=QUANT), "mixture-of-experts"),
], ids=["inter", "hidden", "q_size", "kv_size", "fmt", "not_quantised", "moe"])
def test_new_refusals_name_their_reason(config, reason):
    with pytest.raises(ValueError, match=reason):
        LlamaModelConfig(config, dense_fp8=True)


@pytest.mark.parametrize("kw, reason", [(dict(tuning={"decode_engine": True}), "decode_engine"), (dict(max_loras=1), "max_loras"),
                                        (dict(dense_weight_dtype="fp8"), "must be one of")])
def test_the_engine_option_refuses_what_it_does_not_serve(kw, reason):
    with pytest.raises(ValueError, match=reason):
        EngineConfig(**{**ENGINE, "dense_weight_dtype": "fp8_block", **kw})
