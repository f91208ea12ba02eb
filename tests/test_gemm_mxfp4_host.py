"""MXFP4 dense projections without a device: the engine option and its refusals, the host arithmetic of csrc/gemm_mxfp4.hip and
its entries' argument checks (as tests/test_gemm_fp8_row_host.py: a call that passes every check fails at the launch)."""
import argparse

import pytest

from swiftllm_amd import _hip
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.model_config import LlamaModelConfig
from swiftllm_amd.worker.kernels import linear_mxfp4 as L
from swiftllm_amd.worker.weight import dense_fp8_row_refusal
from test_gemm_fp8_block_host import DENSE, ENGINE
from test_moe_abi import BAD, LAUNCH, OK, P, UNSUPPORTED, no_device
from test_moe_fp8_block_host import MOE

GEMM = ("x", "codes", "scales", "workspace", "workspace_bytes", "num_tokens", "ROWS", "k", "x_row_stride", "k_splits", "dtype", "stream")
ORDERS = {
    "swl_gemm_mxfp4_quantise_pack": ("codes", "scales", "w", "n", "k", "dtype", "stream"),
    "swl_gemm_mxfp4": ("y",) + tuple(f.replace("ROWS", "n") for f in GEMM),
    "swl_gemm_mxfp4_silu_gate": ("act",) + tuple(f.replace("ROWS", "inter") for f in GEMM),
    "swl_mxfp4_dequant": ("out", "codes", "scales", "n", "k", "dtype", "stream"),
}
VALUES = dict(n=80, inter=80, k=1152, dtype=_hip.SWL_BF16, stream=None, workspace_bytes=1 << 20, num_tokens=17, x_row_stride=1152,
              k_splits=0)
BASE = {name: {f: VALUES.get(f, P) for f in order} for name, order in ORDERS.items()}
PLAIN = {k: v for k, v in DENSE.items() if k != "quantization_config"}      # a 16-bit Llama: hidden 256, inter 512
MX = dict(ENGINE, dense_weight_dtype="mxfp4", dtype="bfloat16")


def run(name, **change):
    args = dict(BASE[name], **change)
    return getattr(_hip.load(), name)(*[args[k] for k in ORDERS[name]])


def test_the_option_takes_the_new_value():
    assert EngineConfig(**MX).dense_weight_dtype == "mxfp4" and "mxfp4" in EngineConfig.DENSE_WEIGHT_DTYPES
    ap = argparse.ArgumentParser()
    EngineConfig.add_cli_args(ap)
    assert ap.parse_args(["--model-path", "m", "--dense-weight-dtype", "mxfp4"]).dense_weight_dtype == "mxfp4"
    assert dense_fp8_row_refusal(LlamaModelConfig(PLAIN), mxfp4=True) == ""
    for name, order in ORDERS.items():
        assert name not in _hip.SIGNATURES and len(_hip._SPECIAL[name][0]) == len(order), name


@pytest.mark.parametrize("kw, reason", [(dict(dtype="float16"), "float16's range"), (dict(tuning={"decode_engine": True}), "decode_engine"),
                                        (dict(max_loras=1), "max_loras"), (dict(dense_fp8_wide=True), "needs dense_weight_dtype='fp8_block'")])
def test_the_engine_option_refuses_what_it_does_not_serve(kw, reason):
    with pytest.raises(ValueError, match=reason):
        EngineConfig(**{**MX, **kw})


@pytest.mark.parametrize("config, reason", [
    (MOE, "moe_weight_dtype"),
    (DENSE, "quantization_config"),
    (dict(PLAIN, intermediate_size=480), "multiples of 16 rows and of 128 columns"),
    (dict(PLAIN, hidden_size=192, num_attention_heads=6, num_key_value_heads=2), "is 192 x 192"),    # 192 % 64 == 0, % 128 != 0
], ids=["moe", "quantised", "inter", "hidden"])
def test_the_model_refusals_name_their_reason(config, reason):
    assert reason in dense_fp8_row_refusal(LlamaModelConfig(config, dense_fp8="quantization_config" in config), mxfp4=True)


def test_supported_shapes_splits_and_empty_batches_are_host_arithmetic():
    lib = _hip.load()
    ok, splits = lib.swl_gemm_mxfp4_supported, lib.swl_gemm_mxfp4_choose_splits
    assert ok(6144, 4096, _hip.SWL_BF16) == 1 and ok(16, 128, _hip.SWL_BF16) == 1
    assert not any((ok(6144, 4096, _hip.SWL_F16), ok(6152, 4096, 1), ok(4096, 4160, 1), ok(0, 128, 1), ok(4096, 4096, 2)))
    # a function of (N, K) alone: a power of two <= 8, a slice keeps >= 1024 k, 1 where the row groups fill the card already
    assert splits(28672, 4096) == 1 and splits(14336, 4096) == 2 and splits(4096, 4096) == 4 and splits(4096, 14336) == 4
    assert splits(6144, 4096) == 4 and splits(1024, 32768) == 8 and splits(16, 128) == 1 and splits(80, 1152) == 1
    assert splits(100, 4096) == 0 and splits(4096, 4160) == 0
    assert [L.max_splits(k) for k in (128, 384, 1152, 4096)] == [1, 2, 8, 8] and L.scale_bytes(80, 1152) == 5 * 3 * 256
    for name in BASE:                                       # an empty batch is OK and launches nothing
        if "num_tokens" in BASE[name]:
            assert run(name, num_tokens=0, **{k: None for k, v in BASE[name].items() if v == P}) == OK


@no_device
@pytest.mark.parametrize("name", list(BASE))
def test_validation(name):
    gemm = "num_tokens" in BASE[name]
    assert run(name) == LAUNCH
    assert run(name, dtype=_hip.SWL_F16) == (LAUNCH if name.endswith("quantise_pack") else UNSUPPORTED)
    for field, v in BASE[name].items():                     # null operands, the scales among them
        if v == P and field != "workspace":
            assert run(name, **{field: None}) == BAD, field
    for field in ("x", "codes", "scales") if gemm else ORDERS[name][:3]:
        assert run(name, **{field: P + 8}) == BAD, field
    rows = "inter" if "inter" in BASE[name] else "n"
    for change, want in ((dict(dtype=2), BAD), (dict(k=1216), UNSUPPORTED), ({rows: 72}, UNSUPPORTED),    # 1216 % 64 == 0, % 128 != 0
                         (dict(k=1280, **({"x_row_stride": 1280} if gemm else {})), LAUNCH)):
        assert run(name, **change) == want, change
    if gemm:
        for change, want in ((dict(num_tokens=-1), BAD), (dict(num_tokens=65), UNSUPPORTED), (dict(num_tokens=64), LAUNCH),
                             (dict(x_row_stride=1144), BAD), (dict(k_splits=3), BAD), (dict(k_splits=16), BAD),
                             (dict(k_splits=8), LAUNCH), (dict(k=512, x_row_stride=512, k_splits=8), BAD),   # 8 > 4 k tiles
                             (dict(k_splits=4, workspace=None), BAD),
                             (dict(k_splits=4, workspace_bytes=4 * 17 * (160 if rows == "inter" else 80) * 4 - 1), BAD),
                             (dict(k_splits=1, workspace=None, workspace_bytes=0), LAUNCH)):
            assert run(name, **change) == want, change
