"""Per-row FP8 dense projections of a 16-bit checkpoint without a device: the engine option and its refusals, the host
arithmetic of csrc/gemm_fp8_row.hip and the argument validation of its entries (observed as tests/test_gemm_fp8_block_host.py
does: a call that passes every check fails at the launch, nothing is dereferenced)."""
import pytest

from swiftllm_amd import _hip
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.model_config import LlamaModelConfig
from swiftllm_amd.worker.weight import dense_fp8_row_refusal
from test_gemm_fp8_block_host import DENSE, ENGINE
from test_moe_abi import BAD, LAUNCH, OK, P, UNSUPPORTED, no_device
from test_moe_fp8_block_host import MOE

ORDERS = {
    "swl_gemm_fp8_row_quantise_pack": ("codes", "w", "inv_scale", "n", "k", "dtype", "stream"),
    "swl_gemm_fp8_row": ("y", "x", "codes", "scale", "workspace", "workspace_bytes", "num_tokens", "n", "k", "x_row_stride",
                         "k_splits", "dtype", "stream"),
    "swl_gemm_fp8_row_silu_gate": ("act", "x", "codes", "scale", "workspace", "workspace_bytes", "num_tokens", "inter", "k",
                                   "x_row_stride", "k_splits", "dtype", "stream"),
    "swl_fp8_row_dequant": ("out", "codes", "scale", "n", "k", "dtype", "stream"),
}
BASE = {
    "swl_gemm_fp8_row_quantise_pack": dict(codes=P, w=P, inv_scale=P, n=80, k=576, dtype=_hip.SWL_BF16, stream=None),
    "swl_gemm_fp8_row": dict(y=P, x=P, codes=P, scale=P, workspace=P, workspace_bytes=1 << 20, num_tokens=17, n=80, k=576,
                             x_row_stride=576, k_splits=0, dtype=_hip.SWL_BF16, stream=None),
    "swl_gemm_fp8_row_silu_gate": dict(act=P, x=P, codes=P, scale=P, workspace=P, workspace_bytes=1 << 20, num_tokens=17,
                                       inter=80, k=576, x_row_stride=576, k_splits=0, dtype=_hip.SWL_BF16, stream=None),
    "swl_fp8_row_dequant": dict(out=P, codes=P, scale=P, n=80, k=576, dtype=_hip.SWL_BF16, stream=None),
}
PLAIN = {k: v for k, v in DENSE.items() if k != "quantization_config"}      # a 16-bit Llama: hidden 256, inter 512


def run(name, **change):
    args = dict(BASE[name], **change)
    return getattr(_hip.load(), name)(*[args[k] for k in ORDERS[name]])


def test_the_option_takes_the_new_value():
    assert EngineConfig(**ENGINE, dense_weight_dtype="fp8_e4m3").dense_weight_dtype == "fp8_e4m3"
    assert dense_fp8_row_refusal(LlamaModelConfig(PLAIN)) == ""
    for name, order in ORDERS.items():
        assert name not in _hip.SIGNATURES and len(_hip._SPECIAL[name][0]) == len(order), name


@pytest.mark.parametrize("kw, reason", [(dict(tuning={"decode_engine": True}), "decode_engine"), (dict(max_loras=1), "max_loras"),
                                        (dict(dense_fp8_wide=True), "needs dense_weight_dtype='fp8_block'")])
def test_the_engine_option_refuses_what_it_does_not_serve(kw, reason):
    with pytest.raises(ValueError, match=reason):
        EngineConfig(**{**ENGINE, "dense_weight_dtype": "fp8_e4m3", **kw})


@pytest.mark.parametrize("config, reason", [
    (MOE, "moe_weight_dtype"),
    (DENSE, "dense_weight_dtype='fp8_block'"),             # a checkpoint with a quantization_config
    (dict(PLAIN, intermediate_size=480), "multiples of 16 rows and of 64 columns"),
    (dict(PLAIN, hidden_size=64, num_attention_heads=8, num_key_value_heads=1), "k_proj is 8 x 64"),
], ids=["moe", "quantised", "inter", "kv_size"])
def test_the_model_refusals_name_their_reason(config, reason):
    assert reason in dense_fp8_row_refusal(LlamaModelConfig(config, dense_fp8="quantization_config" in config))


def test_supported_shapes_splits_and_empty_batches_are_host_arithmetic():
    lib = _hip.load()
    ok, splits = lib.swl_gemm_fp8_row_supported, lib.swl_gemm_fp8_row_choose_splits
    assert ok(6144, 4096, _hip.SWL_BF16) == 1 and ok(80, 576, _hip.SWL_F16) == 1 and ok(16, 64, 0) == 1
    assert ok(6152, 4096, 0) == 0 and ok(4096, 4128, 0) == 0 and ok(4096, 4096, 2) == 0 and ok(0, 64, 0) == 0
    # a function of (N, K) alone: a power of two <= 8, a slice keeps >= 512 k, 1 where the row groups fill the card already
    assert splits(28672, 4096) == 1 and splits(14336, 4096) == 2 and splits(4096, 4096) == 4 and splits(4096, 14336) == 4
    assert splits(6144, 4096) == 4 and splits(1024, 4096) == 8 and splits(16, 64) == 1 and splits(80, 576) == 1
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
    for field in ("x", "codes", "scale") if gemm else ORDERS[name][:2]:
        assert run(name, **{field: P + 8}) == BAD, field
    rows = "inter" if "inter" in BASE[name] else "n"
    for change, want in ((dict(dtype=2), BAD), (dict(k=608), UNSUPPORTED), ({rows: 72}, UNSUPPORTED),    # 608 % 32 == 0, % 64 != 0
                         (dict(k=640, **({"x_row_stride": 640} if gemm else {})), LAUNCH)):
        assert run(name, **change) == want, change
    if gemm:
        for change, want in ((dict(num_tokens=-1), BAD), (dict(num_tokens=65), UNSUPPORTED), (dict(num_tokens=64), LAUNCH),
                             (dict(x_row_stride=568), BAD), (dict(k_splits=3), BAD), (dict(k_splits=16), BAD),
                             (dict(k_splits=8), LAUNCH), (dict(k=256, x_row_stride=256, k_splits=8), BAD),   # 8 > 4 k tiles
                             (dict(k_splits=4, workspace=None), BAD),
                             (dict(k_splits=4, workspace_bytes=4 * 17 * (160 if rows == "inter" else 80) * 4 - 1), BAD),
                             (dict(k_splits=1, workspace=None, workspace_bytes=0), LAUNCH)):
            assert run(name, **change) == want, change
