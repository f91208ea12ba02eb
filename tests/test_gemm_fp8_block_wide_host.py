"""The 65..256-token dense block-scaled FP8 entries without a device (csrc/gemm_fp8_block_wide.hip): the ABI rows, the
refusals — those of the 64-row entries, the token limit moved to 256 —, the wide chooser and the engine option."""
import re

import pytest

from swiftllm_amd import _hip
from swiftllm_amd.engine_config import EngineConfig
from test_abi import HEADER
from test_gemm_fp8_block_host import BASE as BASE64, ENGINE, ORDERS as ORDERS64
from test_moe_abi import BAD, LAUNCH, OK, P, UNSUPPORTED, no_device

NAMES = {"swl_gemm_fp8_block_wide": "swl_gemm_fp8_block", "swl_gemm_fp8_block_wide_silu_gate": "swl_gemm_fp8_block_silu_gate"}
ORDERS = dict({w: ORDERS64[n] for w, n in NAMES.items()}, swl_gemm_fp8_block_wide_choose_splits=("n", "k"))
BASE = {w: dict(BASE64[n], num_tokens=200, workspace_bytes=1 << 21) for w, n in NAMES.items()}


def run(name, **change):
    args = dict(BASE[name], **change)
    return getattr(_hip.load(), name)(*[args[k] for k in ORDERS[name]])


def test_the_three_names_are_exported_and_match_the_header():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER, encoding="utf-8").read(), flags=re.S)
    for name, order in ORDERS.items():
        argtypes, restype = _hip._SPECIAL[name]
        assert name not in _hip.SIGNATURES and len(order) == len(argtypes) and restype is _hip._I32 and hasattr(_hip.load(), name)
        params = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).split(",")
        assert tuple(p.split()[-1].lstrip("*") for p in params) == order, name
        for p, ctype in zip(params, argtypes):
            assert ctype is (_hip._P if "*" in p or "swl_stream_t" in p else _hip._I64 if "int64_t" in p else _hip._I32), (name, p)


@no_device
@pytest.mark.parametrize("name", list(BASE))
def test_refusals(name):
    assert run(name) == LAUNCH and run(name, dtype=_hip.SWL_F16) == LAUNCH
    assert run(name, num_tokens=0, **{k: None for k, v in BASE[name].items() if v == P}) == OK
    seg = "inter" if "inter" in BASE[name] else "seg1"
    slab = 200 * (384 if seg == "inter" else 320) * 4      # bytes of one slice's slab: 200 rows x the weight rows
    for change, want in ((dict(num_tokens=-1), BAD), (dict(num_tokens=257), UNSUPPORTED), (dict(num_tokens=256), LAUNCH),
                         (dict(num_tokens=1), LAUNCH), (dict(bscale=None), BAD), (dict(x=P + 8), BAD),
                         (dict(k=608, k_blocks=5), UNSUPPORTED), ({seg: 72}, UNSUPPORTED), (dict(scale_rows=5), BAD),
                         (dict(k_blocks=4), BAD), (dict(k=640, x_row_stride=640), LAUNCH), (dict(k_splits=3), BAD),
                         (dict(k_splits=8), BAD), (dict(k_splits=4), LAUNCH), (dict(k_splits=4, workspace=None), BAD),
                         (dict(k_splits=4, workspace_bytes=4 * slab - 1), BAD), (dict(k_splits=4, workspace_bytes=4 * slab), LAUNCH),
                         (dict(workspace_bytes=2 * slab - 1), BAD),     # k_splits 0: the wide chooser's 2 slices
                         (dict(k_splits=1, workspace=None, workspace_bytes=0), LAUNCH)):
        assert run(name, **change) == want, change


def test_the_wide_chooser_is_a_function_of_the_weight_rows_and_k():
    splits = _hip.load().swl_gemm_fp8_block_wide_choose_splits
    # Llama-3-8B: qkv, o, [up ; gate], down. One workgroup (64 weight rows) a CU: a slice more only while the grid fits 256
    assert [splits(n, k) for n, k in ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336))] == [2, 4, 1, 4]
    assert splits(384, 2112) == 8 and splits(320, 576) == 2 and splits(256, 128) == 1 and splits(64, 1 << 20) == 8
    assert splits(100, 4096) == 0 and splits(4096, 100) == 0 and splits(0, 64) == 0
    for n in range(16, 20000, 976):
        for k in range(64, 20000, 1472):
            ks = splits(n, k)
            assert ks in (1, 2, 4, 8) and ks <= (k + 127) // 128, (n, k, ks)


def test_the_engine_option_needs_the_fp8_block_weights():
    assert EngineConfig(**ENGINE).dense_fp8_wide is False
    assert EngineConfig(**ENGINE, dense_weight_dtype="fp8_block", dense_fp8_wide=True).dense_fp8_wide is True
    with pytest.raises(ValueError, match="dense_fp8_wide=True needs dense_weight_dtype='fp8_block'"):
        EngineConfig(**ENGINE, dense_fp8_wide=True)
