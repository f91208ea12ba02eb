"""The row-tile expert GEMM entries (csrc/moe_wide.hip): header <-> _hip._SPECIAL <-> library, the chooser's host arithmetic,
and argument validation observed without a device as tests/test_moe_abi.py does (accepted calls skip with a device)."""
import os
import re

import pytest

from swiftllm_amd import _hip
from test_moe_abi import BAD, BASE as TWIN, LAUNCH, OK, ORDERS as TWIN_ORDERS, P, UNSUPPORTED, no_device

ORDERS = {"swl_moe_wide_row_tiles": ("num_tokens", "top_k", "num_experts", "hidden", "inter")}
BASE = {}
for _twin in ("swl_moe_up_gate_silu", "swl_moe_down"):      # the twin's arguments, row_tiles before dtype
    _order = list(TWIN_ORDERS[_twin])
    _order.insert(_order.index("dtype"), "row_tiles")
    ORDERS[_twin + "_wide"], BASE[_twin + "_wide"] = tuple(_order), dict(TWIN[_twin], row_tiles=4)


def run(name, **change):
    args = dict(BASE[name], **change)
    return getattr(_hip.load(), name)(*[args[k] for k in ORDERS[name]])


def test_entries_are_registered_with_their_types_and_match_the_header():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swiftllm_hip.h"),
                  encoding="utf-8").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, order in ORDERS.items():
        argtypes, restype = _hip._SPECIAL[name]
        assert len(order) == len(argtypes) and restype is _hip._I32 and hasattr(_hip.load(), name), name
        params = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).split(",")
        assert tuple(p.split()[-1].lstrip("*") for p in params) == order, name
        for p, ctype in zip(params, argtypes):
            want = (_hip._P if "*" in p or "swl_stream_t" in p else _hip._I64 if "int64_t" in p else _hip._I32)
            assert ctype is want, (name, p)


def test_the_chooser_and_empty_batches_are_host_arithmetic():
    f = _hip.load().swl_moe_wide_row_tiles
    assert f(32, 8, 128, 2048, 768) == 0 and f(513, 8, 128, 2048, 768) == 0 and f(-1, 2, 8, 256, 128) == 0
    for t, k, e, h, i in ((1, 2, 8, 4096, 14336), (127, 2, 8, 4096, 14336), (128, 2, 8, 4096, 14336),
                          (511, 8, 128, 2048, 768), (512, 8, 128, 2048, 768), (2048, 2, 4, 256, 128)):
        got = f(t, k, e, h, i)
        assert got in (0, 2, 4) and got == f(t, k, e, h, i) and (got == 0) == (t * k // e < 32), (t, k, e)
    for name in BASE:                                       # an empty batch is OK and launches nothing
        nulls = {k: None for k, v in BASE[name].items() if v == P}
        assert run(name, num_tokens=0, **nulls) == OK and run(name, max_tiles=0, **nulls) == OK


@no_device
@pytest.mark.parametrize("name", list(BASE))
def test_validation_is_the_twin_s_plus_row_tiles(name):
    assert run(name) == LAUNCH and run(name, row_tiles=2) == LAUNCH
    for rt, want in ((0, BAD), (-1, BAD), (3, UNSUPPORTED), (16, UNSUPPORTED)):
        assert run(name, row_tiles=rt) == want, rt
    for field, v in BASE[name].items():                     # null operands; the aligned ones misaligned
        if v == P:
            assert run(name, **{field: None}) == BAD, field
    for field in ("x", "expert_up_gate") if "x" in BASE[name] else ("act", "expert_down"):
        assert run(name, **{field: P + 8}) == BAD, field
    for change, want in ((dict(num_tokens=-1), BAD), (dict(top_k=0), BAD), (dict(top_k=3, num_experts=2), BAD),
                         (dict(num_experts=257), UNSUPPORTED), (dict(top_k=17), UNSUPPORTED),
                         (dict(num_tokens=513), UNSUPPORTED)):          # illegal steps; 513 tokens at k 8
        assert run(name, **change) == want, change
