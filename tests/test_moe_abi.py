"""The mixture-of-experts entry points (csrc/moe.hip): header <-> _hip._SPECIAL <-> library, and their argument validation
observed without a device as tests/test_qk_prep_abi.py does — validation runs before any launch, so an accepted call comes
back as SWL_ERR_LAUNCH (-3), a refused one as -1 (bad argument) or -2 (unsupported). With a device present the accepted
baseline would launch on fake host pointers, so those tests skip."""
import os
import re

import pytest
import torch

from swiftllm_amd import _hip

OK, BAD, UNSUPPORTED, LAUNCH = 0, -1, -2, -3
P = 0x10000          # a 16-byte aligned, never dereferenced "pointer"
no_device = pytest.mark.skipif(torch.cuda.is_available(),
                               reason="argument validation is observed without a device (a baseline would launch on host pointers)")

ORDERS = {
    "swl_moe_supported": ("hidden", "inter", "num_experts", "top_k", "dtype"),
    "swl_moe_max_pairs": (),
    "swl_moe_max_tiles": ("num_tokens", "top_k", "num_experts"),
    "swl_moe_route": ("topk_ids", "topk_w", "logits", "num_tokens", "num_experts", "top_k", "norm_topk_prob",
                      "logits_row_stride", "logits_dtype", "stream"),
    "swl_moe_align": ("tile_rows", "tile_experts", "topk_ids", "num_tokens", "top_k", "num_experts", "max_tiles", "stream"),
    "swl_moe_up_gate_silu": ("act", "x", "expert_up_gate", "tile_rows", "tile_experts", "max_tiles", "num_tokens", "top_k",
                             "hidden", "inter", "num_experts", "x_row_stride", "dtype", "stream"),
    "swl_moe_down": ("y", "act", "expert_down", "tile_rows", "tile_experts", "max_tiles", "num_tokens", "top_k", "hidden",
                     "inter", "num_experts", "dtype", "stream"),
    "swl_moe_combine": ("out", "y", "topk_w", "num_tokens", "top_k", "hidden", "out_row_stride", "dtype", "stream"),
}
# Qwen3-30B-A3B, 32 decode tokens
T, K, E, H, I = 32, 8, 128, 2048, 768
TILES = (T * K + 15) // 16 + min(E, T * K)
BASE = {
    "swl_moe_route": dict(topk_ids=P, topk_w=P, logits=P, num_tokens=T, num_experts=E, top_k=K, norm_topk_prob=1,
                          logits_row_stride=E, logits_dtype=_hip.SWL_BF16, stream=None),
    "swl_moe_align": dict(tile_rows=P, tile_experts=P, topk_ids=P, num_tokens=T, top_k=K, num_experts=E, max_tiles=TILES,
                          stream=None),
    "swl_moe_up_gate_silu": dict(act=P, x=P, expert_up_gate=P, tile_rows=P, tile_experts=P, max_tiles=TILES, num_tokens=T,
                                 top_k=K, hidden=H, inter=I, num_experts=E, x_row_stride=H, dtype=_hip.SWL_BF16, stream=None),
    "swl_moe_down": dict(y=P, act=P, expert_down=P, tile_rows=P, tile_experts=P, max_tiles=TILES, num_tokens=T, top_k=K,
                         hidden=H, inter=I, num_experts=E, dtype=_hip.SWL_BF16, stream=None),
    "swl_moe_combine": dict(out=P, y=P, topk_w=P, num_tokens=T, top_k=K, hidden=H, out_row_stride=H, dtype=_hip.SWL_BF16,
                            stream=None),
}


def run(name, **change):
    args = dict(BASE[name], **change)
    return getattr(_hip.load(), name)(*[args[k] for k in ORDERS[name]])


def test_entries_are_registered_with_their_types_and_match_the_header():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swiftllm_hip.h"),
                  encoding="utf-8").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, order in ORDERS.items():
        argtypes, restype = _hip._SPECIAL[name]
        assert len(order) == len(argtypes) and restype is _hip._I32, name
        assert name not in _hip.SIGNATURES
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m is not None, name
        params = [p for p in m.group(1).split(",") if p.strip() != "void"]
        assert tuple(p.split()[-1].lstrip("*") for p in params) == order, name
        for p, ctype in zip(params, argtypes):              # the C type of every parameter against the ctypes one
            want = (_hip._P if "*" in p or "swl_stream_t" in p else _hip._I64 if "int64_t" in p else _hip._I32)
            assert ctype is want, (name, p)
        assert hasattr(_hip.load(), name)
    assert "SWL_MOE_LOGITS_F32 2" in header
    assert _hip.ABI_VERSION == 2 and _hip.load().swl_abi_version() == 2       # additive: the version stays


def test_host_arithmetic():
    lib = _hip.load()
    assert lib.swl_moe_max_pairs() == 4096
    for t, k, e in ((1, 2, 4), (33, 2, 8), (200, 8, 128), (1, 8, 128), (512, 8, 128), (17, 1, 1), (16, 16, 256)):
        assert lib.swl_moe_max_tiles(t, k, e) == (t * k + 15) // 16 + min(e, t * k)
    assert lib.swl_moe_max_tiles(0, 2, 4) == 0
    assert lib.swl_moe_max_tiles(513, 8, 128) == 0          # past max_pairs: the caller walks token blocks
    assert lib.swl_moe_max_tiles(4, 5, 4) == 0 and lib.swl_moe_max_tiles(4, 2, 257) == 0 and lib.swl_moe_max_tiles(-1, 2, 4) == 0
    ok = lambda *a: lib.swl_moe_supported(*a)               # noqa: E731
    assert ok(2048, 768, 128, 8, _hip.SWL_BF16) == 1 and ok(4096, 14336, 8, 2, _hip.SWL_F16) == 1
    assert ok(256, 128, 8, 2, _hip.SWL_F16) == 1 and ok(256, 192, 4, 4, _hip.SWL_BF16) == 1 and ok(64, 32, 1, 1, 0) == 1
    assert ok(256, 128, 256, 16, 0) == 1 and ok(256, 128, 257, 2, 0) == 0 and ok(256, 128, 32, 17, 0) == 0
    assert ok(2080, 768, 128, 8, 1) == 0 and ok(2048, 760, 128, 8, 1) == 0 and ok(2048, 784, 128, 8, 1) == 0
    assert ok(256, 128, 2, 3, 0) == 0 and ok(256, 128, 8, 2, 2) == 0 and ok(0, 128, 8, 2, 0) == 0 and ok(256, -128, 8, 2, 0) == 0
    assert ok(256, 128, 0, 0, 0) == 0 and ok(16 * 65536, 128, 8, 2, 0) == 0


@pytest.mark.parametrize("name", list(BASE))
def test_an_empty_batch_is_ok_and_launches_nothing(name):
    nulls = {k: None for k, v in BASE[name].items() if v == P}
    assert run(name, num_tokens=0, **nulls) == OK
    assert run(name, num_tokens=0) == OK


@no_device
def test_baseline_forms_are_accepted():
    for name in BASE:
        assert run(name) == LAUNCH, name
    for name in ("swl_moe_up_gate_silu", "swl_moe_down", "swl_moe_combine"):
        assert run(name, dtype=_hip.SWL_F16) == LAUNCH
    for code in (_hip.SWL_F16, _hip.SWL_BF16, 2):
        assert run("swl_moe_route", logits_dtype=code) == LAUNCH
    assert run("swl_moe_route", norm_topk_prob=0, logits_row_stride=E + 3, logits=P + 2) == LAUNCH
    assert run("swl_moe_route", top_k=16, num_experts=16, num_tokens=256) == LAUNCH      # k == E, max_pairs
    assert run("swl_moe_align", max_tiles=TILES + 5) == LAUNCH
    assert run("swl_moe_up_gate_silu", x_row_stride=H + 8) == LAUNCH
    assert run("swl_moe_up_gate_silu", hidden=256, inter=192, x_row_stride=256, num_experts=4, top_k=2) == LAUNCH
    assert run("swl_moe_combine", out_row_stride=H + 8) == LAUNCH
    assert run("swl_moe_up_gate_silu", max_tiles=0) == OK and run("swl_moe_down", max_tiles=0) == OK


@no_device
@pytest.mark.parametrize("name", list(BASE))
def test_refuses_null_operands(name):
    for field, v in BASE[name].items():
        if v == P:
            assert run(name, **{field: None}) == BAD, (name, field)


@no_device
@pytest.mark.parametrize("name, field", [("swl_moe_up_gate_silu", "x"), ("swl_moe_up_gate_silu", "expert_up_gate"),
                                         ("swl_moe_down", "act"), ("swl_moe_down", "expert_down"),
                                         ("swl_moe_combine", "out"), ("swl_moe_combine", "y")])
def test_refuses_misaligned_pointers(name, field):
    assert run(name, **{field: P + 8}) == BAD
    assert run(name, **{field: P + 2}) == BAD


@no_device
@pytest.mark.parametrize("name", ["swl_moe_route", "swl_moe_align", "swl_moe_up_gate_silu", "swl_moe_down"])
@pytest.mark.parametrize("change, want", [(dict(num_tokens=-1), BAD), (dict(top_k=0), BAD), (dict(num_experts=0), BAD),
                                          (dict(top_k=-2), BAD), (dict(top_k=3, num_experts=2), BAD),
                                          (dict(num_experts=257), UNSUPPORTED), (dict(top_k=17), UNSUPPORTED),
                                          (dict(num_tokens=513), UNSUPPORTED), (dict(num_tokens=1 << 30), UNSUPPORTED)])
def test_refuses_an_illegal_step(name, change, want):
    assert run(name, **change) == want


@no_device
@pytest.mark.parametrize("name, change, want", [
    ("swl_moe_route", dict(logits_row_stride=E - 1), BAD), ("swl_moe_route", dict(logits_dtype=3), BAD),
    ("swl_moe_route", dict(logits_dtype=-1), BAD),
    ("swl_moe_align", dict(max_tiles=TILES - 1), BAD), ("swl_moe_align", dict(max_tiles=0), BAD),
    ("swl_moe_align", dict(max_tiles=1 << 20), BAD),
    ("swl_moe_up_gate_silu", dict(hidden=0), BAD), ("swl_moe_up_gate_silu", dict(inter=-768), BAD),
    ("swl_moe_up_gate_silu", dict(x_row_stride=H - 8), BAD), ("swl_moe_up_gate_silu", dict(dtype=2), BAD),
    ("swl_moe_up_gate_silu", dict(max_tiles=-1), BAD), ("swl_moe_up_gate_silu", dict(max_tiles=1 << 20), BAD),
    ("swl_moe_up_gate_silu", dict(hidden=2080, x_row_stride=2080), UNSUPPORTED),
    ("swl_moe_up_gate_silu", dict(inter=760), UNSUPPORTED), ("swl_moe_up_gate_silu", dict(x_row_stride=H + 4), UNSUPPORTED),
    ("swl_moe_down", dict(hidden=-1), BAD), ("swl_moe_down", dict(dtype=-1), BAD), ("swl_moe_down", dict(max_tiles=-1), BAD),
    ("swl_moe_down", dict(max_tiles=1 << 20), BAD),
    ("swl_moe_down", dict(hidden=2080), UNSUPPORTED), ("swl_moe_down", dict(inter=784), UNSUPPORTED),
    ("swl_moe_combine", dict(num_tokens=-1), BAD), ("swl_moe_combine", dict(top_k=0), BAD),
    ("swl_moe_combine", dict(hidden=0), BAD), ("swl_moe_combine", dict(out_row_stride=H - 8), BAD),
    ("swl_moe_combine", dict(dtype=2), BAD), ("swl_moe_combine", dict(top_k=17), UNSUPPORTED),
    ("swl_moe_combine", dict(hidden=2052, out_row_stride=2056), UNSUPPORTED),
    ("swl_moe_combine", dict(out_row_stride=H + 4), UNSUPPORTED), ("swl_moe_combine", dict(num_tokens=513), UNSUPPORTED),
])
def test_refuses_bad_arguments(name, change, want):
    assert run(name, **change) == want
