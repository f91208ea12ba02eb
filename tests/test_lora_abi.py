"""Argument validation of swl_lora_shrink / swl_lora_expand, observed without a device as tests/test_logits_adjust_abi.py
does: validation runs before any launch, so an accepted call comes back as SWL_ERR_LAUNCH (-3) and a refused one as -1 (bad
argument) / -2 (unsupported). With a device present the accepted baseline would launch on fake pointers, so the module
skips. The slot of a row is device data the C entry cannot see: the wrapper (kernels/lora.build_tiles) refuses it."""
import ctypes
import os
import re

import pytest
import torch

from swiftllm_amd import _hip

if torch.cuda.is_available():
    pytest.skip("argument validation is observed without a device (a baseline would launch on host pointers)",
                allow_module_level=True)

OK, BAD, UNSUP, LAUNCH = 0, -1, -2, -3
P = 0x10000          # a 16-byte aligned, never dereferenced "pointer"

SHRINK_ORDER = ("t", "x", "a_stack", "tile_rows", "tile_slots", "num_tiles", "num_tokens", "k", "r_total", "num_slots",
                "x_row_stride", "dtype", "stream")
SHRINK = dict(t=P, x=P, a_stack=P, tile_rows=P, tile_slots=P, num_tiles=3, num_tokens=33, k=256, r_total=48, num_slots=4,
              x_row_stride=256, dtype=_hip.SWL_BF16, stream=None)
EXPAND_ORDER = ("y", "t", "b_stack", "scale", "tile_rows", "tile_slots", "parts", "num_parts", "num_tiles", "num_tokens", "n",
                "r_max", "r_total", "k_splits", "num_slots", "y_row_stride", "dtype", "stream")
EXPAND = dict(y=P, t=P, b_stack=P, scale=P, tile_rows=P, tile_slots=P, parts=((0, 128, 0), (128, 192, 16), (192, 256, 32)),
              num_tiles=3, num_tokens=33, n=256, r_max=16, r_total=48, k_splits=1, num_slots=4, y_row_stride=264,
              dtype=_hip.SWL_F16, stream=None)


def shrink(**change):
    args = dict(SHRINK, **change)
    return _hip.load().swl_lora_shrink(*[args[k] for k in SHRINK_ORDER])


def expand(**change):
    args = dict(EXPAND, **change)
    parts = args["parts"]
    if parts is not None:
        flat = [v for p in parts for v in p]
        keep = (ctypes.c_int32 * len(flat))(*flat)          # (a HOST array the entry reads during the call)
        args["parts"] = ctypes.addressof(keep)
        args.setdefault("num_parts", len(parts))
    else:
        args.setdefault("num_parts", 1)
    return _hip.load().swl_lora_expand(*[args[k] for k in EXPAND_ORDER])


def _header_params(name):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swiftllm_hip.h"),
                  encoding="utf-8").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m is not None, name
    return len(m.group(1).split(","))


def test_entries_are_registered_with_their_types_and_match_the_header():
    for name, order in (("swl_lora_shrink", SHRINK_ORDER), ("swl_lora_expand", EXPAND_ORDER), ("swl_lora_k_splits", ("k",))):
        argtypes, restype = _hip._SPECIAL[name]
        assert name not in _hip.SIGNATURES
        assert len(order) == len(argtypes) == _header_params(name) and restype is _hip._I32
    assert _hip.ABI_VERSION == 2 and _hip.load().swl_abi_version() == 2       # additive: the version stays


def test_k_splits_depend_on_k_alone():
    ks = _hip.load().swl_lora_k_splits
    assert [ks(k) for k in (128, 1024, 1152, 4096, 14336)] == [1, 1, 2, 4, 14]
    assert ks(0) == 0 and ks(-128) == 0


def test_baselines_are_accepted_and_empty_batches_launch_nothing():
    assert shrink() == LAUNCH and expand() == LAUNCH
    assert shrink(dtype=_hip.SWL_F16, k=1792, x_row_stride=2048, r_total=8) == LAUNCH
    for r_max in (8, 16, 32, 64):
        assert expand(r_max=r_max, r_total=3 * r_max, parts=((0, 128, 0), (128, 192, r_max), (192, 256, 2 * r_max))) == LAUNCH
    assert expand(parts=((0, 256, 0),), r_total=16) == LAUNCH
    nothing = dict(tile_rows=None, tile_slots=None)
    assert shrink(num_tiles=0) == OK and shrink(num_tokens=0) == OK
    assert shrink(num_tiles=0, t=None, x=None, a_stack=None, **nothing) == OK
    assert expand(num_tiles=0) == OK and expand(num_tokens=0) == OK
    assert expand(num_tiles=0, y=None, t=None, b_stack=None, scale=None, **nothing) == OK


@pytest.mark.parametrize("field", ["t", "x", "a_stack", "tile_rows", "tile_slots"])
def test_shrink_refuses_null_pointers(field):
    assert shrink(**{field: None}) == BAD


@pytest.mark.parametrize("field", ["y", "t", "b_stack", "scale", "tile_rows", "tile_slots", "parts"])
def test_expand_refuses_null_pointers(field):
    assert expand(**{field: None}) == BAD


@pytest.mark.parametrize("change", [dict(x_row_stride=-256), dict(x_row_stride=128), dict(k=0), dict(k=-128), dict(r_total=0),
                                    dict(num_slots=0), dict(num_tiles=-1), dict(num_tokens=-1), dict(dtype=2), dict(x=P + 8)])
def test_shrink_refuses_bad_arguments(change):
    assert shrink(**change) == BAD


@pytest.mark.parametrize("change", [dict(k=192, x_row_stride=192), dict(k=1000, x_row_stride=1000), dict(r_total=20),
                                    dict(x_row_stride=260), dict(r_total=512)])
def test_shrink_reports_unsupported_shapes(change):
    assert shrink(**change) == UNSUP


@pytest.mark.parametrize("change", [
    dict(y_row_stride=-264), dict(y_row_stride=128), dict(n=0), dict(k_splits=0), dict(num_slots=0), dict(num_tiles=-1),
    dict(dtype=-1), dict(y=P + 2),
    dict(parts=((0, 128, 0), (128, 192, 16))),                    # the parts do not reach n
    dict(parts=((0, 128, 0), (144, 256, 16))),                    # ... or leave a gap
    dict(parts=((0, 128, 0), (128, 256, 40))),                    # a part reads past r_total
    dict(parts=((0, 256, -16),))])
def test_expand_refuses_bad_arguments(change):
    assert expand(**change) == BAD


@pytest.mark.parametrize("change", [
    dict(r_max=24, r_total=72, parts=((0, 128, 0), (128, 192, 24), (192, 256, 48))), dict(r_max=4), dict(r_max=128),
    dict(parts=((0, 120, 0), (120, 256, 16))),                    # an N part that is no multiple of 16
    dict(parts=((0, 128, 0), (128, 256, 12))),                    # a t offset that is no multiple of 8
    dict(y_row_stride=260),
    dict(parts=tuple((64 * i, 64 * i + 64, 0) for i in range(5)), n=320, y_row_stride=320)])
def test_expand_reports_unsupported_shapes(change):
    assert expand(**change) == UNSUP


def test_the_wrapper_refuses_slots_outside_the_stacks_on_the_host():
    from swiftllm_amd.worker.kernels.lora import build_tiles
    with pytest.raises(ValueError, match=r"slots must be in \[-1, 4\)"):
        build_tiles([0, 1, 4], 4)
    with pytest.raises(ValueError, match="slots must be in"):
        build_tiles([0, -2], 4)
    rows, slots = build_tiles([3, -1, 3], 4)
    assert slots.tolist() == [3] and rows.tolist()[:3] == [0, 2, -1]
