"""Argument validation of swl_guide_build_masks and swl_logits_mask, observed without a device as
tests/test_logprobs_abi.py does: validation runs before any launch, so an accepted call comes back as SWL_ERR_LAUNCH (-3)
and a refused one as -1 (bad argument) / -2 (unsupported). With a device present the accepted baseline would launch on fake
host pointers, so the module skips."""
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

BUILD_ORDER = ("masks", "row_base", "num_states", "words_per_row", "trans", "accepting", "tok_bytes", "tok_offsets", "vocab",
               "end_ids", "num_end_ids", "stream")
BUILD = dict(masks=P, row_base=5, num_states=40, words_per_row=32, trans=P, accepting=P, tok_bytes=P, tok_offsets=P,
             vocab=1003, end_ids=P, num_end_ids=2, stream=None)
MASK_ORDER = ("logits", "num_rows", "n", "row_stride", "dtype", "masks", "num_mask_rows", "words_per_row", "row_index",
              "stream")
MASK = dict(logits=P, num_rows=4, n=1003, row_stride=1011, dtype=_hip.SWL_BF16, masks=P, num_mask_rows=64, words_per_row=32,
            row_index=P, stream=None)


def build(**change):
    args = dict(BUILD, **change)
    return _hip.load().swl_guide_build_masks(*[args[k] for k in BUILD_ORDER])


def mask(**change):
    args = dict(MASK, **change)
    return _hip.load().swl_logits_mask(*[args[k] for k in MASK_ORDER])


@pytest.mark.parametrize("name,order", [("swl_guide_build_masks", BUILD_ORDER), ("swl_logits_mask", MASK_ORDER)])
def test_entries_are_registered_with_their_types_and_match_the_header(name, order):
    argtypes, restype = _hip._SPECIAL[name]
    assert len(order) == len(argtypes) and restype is _hip._I32
    assert name not in _hip.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "swiftllm_hip.h"), encoding="utf-8").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m is not None and len(m.group(1).split(",")) == len(argtypes)
    assert hasattr(_hip.load(), name)
    assert _hip.ABI_VERSION == 2 and _hip.load().swl_abi_version() == 2       # additive: the version stays


def test_build_baseline_is_accepted_and_an_empty_guide_is_ok():
    assert build() == LAUNCH
    assert build(row_base=0, num_states=1) == LAUNCH
    assert build(words_per_row=40) == LAUNCH                    # rows wider than the vocabulary are fine
    assert build(end_ids=None, num_end_ids=0) == LAUNCH
    assert build(vocab=4096, words_per_row=128) == LAUNCH
    assert build(num_states=0) == OK
    assert build(num_states=0, masks=None, trans=None, accepting=None, tok_bytes=None, tok_offsets=None, end_ids=None) == OK


@pytest.mark.parametrize("field", ["masks", "trans", "accepting", "tok_bytes", "tok_offsets", "end_ids"])
def test_build_refuses_null_pointers(field):
    assert build(**{field: None}) == BAD


@pytest.mark.parametrize("change", [dict(row_base=-1), dict(num_states=-1), dict(words_per_row=31), dict(words_per_row=0),
                                    dict(words_per_row=-32), dict(vocab=0), dict(vocab=-1003), dict(num_end_ids=-1),
                                    dict(vocab=1025)])
def test_build_refuses_bad_arguments(change):
    assert build(**change) == BAD


def test_build_sizes_beyond_int32_are_unsupported():
    assert build(num_states=1 << 23) == UNSUP                   # 256 * states no longer indexes trans in int32
    assert build(row_base=0x7fffffff, num_states=1) == UNSUP
    assert build(row_base=1 << 40) == UNSUP
    assert build(words_per_row=1 << 26) == UNSUP


def test_mask_baseline_is_accepted_and_an_empty_batch_is_ok():
    assert mask() == LAUNCH
    assert mask(logits=P + 2) == LAUNCH                         # 2-byte alignment is all the logits need
    assert mask(n=1024, row_stride=1024, dtype=_hip.SWL_F16) == LAUNCH
    assert mask(num_mask_rows=0) == LAUNCH                      # no row can be guided: every row returns at once
    assert mask(num_rows=0x7fffffff) == LAUNCH
    assert mask(num_rows=0) == OK
    assert mask(num_rows=0, logits=None, masks=None, row_index=None) == OK


@pytest.mark.parametrize("field", ["logits", "masks", "row_index"])
def test_mask_refuses_null_pointers(field):
    assert mask(**{field: None}) == BAD


@pytest.mark.parametrize("change", [dict(n=0), dict(n=-5), dict(row_stride=1002), dict(row_stride=0), dict(row_stride=-1011),
                                    dict(dtype=2), dict(dtype=-1), dict(logits=P + 1), dict(logits=P + 7),
                                    dict(num_rows=-1), dict(num_mask_rows=-1), dict(words_per_row=31),
                                    dict(words_per_row=0), dict(n=1025, row_stride=1032)])
def test_mask_refuses_bad_arguments(change):
    assert mask(**change) == BAD


def test_mask_too_many_rows_are_unsupported():
    assert mask(num_rows=0x80000000) == UNSUP
    assert mask(num_rows=1 << 40) == UNSUP
    assert mask(num_mask_rows=0x80000000) == UNSUP
