"""Argument validation of swl_logprobs, observed without a device as tests/test_logits_adjust_abi.py does: validation
runs before any launch, so an accepted call comes back as SWL_ERR_LAUNCH (-3) and a refused one as -1 (bad argument) /
-2 (unsupported). With a device present the accepted baseline would launch on fake host pointers, so the module skips."""
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
ORDER = ("lp", "ids", "rank", "logits", "num_rows", "n", "row_stride", "dtype", "chosen", "top_n", "n_cap", "stream")
BASE = dict(lp=P, ids=P, rank=P, logits=P, num_rows=4, n=1003, row_stride=1011, dtype=_hip.SWL_BF16, chosen=P, top_n=P,
            n_cap=20, stream=None)


def call(**change):
    args = dict(BASE, **change)
    return _hip.load().swl_logprobs(*[args[k] for k in ORDER])


def test_entry_is_registered_with_its_types_and_matches_the_header():
    argtypes, restype = _hip._SPECIAL["swl_logprobs"]
    assert len(ORDER) == len(argtypes) == 12 and restype is _hip._I32
    assert "swl_logprobs" not in _hip.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "swiftllm_hip.h"), encoding="utf-8").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+swl_logprobs\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m is not None and len(m.group(1).split(",")) == len(argtypes)
    assert hasattr(_hip.load(), "swl_logprobs")
    assert _hip.ABI_VERSION == 2 and _hip.load().swl_abi_version() == 2       # additive: the version stays


def test_baseline_is_accepted_and_an_empty_batch_is_ok():
    assert call() == LAUNCH
    assert call(logits=P + 2) == LAUNCH                 # 2-byte alignment is all the logits need
    assert call(n=1000, row_stride=1000, dtype=_hip.SWL_F16) == LAUNCH
    assert call(n_cap=0) == LAUNCH
    assert call(num_rows=0x7fffffff) == LAUNCH
    assert call(num_rows=0) == OK
    assert call(num_rows=0, lp=None, ids=None, rank=None, logits=None, chosen=None, top_n=None) == OK


@pytest.mark.parametrize("field", ["lp", "ids", "rank", "logits", "chosen", "top_n"])
def test_null_pointers_are_refused(field):
    assert call(**{field: None}) == BAD


@pytest.mark.parametrize("change", [dict(n=0), dict(n=-5), dict(row_stride=1002), dict(row_stride=0), dict(row_stride=-1011),
                                    dict(dtype=2), dict(dtype=-1), dict(logits=P + 1), dict(logits=P + 7),
                                    dict(n_cap=-1), dict(n_cap=21), dict(num_rows=-1)])
def test_bad_arguments_are_refused(change):
    assert call(**change) == BAD


def test_too_many_rows_are_unsupported():
    assert call(num_rows=0x80000000) == UNSUP
    assert call(num_rows=1 << 40) == UNSUP
