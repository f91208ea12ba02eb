"""Argument validation of swl_qk_prep_rotary, observed without a device as tests/test_guided_abi.py does: validation
runs before any launch, so an accepted call comes back as SWL_ERR_LAUNCH (-3) and a refused one as -1 (bad argument). With a
device present the accepted baseline would launch on fake host pointers, so the module skips."""
import os
import re

import pytest
import torch

from swiftllm_amd import _hip

if torch.cuda.is_available():
    pytest.skip("argument validation is observed without a device (a baseline would launch on host pointers)",
                allow_module_level=True)

OK, BAD, LAUNCH = 0, -1, -3
P = 0x10000          # a 16-byte aligned, never dereferenced "pointer"

ORDER = ("q", "k", "v", "q_bias", "k_bias", "v_bias", "q_norm_w", "k_norm_w", "eps", "cos_table", "sin_table", "pos_idx",
         "num_tokens", "num_q_heads", "num_kv_heads", "head_dim", "q_tok_stride", "k_tok_stride", "v_tok_stride", "dtype",
         "stream")
# Qwen3-8B rows inside one fused qkv output: 32 + 8 + 8 heads of 128
BASE = dict(q=P, k=P, v=P, q_bias=P, k_bias=P, v_bias=P, q_norm_w=P, k_norm_w=P, eps=1e-6, cos_table=P, sin_table=P, pos_idx=P,
            num_tokens=37, num_q_heads=32, num_kv_heads=8, head_dim=128, q_tok_stride=6144, k_tok_stride=6144,
            v_tok_stride=6144, dtype=_hip.SWL_BF16, stream=None)


def prep(**change):
    args = dict(BASE, **change)
    return _hip.load().swl_qk_prep_rotary(*[args[k] for k in ORDER])


def test_entry_is_registered_with_its_types_and_matches_the_header():
    argtypes, restype = _hip._SPECIAL["swl_qk_prep_rotary"]
    assert len(ORDER) == len(argtypes) == 21 and restype is _hip._I32
    assert argtypes[ORDER.index("eps")] is _hip._F32 and argtypes[ORDER.index("num_tokens")] is _hip._I64
    assert all(argtypes[ORDER.index(n)] is _hip._I64 for n in ("q_tok_stride", "k_tok_stride", "v_tok_stride"))
    assert "swl_qk_prep_rotary" not in _hip.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "swiftllm_hip.h"), encoding="utf-8").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+swl_qk_prep_rotary\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m is not None and len(m.group(1).split(",")) == len(argtypes)
    names = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert tuple(names) == ORDER
    assert hasattr(_hip.load(), "swl_qk_prep_rotary")
    assert _hip.ABI_VERSION == 2 and _hip.load().swl_abi_version() == 2       # additive: the version stays


def test_baseline_forms_are_accepted_and_an_empty_batch_is_ok():
    assert prep() == LAUNCH
    assert prep(dtype=_hip.SWL_F16) == LAUNCH
    assert prep(q_bias=None, k_bias=None, v_bias=None) == LAUNCH                            # norm only
    assert prep(q_bias=None, k_bias=None, v_bias=None, v=None, v_tok_stride=0) == LAUNCH    # ... v is then not looked at
    assert prep(q_norm_w=None, k_norm_w=None) == LAUNCH                                     # bias only
    assert prep(q_norm_w=None, k_norm_w=None, q_bias=None, k_bias=None, v_bias=None, v=None) == LAUNCH   # neither
    assert prep(v_bias=None, v=None) == LAUNCH                                              # each bias on its own
    assert prep(pos_idx=None) == LAUNCH                                                     # row t
    assert prep(q_tok_stride=4096, k_tok_stride=1024, v_tok_stride=1024) == LAUNCH          # dense rows
    for d in (32, 64, 128, 256):
        assert prep(head_dim=d, num_q_heads=5, num_kv_heads=1, q_tok_stride=7 * d + 8, k_tok_stride=7 * d + 8,
                    v_tok_stride=7 * d + 8) == LAUNCH
    assert prep(eps=0.0) == LAUNCH
    assert prep(num_tokens=0) == OK
    assert prep(num_tokens=0, q=None, k=None, v=None, cos_table=None, sin_table=None, q_norm_w=None) == OK


@pytest.mark.parametrize("field", ["q", "k", "v", "cos_table", "sin_table"])
def test_refuses_null_operands(field):
    assert prep(**{field: None}) == BAD


@pytest.mark.parametrize("field", ["q_norm_w", "k_norm_w"])
def test_refuses_one_norm_weight_without_its_twin(field):
    assert prep(**{field: None}) == BAD


@pytest.mark.parametrize("field", ["q", "k", "v", "q_bias", "k_bias", "v_bias", "q_norm_w", "k_norm_w", "cos_table", "sin_table"])
def test_refuses_misaligned_pointers(field):
    assert prep(**{field: P + 8}) == BAD
    assert prep(**{field: P + 2}) == BAD


@pytest.mark.parametrize("change", [dict(num_tokens=-1), dict(num_q_heads=0), dict(num_kv_heads=0), dict(num_q_heads=-32),
                                    dict(head_dim=0), dict(head_dim=-128), dict(head_dim=16), dict(head_dim=96),
                                    dict(head_dim=512), dict(q_tok_stride=4095), dict(q_tok_stride=4100),
                                    dict(k_tok_stride=1016), dict(k_tok_stride=1028), dict(v_tok_stride=1016),
                                    dict(v_tok_stride=6148), dict(q_tok_stride=0), dict(q_tok_stride=-6144),
                                    dict(dtype=2), dict(dtype=-1), dict(eps=-1e-6), dict(eps=float("nan"))])
def test_refuses_bad_arguments(change):
    assert prep(**change) == BAD


def test_v_stride_is_not_looked_at_without_a_v_bias():
    assert prep(v_bias=None, v_tok_stride=3) == LAUNCH
    assert prep(v_bias=None, v=P + 2) == LAUNCH
