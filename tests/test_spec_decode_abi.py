"""Argument validation of swl_paged_attn_verify and the values of swl_paged_attn_verify_max_tokens, observed without a
device as tests/test_abi_contract.py does: validation runs before any launch, so an accepted call comes back as
SWL_ERR_LAUNCH (-3) and a refused one as -1 (bad argument) / -2 (unsupported). With a device present the accepted
baseline would launch on fake host pointers, so the module skips."""
import pytest
import torch

from swiftllm_amd import _hip

if torch.cuda.is_available():
    pytest.skip("argument validation is observed without a device (a baseline would launch on host pointers)",
                allow_module_level=True)

OK, BAD, UNSUP, LAUNCH = 0, -1, -2, -3
P = 0x10000          # a 16-byte aligned, never dereferenced "pointer"
ORDER = ("o", "q", "k_cache", "v_cache", "block_table", "seq_ids", "cu_seqlens", "ctx_lens", "row_lens", "scratch",
         "softmax_scale", "num_seqs", "num_rows", "max_new_len", "max_total_len", "H", "KVH", "D", "L", "block_size",
         "cur_layer", "max_blocks_per_seq", "seq_block_size", "num_seq_blocks", "q_tok_stride", "o_tok_stride", "dtype",
         "stream")
# Llama-3-8B heads: 2 sequences, 7 rows, up to 4 new tokens behind up to 1096 resident ones, 5 splits of 256
BASE = dict(o=P, q=P, k_cache=P, v_cache=P, block_table=P, seq_ids=P, cu_seqlens=P, ctx_lens=P, row_lens=P, scratch=P,
            softmax_scale=128 ** -0.5, num_seqs=2, num_rows=7, max_new_len=4, max_total_len=1100, H=32, KVH=8, D=128, L=2,
            block_size=16, cur_layer=1, max_blocks_per_seq=69, seq_block_size=256, num_seq_blocks=5, q_tok_stride=4096,
            o_tok_stride=4096, dtype=_hip.SWL_BF16, stream=None)


def call(**change):
    args = dict(BASE, **change)
    return _hip.load().swl_paged_attn_verify(*[args[k] for k in ORDER])


def test_both_entries_are_registered_with_their_types():
    assert len(ORDER) == len(_hip._SPECIAL["swl_paged_attn_verify"][0]) == 28
    assert "swl_paged_attn_verify" not in _hip.SIGNATURES and "swl_paged_attn_verify_max_tokens" not in _hip.SIGNATURES
    assert _hip.ABI_VERSION == 2 and _hip.load().swl_abi_version() == 2       # additive: the version stays


@pytest.mark.parametrize("h,kvh,want", [(8, 8, 16), (8, 4, 8), (32, 8, 4), (16, 2, 2), (12, 4, 0), (32, 2, 0),
                                        (0, 8, 0), (8, 0, 0), (9, 2, 0)])
def test_max_tokens(h, kvh, want):
    """16 / G for G = 1, 2, 4, 8; 0 for G = 3, 16 and for head counts that are no GQA geometry."""
    assert _hip.load().swl_paged_attn_verify_max_tokens(h, kvh) == want


def test_baseline_is_accepted_and_an_empty_batch_is_ok():
    assert call() == LAUNCH
    assert call(num_seq_blocks=1, seq_block_size=1104, scratch=None) == LAUNCH       # one split: no scratch needed
    assert call(H=8, KVH=8, max_new_len=16, num_rows=20, q_tok_stride=1024, o_tok_stride=1024) == LAUNCH     # G = 1
    assert call(num_seqs=0) == OK and call(num_rows=0) == OK
    assert call(num_seqs=0, o=None, q=None, k_cache=None) == OK


@pytest.mark.parametrize("field", ["o", "q", "k_cache", "v_cache", "block_table", "seq_ids", "cu_seqlens", "ctx_lens",
                                   "row_lens", "scratch"])
def test_null_pointers_are_refused(field):
    assert call(**{field: None}) == BAD


@pytest.mark.parametrize("change", [
    dict(o=P + 8), dict(q=P + 2), dict(k_cache=P + 8), dict(v_cache=P + 4), dict(scratch=P + 8),     # 16-byte alignment
    dict(q_tok_stride=4100), dict(o_tok_stride=4092), dict(q_tok_stride=4088), dict(o_tok_stride=2048),
    dict(cur_layer=2), dict(cur_layer=-1), dict(L=0),
    dict(max_blocks_per_seq=68),                    # ceil(1100 / 16) = 69 entries of a table row are read
    dict(num_seq_blocks=4),                         # 4 x 256 keys do not cover 1100
    dict(seq_block_size=250, num_seq_blocks=5), dict(seq_block_size=0),
    dict(num_seqs=-1), dict(num_rows=-1), dict(num_rows=9), dict(max_new_len=0), dict(max_total_len=3),
    dict(H=30), dict(KVH=0), dict(dtype=7),
])
def test_bad_arguments_are_refused(change):
    assert call(**change) == BAD


@pytest.mark.parametrize("change", [
    dict(block_size=32), dict(block_size=8),
    dict(D=96, q_tok_stride=4096), dict(D=256, q_tok_stride=8192, o_tok_stride=8192), dict(D=16),
    dict(H=24, KVH=8), dict(H=32, KVH=2),           # G = 3, G = 16
    dict(max_new_len=5, num_rows=7),                # > 16 / G
    dict(H=16, KVH=2, max_new_len=3, num_rows=4),   # G = 8: two tokens at most
    dict(num_seqs=65536, num_rows=65535), dict(num_seqs=40000, num_rows=65536),
])
def test_unsupported_shapes_are_refused(change):
    assert call(**change) == UNSUP
