"""swiftllm_amd/guided/vocab.py: the bytes each id spells, read from synthetic tokenizer.json files in both forms."""
import json

import numpy as np
import pytest

from swiftllm_amd.guided import TokenVocab
from swiftllm_amd.guided.vocab import _gpt2_byte_decoder


def gpt2_bytes_to_unicode() -> dict:
    """The published GPT-2 table, written out independently of the code under test: printable Latin-1 bytes stand for
    themselves, the 68 others take the code points from 256 up in byte order."""
    printable = [b for b in range(256) if 33 <= b <= 126 or 161 <= b <= 172 or 174 <= b <= 255]
    table, n = {}, 0
    for b in range(256):
        if b in printable:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + n)
            n += 1
    assert n == 68
    return table


def write(tmp_path, spec) -> str:
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(spec, ensure_ascii=False), encoding="utf-8")
    return str(path)


def test_byte_level_bpe_covers_all_256_bytes(tmp_path):
    enc = gpt2_bytes_to_unicode()
    assert enc[ord("A")] == "A" and enc[0x20] == "Ġ" and enc[0x0a] == "Ċ"     # the table's well-known entries
    assert {b: c for c, b in _gpt2_byte_decoder().items()} == enc
    vocab = {enc[b]: b for b in range(256)}
    vocab["Ġhello"] = 256
    vocab[enc[0xc3] + enc[0xa9]] = 257                   # 'é' as its two bytes
    vocab[enc[0xe2] + enc[0x82]] = 258                   # two thirds of '€': no valid UTF-8, still bytes
    spec = {"model": {"type": "BPE", "vocab": vocab},
            "pre_tokenizer": {"type": "Sequence", "pretokenizers": [{"type": "Split"}, {"type": "ByteLevel"}]},
            "decoder": {"type": "ByteLevel"},
            "added_tokens": [{"id": 259, "content": "<|begin_of_text|>", "special": True},
                             {"id": 260, "content": "<tool>", "special": False}]}
    v = TokenVocab.from_tokenizer_json(write(tmp_path, spec), 264)
    assert len(v) == 264
    for b in range(256):
        assert v.tokens[b] == bytes([b])
    assert v.tokens[256] == b" hello" and v.tokens[257] == "é".encode() and v.tokens[258] == b"\xe2\x82"
    assert v.tokens[259] is None                         # special
    assert v.tokens[260] == b"<tool>"                    # added, not special: literal text
    assert v.tokens[261:] == [None, None, None]          # ids the file does not define
    assert v.token_bytes(256) == b" hello" and v.token_bytes(-1) is None and v.token_bytes(264) is None


def test_byte_level_is_recognised_by_the_decoder_alone(tmp_path):
    enc = gpt2_bytes_to_unicode()
    spec = {"model": {"vocab": {enc[0x20] + "a": 0, "b": 1}}, "pre_tokenizer": None, "decoder": {"type": "ByteLevel"}}
    assert TokenVocab.from_tokenizer_json(write(tmp_path, spec), 2).tokens == [b" a", b"b"]


def test_sentencepiece_style_vocabulary(tmp_path):
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2, "<0x0A>": 3, "<0xFF>": 4, "▁the": 5, "▁": 6, "é": 7, "a▁b": 8, "<0xZZ>": 9}
    spec = {"model": {"type": "BPE", "vocab": vocab}, "pre_tokenizer": None,
            "decoder": {"type": "Sequence", "decoders": [{"type": "Replace"}, {"type": "ByteFallback"}, {"type": "Fuse"}]},
            "added_tokens": [{"id": 0, "content": "<unk>", "special": True}, {"id": 1, "content": "<s>", "special": True},
                             {"id": 2, "content": "</s>", "special": True}]}
    v = TokenVocab.from_tokenizer_json(write(tmp_path, spec), 12)
    assert v.tokens[:3] == [None, None, None]
    assert v.tokens[3] == b"\n" and v.tokens[4] == b"\xff"
    assert v.tokens[5] == b" the" and v.tokens[6] == b" " and v.tokens[7] == "é".encode() and v.tokens[8] == b"a b"
    assert v.tokens[9] == b"<0xZZ>"                      # not a byte token: its text
    assert v.tokens[10:] == [None, None]


def test_unigram_vocab_lists_and_a_vocab_size_that_is_too_small(tmp_path):
    spec = {"model": {"type": "Unigram", "vocab": [["<unk>", 0.0], ["▁a", -1.0], ["<0x41>", -2.0]]}}
    path = write(tmp_path, spec)
    assert TokenVocab.from_tokenizer_json(path, 4).tokens == [b"<unk>", b" a", b"A", None]
    with pytest.raises(ValueError, match="does not fit"):
        TokenVocab.from_tokenizer_json(path, 2)
    with pytest.raises(ValueError, match="no model.vocab"):
        TokenVocab.from_tokenizer_json(write(tmp_path, {"model": {}}), 4)


def test_flat_form():
    v = TokenVocab([b"ab", None, b"", b"\xff", b"cde"])
    assert v.tokens == [b"ab", None, None, b"\xff", b"cde"]
    data, offsets = v.flat()
    assert data.dtype == np.uint8 and offsets.dtype == np.int32
    assert data.tobytes() == b"ab\xffcde" and offsets.tolist() == [0, 2, 2, 2, 3, 6]
    assert v.flat()[0] is data                           # computed once
    with pytest.raises(TypeError):
        TokenVocab(["ab"])
    with pytest.raises(ValueError):
        TokenVocab([])
