"""The bytes each token id spells, for guided decoding. Read from a HuggingFace tokenizer.json with `json` alone."""
import json
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np


def _gpt2_byte_decoder() -> dict:
    """unicode character -> byte of the GPT-2 byte-level BPE alphabet (the published bytes_to_unicode table, inverted)."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xa1, 0xad)) + list(range(0xae, 0x100))
    chars = keep[:]
    n = 0
    for b in range(256):
        if b not in keep:
            keep.append(b)
            chars.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(keep, chars)}


_BYTE_DECODER = _gpt2_byte_decoder()
_BYTE_TOKEN = re.compile(r"^<0x([0-9A-Fa-f]{2})>$")


def _mentions_byte_level(node) -> bool:
    """A `ByteLevel` component anywhere in a pre_tokenizer / decoder description (they nest in Sequence objects)."""
    if isinstance(node, dict):
        return node.get("type") == "ByteLevel" or any(_mentions_byte_level(v) for v in node.values())
    if isinstance(node, list):
        return any(_mentions_byte_level(v) for v in node)
    return False


class TokenVocab:
    """`tokens[id]`: the bytes id spells; None or b"" marks an id a guide never allows (special tokens, ids the tokenizer
    does not define)."""

    def __init__(self, tokens: Sequence[Optional[bytes]]):
        out: List[Optional[bytes]] = []
        for i, t in enumerate(tokens):
            if t is not None and not isinstance(t, (bytes, bytearray)):
                raise TypeError(f"token {i}: expected bytes or None, got {type(t).__name__}")
            out.append(bytes(t) if t else None)
        if not out:
            raise ValueError("an empty vocabulary")
        self.tokens = out
        self._flat = None

    def __len__(self) -> int:
        return len(self.tokens)

    def token_bytes(self, token_id: int) -> Optional[bytes]:
        return self.tokens[token_id] if 0 <= token_id < len(self.tokens) else None

    def flat(self) -> Tuple[np.ndarray, np.ndarray]:
        """(bytes: uint8 [total], offsets: int32 [V + 1]); token t spells bytes[offsets[t]:offsets[t + 1]]."""
        if self._flat is None:
            lens = np.fromiter((len(t) if t else 0 for t in self.tokens), dtype=np.int64, count=len(self.tokens))
            offsets = np.zeros(len(self.tokens) + 1, dtype=np.int64)
            np.cumsum(lens, out=offsets[1:])
            if int(offsets[-1]) >= 2 ** 31:
                raise ValueError("the vocabulary spells more than 2**31 bytes")
            data = np.frombuffer(b"".join(t for t in self.tokens if t), dtype=np.uint8).copy()
            self._flat = (data, offsets.astype(np.int32))
        return self._flat

    @classmethod
    def from_tokenizer_json(cls, path: str, vocab_size: int) -> "TokenVocab":
        """Byte-level BPE (a ByteLevel pre-tokenizer or decoder) is inverted with the GPT-2 byte <-> unicode table; any other
        vocabulary is read SentencePiece-style: `▁` is a space, `<0xHH>` is byte HH, the rest its UTF-8. `added_tokens`
        marked special become None, and so do the ids in [len, vocab_size)."""
        with open(path, encoding="utf-8") as f:
            spec = json.load(f)
        model = spec.get("model") or {}
        vocab = model.get("vocab")
        if isinstance(vocab, list):         # (Unigram: [[piece, score], ...])
            vocab = {entry[0]: i for i, entry in enumerate(vocab)}
        if not isinstance(vocab, dict) or not vocab:
            raise ValueError(f"{path}: no model.vocab")
        byte_level = _mentions_byte_level(spec.get("pre_tokenizer")) or _mentions_byte_level(spec.get("decoder"))
        added = spec.get("added_tokens") or []
        top = max([int(i) for i in vocab.values()] + [int(a["id"]) for a in added if "id" in a])
        if top >= vocab_size:
            raise ValueError(f"{path}: token id {top} does not fit a vocabulary of {vocab_size}")
        tokens: List[Optional[bytes]] = [None] * vocab_size

        def spell(piece: str) -> Optional[bytes]:
            if byte_level:
                try:
                    return bytes(_BYTE_DECODER[ch] for ch in piece)
                except KeyError:
                    return None             # (not in the byte alphabet: no byte-level token)
            m = _BYTE_TOKEN.match(piece)
            if m:
                return bytes([int(m.group(1), 16)])
            return piece.replace("▁", " ").encode("utf-8")

        for piece, i in vocab.items():
            tokens[int(i)] = spell(piece)
        for a in added:
            if "id" not in a:
                continue
            # (an added token's content is literal text, never byte-alphabet text)
            tokens[int(a["id"])] = None if a.get("special") else str(a.get("content", "")).encode("utf-8")
        return cls(tokens)
