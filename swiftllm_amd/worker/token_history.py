"""TokenHistory — which tokens a sequence has seen, kept on the host for the logits adjustment (csrc/logits_adjust.hip).

One entry per distinct token id: `ids[k]` and `meta[k]`, where bits 0..30 of `meta` count the token's occurrences among
the OUTPUT tokens and bit 31 says that it occurs in the PROMPT — the words the kernel reads. Updates are incremental:
O(1) per token through a dict from id to entry, numpy arrays that double when they fill up; nothing is rebuilt per step.
`row_entries` merges a history with a request's logit_bias and its min_tokens ban into the row's entries, one per id.
"""
import math
from typing import Iterable, Optional, Tuple

import numpy as np

from swiftllm_amd.sampling_params import SamplingParams

IN_PROMPT = np.int32(-2 ** 31)      # bit 31 of a meta word
COUNT_MASK = 0x7fffffff

_EMPTY_I = np.zeros(0, dtype=np.int32)
_EMPTY_F = np.zeros(0, dtype=np.float32)


class TokenHistory:
    __slots__ = ("ids", "meta", "size", "index", "num_prompt", "num_output")

    def __init__(self, capacity: int = 64):
        self.ids = np.zeros(max(capacity, 1), dtype=np.int32)
        self.meta = np.zeros(max(capacity, 1), dtype=np.int32)
        self.size = 0
        self.index = {}         # token id -> entry
        self.num_prompt = 0
        self.num_output = 0

    def __len__(self) -> int:
        """Tokens recorded: prompt tokens plus output tokens (what the sequence's length is held against)."""
        return self.num_prompt + self.num_output

    def _entry(self, tok: int) -> int:
        k = self.index.get(tok)
        if k is None:
            k = self.size
            if k == self.ids.size:
                self.ids = np.concatenate([self.ids, np.zeros_like(self.ids)])
                self.meta = np.concatenate([self.meta, np.zeros_like(self.meta)])
            self.ids[k] = tok
            self.meta[k] = 0
            self.index[tok] = k
            self.size = k + 1
        return k

    def add_prompt(self, tokens: Iterable[int], undo: Optional[list] = None):
        """`undo` (here and in add_output): a list that receives (entry, meta word before) per token, for `rollback`."""
        for tok in tokens:
            k = self._entry(int(tok))       # (may replace the arrays: looked up before `self.meta` is)
            if undo is not None:
                undo.append((k, int(self.meta[k])))
            self.meta[k] |= IN_PROMPT
            self.num_prompt += 1

    def add_output(self, tok: int, undo: Optional[list] = None):
        k = self._entry(int(tok))
        if (int(self.meta[k]) & COUNT_MASK) == COUNT_MASK:
            raise OverflowError("a token's output count passed 2**31 - 1")
        if undo is not None:
            undo.append((k, int(self.meta[k])))
        self.meta[k] += 1
        self.num_output += 1

    def mark(self) -> Tuple[int, int, int]:
        return self.size, self.num_prompt, self.num_output

    def rollback(self, mark: Tuple[int, int, int], undo: list):
        """Back to the state `mark()` described, given the `undo` records of every add since."""
        for k, word in reversed(undo):
            self.meta[k] = word
        for k in range(mark[0], self.size):
            del self.index[int(self.ids[k])]
        self.size, self.num_prompt, self.num_output = mark

    def entries(self) -> Tuple[np.ndarray, np.ndarray]:
        """Views of the live (ids, meta) entries, in first-seen order."""
        return self.ids[:self.size], self.meta[:self.size]


def row_entries(params: SamplingParams, hist: Optional[TokenHistory]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(ids int32, meta int32, bias float32) of one row, each id once: the history's tokens (only under a penalty: a bias
    alone needs none of them), the logit_bias entries, and a -inf bias on every stop token while the sequence has fewer
    than min_tokens output tokens. A biased or banned token the history knows keeps its meta word; another gets meta 0."""
    extra = {}
    if params.logit_bias is not None:
        extra.update(params.logit_bias)
    if params.stop_token_ids and (hist.num_output if hist is not None else 0) < params.min_tokens:
        for tok in params.stop_token_ids:
            extra[tok] = -math.inf
    if params.penalised and hist is not None and hist.size:
        ids, meta = hist.entries()
        bias = np.zeros(ids.size, dtype=np.float32)
        if not extra:
            return ids, meta, bias
        new = []
        for tok, b in extra.items():
            k = hist.index.get(tok)
            if k is None:
                new.append((tok, b))
            else:
                bias[k] = b
        if not new:
            return ids, meta, bias
        return (np.concatenate([ids, np.array([t for t, _ in new], dtype=np.int32)]),
                np.concatenate([meta, np.zeros(len(new), dtype=np.int32)]),
                np.concatenate([bias, np.array([b for _, b in new], dtype=np.float32)]))
    if not extra:
        return _EMPTY_I, _EMPTY_I, _EMPTY_F
    return (np.fromiter(extra.keys(), dtype=np.int32, count=len(extra)), np.zeros(len(extra), dtype=np.int32),
            np.fromiter(extra.values(), dtype=np.float32, count=len(extra)))
