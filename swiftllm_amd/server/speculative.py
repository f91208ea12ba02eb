"""Prompt-lookup speculative decoding: drafts come from the request's own prompt and output (no second model).

A verify step (LlamaModel.forward_verify) feeds a sequence's last accepted token followed by its drafts through ONE
forward and returns the greedy token after each of them; the longest prefix of drafts that equal the tokens before them
is kept, plus the token after it: between 1 and len(drafts) + 1 tokens per pass over the weights, and exactly the greedy
stream whatever the drafts were. The proposer costs nothing when it finds no match (the step is a plain decode step then).
"""
from typing import Dict, List, Sequence, Tuple

MAX_NGRAM = 3


class NgramProposer:
    """Per-request, incremental n-gram index over prompt + output.

    For n = 1..3 a dict maps an n-gram to the start of its most recent occurrence THAT HAS A SUCCESSOR: an n-gram is
    entered when the token after it is appended, so the current suffix is never its own match. Appending a token is
    O(1) (three dict stores), a proposal is at most three lookups and one slice: O(k), not O(history)."""

    __slots__ = ("tokens", "_index")

    def __init__(self, tokens: Sequence[int] = ()):
        self.tokens: List[int] = []
        self._index: Tuple[Dict[tuple, int], ...] = tuple({} for _ in range(MAX_NGRAM))
        self.extend(tokens)

    def __len__(self) -> int:
        return len(self.tokens)

    def append(self, token: int) -> None:
        toks = self.tokens
        end = len(toks)             # the n-grams that end at end - 1 gain their successor now
        for n in range(1, MAX_NGRAM + 1):
            if end >= n:
                self._index[n - 1][tuple(toks[end - n:end])] = end - n
        toks.append(int(token))

    def extend(self, tokens: Sequence[int]) -> None:
        for t in tokens:
            self.append(t)

    def sync(self, prompt: Sequence[int], output: Sequence[int]) -> None:
        """Bring the index up to prompt + output (both only ever grow)."""
        have = len(self.tokens)
        if have < len(prompt):
            self.extend(prompt[have:])
            have = len(prompt)
        self.extend(output[have - len(prompt):])

    def propose(self, k: int) -> List[int]:
        """Up to k draft tokens: n from 3 down to 1, the most recent earlier occurrence of the last n tokens, the tokens
        that followed it; the first n that matches decides. [] when nothing matches or k <= 0."""
        if k <= 0:
            return []
        toks = self.tokens
        size = len(toks)
        for n in range(min(MAX_NGRAM, size - 1), 0, -1):
            start = self._index[n - 1].get(tuple(toks[size - n:]))
            if start is not None:
                return toks[start + n:start + n + k]
        return []


def accept(drafts: Sequence[int], targets: Sequence[int]) -> int:
    """Length of the longest prefix with drafts[i] == targets[i]: targets[i] is the model's token after the i-th input
    of the verify step (the last accepted token, then the drafts), so draft i is right exactly when it equals it and
    every draft before it was right."""
    a = 0
    for d, t in zip(drafts, targets):
        if d != t:
            break
        a += 1
    return a
