"""SamplingParams — how one sequence picks its next token.

The reference samples greedily only (swiftllm/worker/layers/post_layer.py:40); greedy stays the default here. A
sampled request draws from softmax(logits / temperature), optionally restricted to the `top_k` largest logits and
then to the smallest nucleus holding `top_p` of the remaining mass. The draw is seeded: the same (seed, position)
gives the same token whatever batch, row, graph bucket or replica serves it (csrc/sampling.hip has the contract).
"""
import dataclasses
import math
import secrets
from typing import Optional


@dataclasses.dataclass(frozen=True)
class SamplingParams:
    temperature: float = 0.0    # 0: greedy (argmax), the reference's behaviour
    top_k: int = 0              # 0: off
    top_p: float = 1.0          # 1: off
    seed: Optional[int] = None  # None: a fresh 64-bit seed is drawn when the request (or forward call) takes it

    def __post_init__(self):
        t = self.temperature
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or t < 0:
            raise ValueError(f"temperature must be a finite number >= 0, got {t!r}")
        k = self.top_k
        if isinstance(k, bool) or not isinstance(k, int) or k < 0 or k >= 2 ** 31:
            raise ValueError(f"top_k must be an integer >= 0, got {k!r}")
        p = self.top_p
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 < p <= 1.0):
            raise ValueError(f"top_p must be a number in (0, 1], got {p!r}")
        s = self.seed
        if s is not None and (isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < 2 ** 64):
            raise ValueError(f"seed must be an integer in [0, 2**64), got {s!r}")

    @property
    def greedy(self) -> bool:
        return self.temperature == 0

    def with_seed(self) -> "SamplingParams":
        """These parameters with a concrete seed (a fresh one drawn when `seed` is None)."""
        return self if self.seed is not None else dataclasses.replace(self, seed=secrets.randbits(64))


def is_greedy(params: Optional[SamplingParams]) -> bool:
    return params is None or params.greedy
