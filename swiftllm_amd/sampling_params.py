"""SamplingParams — how one sequence picks its next token.

The reference samples greedily only (swiftllm/worker/layers/post_layer.py:40); greedy stays the default here. A
sampled request draws from softmax(logits / temperature), optionally restricted to the `top_k` largest logits and
then to the smallest nucleus holding `top_p` of the remaining mass. The draw is seeded: the same (seed, position)
gives the same token whatever batch, row, graph bucket or replica serves it (csrc/sampling.hip has the contract).

Before the token is picked, greedily or not, the logits can be edited (csrc/logits_adjust.hip has the contract): a
repetition penalty (tokens seen in the prompt or the output: positive logits divided, the others multiplied), a presence
and a frequency penalty (output tokens only), an additive `logit_bias` per token id, and `min_p` (tokens whose
probability is below `min_p` times the largest one are removed before top-k / top-p act). `stop_token_ids` end the
request at the first of them (delivered as its last token); while fewer than `min_tokens` tokens have been generated the
stop tokens cannot be picked.

`logprobs` = N (0..20) asks for the log-probability and the rank of every generated token and for the N most likely
tokens at its position (csrc/logprobs.hip has the contract): the model's distribution at temperature 1 over the logits
as they stand when the token is picked — after the edits above, before temperature / top-k / top-p, which do not
renormalise it. It changes no token.

`guided_regex`, `guided_choice` and `allowed_token_ids` (at most one of them) hold the output to a shape: the bytes the
generated tokens spell fullmatch the regex (the byte-level subset of swiftllm_amd/guided/regex.py), are one of the choices,
or every token is one of the ids. Before anything else reads the logits, the tokens the request's state does not allow
become -inf (csrc/guided.hip), so min-p, the pickers and logprobs see the allowed tokens only. The request's
`stop_token_ids` are its end ids: allowed exactly where the text so far is a full match. A regex / choice request ends at
such a stop token, or — without one — as soon as nothing can follow (its last token is delivered); one that reaches
`output_len` first is cut where it stands, mid-pattern; one whose guide reaches a state in which the vocabulary offers no
token (no token spells the bytes needed there, or only a stop id does) ends there with an error. `min_tokens` cannot be combined with a guide: a state in which
only the end ids are left would have nothing to pick.
"""
import dataclasses
import math
import secrets
from typing import NamedTuple, Optional, Tuple

MAX_LOGPROBS = 20   # alternatives a token can report (the kernel's LDS-ordered survivors)


class TokenLogprob(NamedTuple):
    """What a request that asks for logprobs learns about one generated token."""
    token_id: int
    logprob: float      # NaN when the row's maximum is not finite
    rank: int           # 1 = the most likely token (ties: the lowest id first)
    top: Tuple[Tuple[int, float], ...] = ()     # the N most likely (id, logprob), in order


@dataclasses.dataclass(frozen=True)
class SamplingParams:
    temperature: float = 0.0    # 0: greedy (argmax), the reference's behaviour
    top_k: int = 0              # 0: off
    top_p: float = 1.0          # 1: off
    seed: Optional[int] = None  # None: a fresh 64-bit seed is drawn when the request (or forward call) takes it
    repetition_penalty: float = 1.0     # 1: off
    presence_penalty: float = 0.0       # 0: off
    frequency_penalty: float = 0.0      # 0: off
    min_p: float = 0.0                  # 0: off
    logit_bias: Optional[Tuple[Tuple[int, float], ...]] = None  # a mapping / pairs id -> bias; stored as sorted pairs
    stop_token_ids: Tuple[int, ...] = ()
    min_tokens: int = 0                 # stop tokens are banned while fewer output tokens exist
    logprobs: Optional[int] = None      # None: off; N in 0..20: every generated token reports itself and its top N
    guided_regex: Optional[str] = None                  # the output's bytes fullmatch this pattern
    guided_choice: Optional[Tuple[str, ...]] = None     # ... or are one of these strings
    allowed_token_ids: Optional[Tuple[int, ...]] = None     # ... or every token is one of these ids; stored sorted, unique

    def __post_init__(self):
        self._check_sampling()
        self._check_processing()
        n = self.logprobs
        if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MAX_LOGPROBS):
            raise ValueError(f"logprobs must be None or an integer in [0, {MAX_LOGPROBS}], got {n!r}")
        self._check_guided()

    def _check_guided(self):
        """Shapes only: the pattern itself is compiled when the request is submitted (swiftllm_amd/guided)."""
        r, c, a = self.guided_regex, self.guided_choice, self.allowed_token_ids
        if sum(v is not None for v in (r, c, a)) > 1:
            raise ValueError("at most one of guided_regex, guided_choice and allowed_token_ids may be set")
        if r is not None and not isinstance(r, str):
            raise ValueError(f"guided_regex must be a string, got {r!r}")
        if c is not None:
            if isinstance(c, (str, bytes)) or not hasattr(c, "__iter__"):
                raise ValueError(f"guided_choice must be a sequence of strings, got {c!r}")
            c = tuple(c)
            if not c or any(not isinstance(s, str) or s == "" for s in c):
                raise ValueError(f"guided_choice must name at least one choice, each a non-empty string, got {c!r}")
            if len(set(c)) != len(c):
                raise ValueError(f"guided_choice names a choice twice: {c!r}")
            object.__setattr__(self, "guided_choice", c)
        if a is not None:
            if isinstance(a, (str, bytes)) or not hasattr(a, "__iter__"):
                raise ValueError(f"allowed_token_ids must be a sequence of integers, got {a!r}")
            a = tuple(a)
            if not a or any(isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < 2 ** 31 for t in a):
                raise ValueError(f"allowed_token_ids must name at least one integer in [0, 2**31), got {a!r}")
            object.__setattr__(self, "allowed_token_ids", tuple(sorted(set(a))))
        if self.guided and self.min_tokens > 0:
            raise ValueError("min_tokens > 0 cannot be combined with a guide: a state in which only the end ids are allowed "
                             "would have nothing left to pick")

    def _check_processing(self):
        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float))
        r = self.repetition_penalty
        if not number(r) or not math.isfinite(r) or r <= 0:
            raise ValueError(f"repetition_penalty must be a finite number > 0, got {r!r}")
        for name in ("presence_penalty", "frequency_penalty"):
            v = getattr(self, name)
            if not number(v) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        p = self.min_p
        if not number(p) or not 0.0 <= p < 1.0:
            raise ValueError(f"min_p must be a number in [0, 1), got {p!r}")
        bias = self.logit_bias
        if bias is not None:
            try:
                pairs = list(bias.items()) if hasattr(bias, "items") else [tuple(kv) for kv in bias]
            except TypeError:
                raise ValueError(f"logit_bias must be a mapping or pairs of id -> bias, got {bias!r}") from None
            out = {}
            for kv in pairs:
                if len(kv) != 2:
                    raise ValueError(f"logit_bias entries are (id, bias) pairs, got {kv!r}")
                tok, b = kv
                if isinstance(tok, bool) or not isinstance(tok, int) or not 0 <= tok < 2 ** 31:
                    raise ValueError(f"logit_bias ids must be integers in [0, 2**31), got {tok!r}")
                if not number(b) or math.isnan(b) or b == math.inf:
                    raise ValueError(f"logit_bias values must be finite or -inf, got {b!r}")
                if tok in out:
                    raise ValueError(f"logit_bias names id {tok} twice")
                out[tok] = float(b)
            object.__setattr__(self, "logit_bias", tuple(sorted(out.items())) or None)
        stops = self.stop_token_ids
        if isinstance(stops, (str, bytes)) or not hasattr(stops, "__iter__"):
            raise ValueError(f"stop_token_ids must be a sequence of integers, got {stops!r}")
        stops = tuple(stops)
        if any(isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < 2 ** 31 for t in stops):
            raise ValueError(f"stop_token_ids must be integers in [0, 2**31), got {stops!r}")
        object.__setattr__(self, "stop_token_ids", stops)
        n = self.min_tokens
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(f"min_tokens must be an integer >= 0, got {n!r}")

    def _check_sampling(self):
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

    @property
    def penalised(self) -> bool:
        """Some penalty is on: the row's entries include the tokens of its sequence."""
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0

    @property
    def processes_logits(self) -> bool:
        """The logits of this request are edited before its token is picked (by a step, or by some step)."""
        return (self.penalised or self.min_p != 0.0 or self.logit_bias is not None
                or (self.min_tokens > 0 and bool(self.stop_token_ids)))

    @property
    def guided(self) -> bool:
        """The output is held to a regex, a choice or a set of token ids (it needs no token history: `processes_logits`
        does not depend on it)."""
        return self.guided_regex is not None or self.guided_choice is not None or self.allowed_token_ids is not None

    def guide_spec(self):
        """(kind, spec) for swiftllm_amd.guided.guide_key, or None."""
        if self.guided_regex is not None:
            return "regex", self.guided_regex
        if self.guided_choice is not None:
            return "choice", self.guided_choice
        if self.allowed_token_ids is not None:
            return "tokens", self.allowed_token_ids
        return None

    @property
    def plain(self) -> bool:
        """Nothing to do beyond the argmax of the raw logits, run to output_len: what None means."""
        return (self.greedy and not self.processes_logits and not self.stop_token_ids and self.logprobs is None
                and not self.guided)

    def min_p_gap(self) -> float:
        """What the kernel compares x_i - max(x) with: T * ln(min_p), computed in double precision (the caller rounds it
        to fp32); -inf when min-p is off or the row is greedy (T == 0: the argmax survives any min_p)."""
        if self.min_p <= 0.0 or self.temperature <= 0.0:
            return -math.inf
        return float(self.temperature) * math.log(self.min_p)

    def with_seed(self) -> "SamplingParams":
        """These parameters with a concrete seed (a fresh one drawn when `seed` is None)."""
        return self if self.seed is not None else dataclasses.replace(self, seed=secrets.randbits(64))


def is_greedy(params: Optional[SamplingParams]) -> bool:
    return params is None or params.greedy
