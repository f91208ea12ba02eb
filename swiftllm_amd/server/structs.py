"""Request bookkeeping shared by the scheduler, the engine and the HTTP layer.
Same names and fields as the reference's swiftllm/server/structs.py:4-63."""
import asyncio
import dataclasses
from typing import List, Optional

from swiftllm_amd.sampling_params import SamplingParams, TokenLogprob


@dataclasses.dataclass
class StepOutput:
    """One generated token of one request; `logprobs`: what a request that asks for them learns about it."""
    token_id: int
    request: "Request"
    logprobs: Optional[TokenLogprob] = None


class RawRequest:
    """What a user submits: a prompt and how many tokens to generate. `prompt_token_ids` may be given
    instead of text (tokenizer-less use: benchmarks, synthetic checkpoints). `sampling_params` (an addition to the
    reference): None or temperature 0 = greedy; its stop_token_ids end the request before output_len. `lora` (an addition):
    the name of a loaded LoRA adapter the request runs with, None = the base model."""

    def __init__(self, prompt: str, output_len: int, prompt_token_ids: Optional[List[int]] = None, *,
                 sampling_params: Optional[SamplingParams] = None, lora: Optional[str] = None):
        self.prompt = prompt
        self.output_len = output_len
        self.prompt_token_ids = prompt_token_ids
        self.sampling_params = sampling_params
        self.lora = lora


class Request:
    """A request inside the system: waiting, running (prefill or decode), swapped out, or finished."""

    def __init__(self, raw_request: RawRequest):
        self.prompt_token_ids: List[int] = list(raw_request.prompt_token_ids or [])
        self.prompt_len = len(self.prompt_token_ids)
        self.output_len = raw_request.output_len
        self.output_q: "asyncio.Queue[StepOutput]" = asyncio.Queue()    # streaming consumers read here
        self.finished_event = asyncio.Event()                           # non-streaming consumers wait here
        self.request_id = -1            # row of the block table, assigned when the request is admitted
        self.output_token_ids: List[int] = []
        # one TokenLogprob per output token, for a request whose sampling params ask for logprobs (empty otherwise)
        self.output_logprobs: List[TokenLogprob] = []
        self.error: Optional[str] = None    # set instead of scheduling when the request can never be served
        self.error_retryable = False        # ... for a reason that passes (a full guide store): HTTP 503 instead of 400
        self.aborted = False                # ended by the engine with `error` set after it had started: finished, whatever
                                            # it has generated (a guide that ran into a state in which no token is allowed)
        # guided decoding: the request's cursor through its guide (swiftllm_amd.guided.GuideCursor over a guide acquired when
        # the request was submitted; the engine advances it with every delivered token and releases the guide when the
        # request retires); None = not guided. Such a request is never speculated (its sampling params are not None)
        self.guide_cursor = None
        # multi-LoRA serving: the adapter every step of this request runs with (None = the base model); such a request is
        # never speculated
        self.lora: Optional[str] = getattr(raw_request, "lora", None)
        # None = greedy. A None seed is resolved here, once: the stream depends on (seed, position) only, so the request
        # draws the same tokens through preemption, swap-out and swap-in, in any batch, on any replica
        # (None also stands for params that ask for nothing — `plain`; a greedy request with penalties, a bias, min_tokens
        # or stop tokens keeps its params: the data plane processes its logits, and it is never speculated; so does one
        # that asks for logprobs: the data plane scores its tokens)
        sp = getattr(raw_request, "sampling_params", None)
        self.sampling_params: Optional[SamplingParams] = (None if sp is None or sp.plain else
                                                          sp if sp.greedy else sp.with_seed())
        # the request also ends at the first of these tokens (delivered as its last one) once it has generated more than
        # min_tokens tokens — before that the data plane bans them
        self._stop_ids = frozenset(sp.stop_token_ids) if sp is not None else frozenset()
        self._min_tokens = sp.min_tokens if sp is not None else 0

        # chunked prefill: prompt tokens whose KV is resident (forwarded in earlier steps), and the tokens the scheduler
        # gave this request in the step being built (0: not a prompt chunk / the whole rest of the prompt)
        self.num_prefilled = 0
        self.prefill_take = 0
        # speculative decoding: high-water mark of the tokens this request holds KV blocks for. A verify step stores its
        # drafts' K/V too; the blocks rejected drafts claimed stay with the request, and the scheduler counts them
        # (max(num_tokens, kv_reserved_tokens)). 0 = never verified: the arithmetic of always.
        self.kv_reserved_tokens = 0
        # ... and its prompt-lookup index (server/speculative.py: NgramProposer), built by the engine the first time the
        # request is a candidate for a verify step; None = never was
        self.ngram_proposer = None

    def is_finished(self) -> bool:
        out = self.output_token_ids
        if self.aborted or len(out) >= self.output_len:
            return True
        if bool(self._stop_ids) and len(out) > self._min_tokens and out[-1] in self._stop_ids:
            return True
        # a guided request also ends once nothing can follow what it has generated (its last token was delivered); one that
        # reaches output_len first is cut where it stands
        cur = self.guide_cursor
        return cur is not None and bool(out) and cur.complete

    def get_cur_output_len(self) -> int:
        return len(self.output_token_ids)

    def is_prefill_stage(self) -> bool:
        return not self.output_token_ids

    def is_prompt_resident(self) -> bool:
        """The whole prompt has been forwarded: the request decodes from here on. (`is_prefill_stage()` stays "no token
        generated yet", which is also true between the chunks of a chunked prefill.)"""
        return self.num_prefilled >= self.prompt_len or bool(self.output_token_ids)

    def num_tokens(self) -> int:
        """Tokens whose KV must be resident: the prompt plus everything generated so far."""
        return self.prompt_len + len(self.output_token_ids)
