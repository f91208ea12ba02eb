"""Final norm, lm_head and sampling (greedy, or seeded when the step is sampled). Reference:
swiftllm/worker/layers/post_layer.py:9-40."""
import torch

from ..kernels.rmsnorm import rmsnorm_inplace
from ..kernels.linear import linear
from ..kernels.guided import mask_logits
from ..kernels.logits_process import adjust_logits
from ..kernels.logprobs import token_logprobs
from ..kernels.sampling import argmax_rows, sample_rows


class LlamaPostLayer:
    def __init__(self, model_config, weights):
        self.model_config = model_config
        self.weights = weights
        self.skinny = False     # set by LlamaModel from EngineConfig.use_skinny_gemm
        # tests set this to a list: every forward appends its pre-argmax logits (the DEVICE tensor — no
        # host copy here, a forward may be under hipGraph capture; LlamaModel appends a copy after each replay)
        self.logits_tap = None
        self.last_logits = None     # the logits tensor of the most recent (eager or captured) forward

    def forward(self, input_embds: torch.Tensor, infer_state) -> torch.Tensor:
        """[num_tokens, hidden] -> next-token ids int64 [batch_size] (argmax; ties -> lowest id)."""
        idx = infer_state.last_token_indices
        if idx is None:
            # the last token of each prefill sequence, then every decoding token
            idx = torch.cat((
                infer_state.prefill_seq_start_locs + infer_state.prefill_seq_lens - 1,
                torch.arange(infer_state.num_prefill_tokens, infer_state.num_tokens,
                             device=input_embds.device, dtype=torch.int32)))
        last_input = input_embds.index_select(0, idx)    # fresh [batch, hidden] copy
        rmsnorm_inplace(last_input, self.weights.final_norm, self.model_config.rms_norm_eps)
        return self.forward_normed(last_input, sampling=infer_state.sampling, adjust=infer_state.adjust,
                                   logprobs=infer_state.logprobs, guide=infer_state.guide)

    def forward_normed(self, last_input: torch.Tensor, out: torch.Tensor = None, sampling=None,
                       adjust=None, logprobs=None, guide=None) -> torch.Tensor:
        """lm_head + sampling on rows that already went through the final norm (a pure-decode batch whose
        last add + norm ran fused on the split-K partials of the last down projection: every row is a last token).
        `sampling`: the step's kernels/sampling.SampleArgs, or None for an all-greedy step (argmax, as before).
        `adjust`: the step's kernels/logits_process.AdjustArgs — penalties, bias and min-p are applied to the logits in
        place before the token is picked (the tap then shows what it was picked from) — or None: no launch.
        `logprobs`: the step's kernels/logprobs.LogprobArgs — once the tokens are picked, the asking rows' log-probability,
        rank and top-N alternatives are written into its buffers, from the same logits — or None: no launch.
        `guide`: the step's kernels/guided.GuideArgs — every guided row's disallowed tokens become -inf before anything
        else reads the logits (mask -> adjust -> pick -> logprobs: min-p takes its maximum over the allowed tokens, the tap
        shows what the token was picked from, logprobs are the distribution over the allowed tokens) — or None: no launch."""
        logits = linear(last_input, self.weights.lm_head, self.skinny)   # [batch, vocab]
        if guide is not None:
            mask_logits(logits, guide)
        if adjust is not None:
            adjust_logits(logits, adjust)
        self.last_logits = logits
        if self.logits_tap is not None:
            self.logits_tap.append(logits)
        if sampling is not None:
            tokens = sample_rows(logits, sampling, None, out)
        else:
            tokens = argmax_rows(logits, out)
        if logprobs is not None:
            token_logprobs(logits, tokens, logprobs)
        return tokens
