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
        return self.forward_normed(last_input, logits=infer_state.logits)

    def forward_normed(self, last_input: torch.Tensor, out: torch.Tensor = None, logits=None) -> torch.Tensor:
        """lm_head + sampling on rows that already went through the final norm (a pure-decode batch whose
        last add + norm ran fused on the split-K partials of the last down projection: every row is a last token).
        `logits`: the step's worker/step_logits.LogitsArgs, each field None for no launch, or None for a plain step (argmax
        of the raw logits). mask -> adjust -> pick -> logprobs: `guide` turns every guided row's disallowed tokens into -inf
        before anything else reads the logits (so min-p takes its maximum over the allowed tokens and logprobs are the
        distribution over them); `adjust` applies penalties, bias and min-p in place (the tap shows what the token was
        picked from); `sampling` draws where a row is not greedy; `logprobs` scores the picked tokens on the same logits."""
        guide, adjust, sampling, logprobs = logits or (None,) * 4
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
