"""One LLaMA transformer block on the gfx950 operators.

Operator order and buffer aliasing follow swiftllm/worker/layers/transformer_layer.py:31-130: residual-add + attention
norm, q/k/v projections, rotary, KV store, attention, output projection, residual-add + FFN norm, up/gate projection,
SiLU-gate, down projection. Which kernels carry that sequence is decided ONCE per (layer, step shape) by `decide_route`, a
pure function of the layer's static facts (`LayerFacts`) and the step's facts (`StepFacts`); `forward` looks the
`LayerRoute` up and runs one body per stage. `forward` returns, and accepts, a tensor, the down projection's split-K slabs
(SplitKPartials) or a RawResidual marker (the down projection already added itself into the residual buffer). Why each
form exists and what it buys is in DESIGN.md sections 4.4-4.9, 4.11 and 4.14.

Launches per layer by route (pure decode of m sequences unless said; default switches; "slabs" = fp32 split-K partials):

| route (o_proj / FFN, down)        | when                                             | launches                                      |
|-----------------------------------|--------------------------------------------------|-----------------------------------------------|
| ROWS_NF, ROWS                     | bfloat16, m <= 16                                | qkv_nf, attention(qkv slabs), o_rows, silu_gate_nf, down_rows: 5 |
| ROWS_NF, SPLITK                   | bfloat16, 17 <= m <= 32                          | add_scale, qkv, attention(qkv slabs), o_rows, silu_gate_nf, down: 6 |
| ROWS_NX, ROWS_SSQ                 | float16 (or defer_rmsnorm off), m <= 16          | qkv_nx, attention(qkv slabs), o_rows_ssq, silu_gate_nx, down_rows_ssq: 5 |
| ROWS_NX, SPLITK                   | float16 (or defer_rmsnorm off), 17 <= m <= 32    | add_norm, qkv, attention(qkv slabs), o_rows_ssq, silu_gate_nx, down: 6 |
| TINY, SPLITK                      | bfloat16, m <= 2, rows not taken, slabs handed on | qkv_from_slabs, attention(qkv slabs), o (or o_from_attention_partials), silu_gate_from_slabs, down: 5 |
| SPLITK_DEFERRED, SPLITK           | bfloat16, m <= 32, rows not taken                | add_scale, qkv, attention(qkv slabs), o, add_scale, silu_gate_rs, down: 7 |
| SPLITK_FUSED, SPLITK              | 33 <= m <= 256 (or float16 without rows)         | add_norm, qkv, attention(qkv slabs), o, add_norm, silu_gate, down: 7 |
| ... with QKV.SLABS_ROTARY         | fuse_rope_into_attention off (or head_dim, m > 256) | ... qkv, rotary+store(qkv slabs), attention ... |
| PLAIN, PLAIN, QKV.FUSED_DECODE    | fuse_splitk_consumers or use_skinny_gemm off     | add_norm, q/k/v, rotary+store, attention, o, add_norm, up_gate (+ silu), down |
| PLAIN, PLAIN, QKV.FUSED_PREFILL   | a prompt row in the batch                        | the same with the prompt rotary+store and prefill attention (riding decodes on the side stream) |
| PLAIN, PLAIN, QKV.ROTARY_THEN_STORE | FP8 pools, fuse_rope_kvstore off, no positions | ... rotary, (quantising) store ... (QKV.ROTARY_ONLY: ignore_kvcache) |
| SPLITK_FUSED (or _DEFERRED), SPLITK, QKV.ROTARY_THEN_STORE | plain_qkv (Qwen2 / Qwen3 / q_size != hidden)          | add_norm, qkv, prep, store, attention, o, add_norm (or add_scale), silu_gate, down: 9 (as FP8 pools) |
| PLAIN, PLAIN, QKV.ROTARY_THEN_STORE | plain_qkv, a prompt row (or the switches above off) | add_norm, q/k/v, prep, store, attention, o, add_norm, up_gate (+ silu), down |
| SPLITK_FUSED (or PLAIN), MOE      | a mixture-of-experts layer (Qwen3-MoE, Mixtral)  | ... o, add_norm, router, route, align, up_gate_silu, down, combine (prompt steps: the six MoE launches per block of tokens) |
| lora                              | some row names an adapter                        | the plain sequence with the adapter update after every projection |

"prep" is the one launch between the projections and the store: bias + per-head QK-norm + rotary (swl_qk_prep_rotary) for
a model with a q/k/v bias or a QK-norm, swl_rotary for one that only decouples q_size from hidden (Mistral-Nemo).
A mixture-of-experts layer ends the o_proj / FFN-norm stage with the normalised activations as a tensor, computes the router
logits with the dense `linear()` on the [E, H] router weight, and hands a plain tensor to the next layer (kernels/moe.py).
The first layer of a step receives a tensor, so its input norm is the fused add+norm whatever the route of the others.
"""
import enum
from typing import NamedTuple

import torch

from swiftllm_amd import _hip
from ..kernels.linear import (RawResidual, SplitKPartials, _TINY_MAX_KC, _TINY_POLICY_M as TINY_POLICY_M, alt_residual_like,
                              linear, linear_rows_add, linear_silu_gate, linear_silu_gate_from_splitk, linear_silu_gate_nf,
                              linear_silu_gate_nx, linear_splitk, linear_splitk_from_attn_partials,
                              linear_splitk_from_splitk, linear_splitk_nf, linear_splitk_nx)
from ..kernels.rmsnorm import (RowScalePending, add_scale_from_splitk, deferred_norm_ok, fused_add_rmsnorm_inplace,
                               fused_add_rmsnorm_from_splitk)
from ..kernels.rotary_emb import (qk_prep_rotary_inplace, rotary_embedding_inplace, rotary_embedding_and_store_kvcache_decode,
                                  rotary_embedding_and_store_kvcache_decode_from_splitk,
                                  rotary_embedding_and_store_kvcache_prefill)
from ..kernels.kvcache_mgmt import store_kvcache
from ..kernels.prefill_attn import prefill_attention, prefill_attention_paged
from ..kernels.paged_attn import paged_attention, paged_attention_from_qkv_splitk, paged_attention_verify
from ..kernels.silu_and_mul import silu_and_mul_inplace
from ..kernels.lora import lora_apply
from ..kernels.moe import moe_ffn

# Where the row-owned projections win on MI355X (tools/gemm_rows_micro.py --layer, tools/rows_kernel_us.py): every
# workgroup of such a projection pulls ALL of x through its own L1, so the win shrinks with the batch. With x staged as
# full lines through LDS (r06b, csrc/gemm_rows.hip) o_proj (x = M x 8 KiB) beats the split-K pair at 32 sequences by
# ~4 us (10.5 vs 9.6 + 5), down_proj (x = M x 28 KiB) wins by ~3 us at 16 (23.8 vs 20.5 + 5; layer chain 83.1 vs 86.3),
# ties at 24 and loses at 32 (28.4 vs 21.4 + 5) — profiles/r06b_rows_ab.jsonl, r06b_rows_kernel_us.jsonl. (r05: 8.)
ROWS_O_MAX_M = 32
ROWS_DOWN_MAX_M = 16


# ---- the values a LayerRoute is made of ---------------------------------------------------------------------------------
# Input: what the previous layer (or the embedding) hands to `forward`
#   TENSOR   activations: the embedding, or a projection that came back whole
#   SLABS    the previous down projection's split-K slabs
#   RAW      RawResidual: the previous down projection is already in the residual buffer
#   RAW_SSQ  ... with the rows' per-tile sums of squares
# AttnNorm: how the layer's input is normalised for attention
#   FUSED          residual add + norm in one launch (in place, or from slabs)
#   SCALE_PENDING  element-wise add + scale; the 1/rms is applied by the attention prologue
#   TINY           the qkv projection sums the slabs itself; 1/rms pending
#   RAW_NF         the qkv projection normalises the raw residual rows; 1/rms pending
#   RAW_NX         ... exactly, from the rows' sums of squares
# QKV: how q/k/v reach attention
#   SLABS_ATTN         fused qkv slabs -> rotary + KV store + paged attention in one launch
#   SLABS_ROTARY       fused qkv slabs -> rotary + KV store in one launch
#   FUSED_DECODE       projections, then rotary + KV store in one launch (decode tokens)
#   FUSED_PREFILL      ... (prompt tokens, one pass over k; riding decodes: their fused launch)
#   ROTARY_THEN_STORE  rotary, then the store (the quantising one with FP8 pools)
#   ROTARY_ONLY        ignore_kvcache: nothing is stored
# Attn: which attention serves the step's rows (riding decodes: paged attention on the side stream)
#   DECODE  paged attention
#   FRESH   whole prompts attend to their fresh projections
#   PAGED   prompt chunks behind a resident context attend to the pool
#   VERIFY  the rows of a speculative-decoding verify step
# OFfn: o_proj + FFN norm + up/gate
#   ROWS_NF          o_proj adds itself into the residual; the SiLU-gate GEMM normalises the raw rows (1/rms deferred)
#   ROWS_NX          ... with the reference's rounding points, from the rows' sums of squares
#   TINY             o_proj slabs (route.merge: from the flash-decoding partials) summed by the SiLU-gate GEMM
#   SPLITK_DEFERRED  o_proj slabs -> add + scale -> SiLU-gate GEMM applying the 1/rms
#   SPLITK_FUSED     o_proj slabs -> fused add + norm -> SiLU-gate GEMM
#   PLAIN            the reference sequence
# Down: the down projection
#   ROWS      adds itself into the residual: the layer returns a RawResidual
#   ROWS_SSQ  ... carrying the rows' sums of squares
#   SPLITK    slabs where the kernel splits K
#   PLAIN     a tensor
#   MOE       the mixture-of-experts FFN took the place of up/gate and down: a tensor
Input = enum.Enum("Input", "TENSOR SLABS RAW RAW_SSQ")
AttnNorm = enum.Enum("AttnNorm", "FUSED SCALE_PENDING TINY RAW_NF RAW_NX")
QKV = enum.Enum("QKV", "SLABS_ATTN SLABS_ROTARY FUSED_DECODE FUSED_PREFILL ROTARY_THEN_STORE ROTARY_ONLY")
Attn = enum.Enum("Attn", "DECODE FRESH PAGED VERIFY")
OFfn = enum.Enum("OFfn", "ROWS_NF ROWS_NX TINY SPLITK_DEFERRED SPLITK_FUSED PLAIN")
Down = enum.Enum("Down", "ROWS ROWS_SSQ SPLITK PLAIN MOE")


class LayerRoute(NamedTuple):
    attn_norm: AttnNorm
    qkv: QKV
    attention: Attn
    piggyback: bool             # decode rows ride along with prompt rows: their attention runs on the side stream
    merge: bool                 # a split flash-decoding is merged by o_proj (phase 1 only + linear_splitk_from_attn_partials)
    o_ffn: OFfn
    down: Down
    lora: bool                  # the LoRA body: plain operators, an adapter update after every projection


class StepFacts(NamedTuple):
    input: Input
    prefill: bool               # num_prefill_seqs > 0
    m: int                      # num_decoding_seqs
    ignore_kvcache: bool
    positions: bool             # position_indices given
    split: bool                 # num_seq_blocks > 1
    verify: bool
    chunked: bool               # prefill_ctx_lens given
    lora: bool


class LayerFacts(NamedTuple):
    """What `decide_route` needs to know about a layer: computed once (`layer_facts`), never inside a predicate."""
    tuning: object              # the EngineConfig: its tuning switches are read as plain attributes
    skinny: bool                # use_skinny_gemm
    kv_fp8: bool
    fused_qkv: bool
    dtype: torch.dtype
    hidden: int
    head_dim: int
    qkv_splits: int             # k-splits linear_splitk picks for the fused qkv projection at <= 32 tokens (0: none)
    qkv_even: bool              # packed fused qkv whose splits are even splits of whole 128-column tiles (norm on the fly)
    o_splits: int               # ... for o_proj
    rows_o: bool                # linear_rows_add takes o_proj / down_proj
    rows_down: bool
    fly_ffn: bool               # the SiLU-gate GEMM can apply a norm itself (NF / NX / pending row scale)
    tiny: bool                  # qkv and up/gate can sum the previous projection's slabs themselves
    merge: bool                 # o_proj can merge flash-decoding partials itself
    # the model has a q/k/v bias, a per-head QK-norm, or q_size != hidden (Qwen2, Qwen3, Mistral-Nemo): q/k/v stay plain
    # tensors up to the store — none of the forms that consume the qkv projection's slabs, and no rotary + store fusion
    plain_qkv: bool = False
    # a mixture-of-experts FFN: the FFN norm ends in a tensor, the experts (kernels/moe.py) return one
    moe: bool = False


def layer_facts(engine_config, dtype, hidden: int, num_q_heads: int, head_dim: int, shapes: dict, packed, lib,
                plain_qkv: bool = False, moe: bool = False) -> LayerFacts:
    """`shapes`: (N, K) of "qkv" (absent without the fused projection), "o", "up_gate", "down"; `packed`: the names that
    carry a packed twin; `lib`: the loaded library, asked for its host arithmetic only (split counts, shape support)."""
    def takes(name):            # the weight-streaming GEMMs take the shape
        n, k = shapes.get(name, (0, 0))
        return n > 0 and n % 32 == 0 and k % 128 == 0

    def splits(name, plain=False):  # the split count linear_splitk (plain: the row-major kernels) picks at <= 32 tokens
        choose = lib.swl_gemm_skinny_choose_splits if plain or name not in packed else lib.swl_gemm_skinny_packed_choose_splits
        return int(choose(*shapes[name])) if takes(name) else 0

    def chunked(name, ks):      # csrc/gemm_tiny.hip: every K-chunk is whole tiles and fits the workgroup's LDS
        k = shapes[name][1]
        return ks > 0 and k % ks == 0 and (k // ks) % 128 == 0 and k // ks <= _TINY_MAX_KC

    def rows(name):
        n, k = shapes[name]
        return name in packed and takes(name) and n == hidden and bool(lib.swl_gemm_rows_supported(1, n, k))
    fused, up_n, up_k = "qkv" in shapes, *shapes["up_gate"]
    qkv_splits = splits("qkv")
    return LayerFacts(
        tuning=engine_config, skinny=bool(engine_config.use_skinny_gemm), kv_fp8=engine_config.kv_cache_dtype == "fp8_e4m3",
        fused_qkv=fused, dtype=dtype, hidden=hidden, head_dim=head_dim, qkv_splits=qkv_splits,
        qkv_even="qkv" in packed and qkv_splits >= 1 and shapes["qkv"][1] % (128 * qkv_splits) == 0,
        o_splits=splits("o"), rows_o=rows("o"), rows_down=rows("down"),
        fly_ffn="up_gate" in packed and takes("up_gate") and up_n % 64 == 0,
        tiny=("qkv" in packed and "up_gate" in packed and shapes["qkv"][1] == shapes["down"][0]
              and splits("qkv", True) in (1, 2, 4) and chunked("qkv", splits("qkv", True))
              and up_n % 128 == 0 and up_k % 128 == 0 and up_k <= _TINY_MAX_KC and splits("o", True) > 1 and splits("down", True) > 1),
        merge=("o" in packed and head_dim % 8 == 0 and shapes["o"][1] == num_q_heads * head_dim
               and splits("o", True) > 1 and chunked("o", splits("o", True))),
        plain_qkv=bool(plain_qkv), moe=bool(moe))


def decide_route(f: LayerFacts, s: StepFacts) -> LayerRoute:
    """The launches of one layer for one step shape. Pure: no launch, no allocation, nothing of the layer is touched."""
    piggyback = s.prefill and s.m > 0
    attention = Attn.DECODE if not s.prefill else Attn.VERIFY if s.verify else Attn.PAGED if s.chunked else Attn.FRESH
    # rotary + KV store can be one launch; the projections' slabs can go to fused consumers; ... to the attention prologue
    # (a LoRA step takes none of the fused forms: they consume a projection's output before a delta could be added)
    rope_store = not (s.lora or s.ignore_kvcache or f.kv_fp8 or f.plain_qkv) and s.positions and f.tuning.fuse_rope_kvstore
    fast = f.skinny and not (s.lora or s.prefill) and s.m > 0 and f.tuning.fuse_splitk_consumers
    slab_attn = (fast and rope_store and f.fused_qkv and f.tuning.fuse_rope_into_attention and f.head_dim in (32, 64, 128)
                 and s.m <= 256)      # (batches the slab-producing GEMMs serve)
    # the 1/rms of a norm can be left to the consumer of the normalised activations: bfloat16, <= 32 sequences
    defer = f.tuning.defer_rmsnorm and deferred_norm_ok(s.m, f.hidden, f.dtype)
    deferred = slab_attn and defer and f.qkv_splits in (1, 2, 4)
    rows = (not f.moe and f.tuning.rows_decode and slab_attn and (deferred or f.hidden % 1024 == 0) and s.m <= ROWS_O_MAX_M and f.rows_o
            and f.fly_ffn)
    rows_down = rows and s.m <= ROWS_DOWN_MAX_M and f.rows_down and f.qkv_even
    tiny = not f.moe and s.input is Input.SLABS and f.tuning.tiny_decode_batches and s.m <= TINY_POLICY_M and deferred and f.tiny

    if s.input in (Input.RAW, Input.RAW_SSQ):
        # the previous layer's route is this one: its down projection ran row-owned, in the form this layer's norm takes
        assert rows_down and (s.input is Input.RAW) == deferred, "a RawResidual reached a layer whose route hands none on"
        attn_norm = AttnNorm.RAW_NF if deferred else AttnNorm.RAW_NX
    elif s.input is Input.SLABS:
        attn_norm = AttnNorm.TINY if tiny else AttnNorm.SCALE_PENDING if deferred else AttnNorm.FUSED
    else:
        attn_norm = AttnNorm.FUSED
    if slab_attn:
        qkv = QKV.SLABS_ATTN
    elif fast and rope_store and f.fused_qkv:
        qkv = QKV.SLABS_ROTARY
    elif rope_store:
        qkv = QKV.FUSED_PREFILL if s.prefill else QKV.FUSED_DECODE
    else:
        qkv = QKV.ROTARY_ONLY if s.ignore_kvcache else QKV.ROTARY_THEN_STORE
    if f.moe:
        # the router and the experts read the normalised activations as a tensor: the forms that end in one
        o_ffn, down = OFfn.SPLITK_FUSED if fast else OFfn.PLAIN, Down.MOE
    elif tiny:
        o_ffn, down = OFfn.TINY, Down.SPLITK
    elif rows:
        o_ffn = OFfn.ROWS_NF if deferred else OFfn.ROWS_NX
        down = Down.SPLITK if not rows_down else Down.ROWS if deferred else Down.ROWS_SSQ
    elif fast:
        o_ffn, down = OFfn.SPLITK_DEFERRED if defer and f.o_splits > 1 and f.fly_ffn else OFfn.SPLITK_FUSED, Down.SPLITK
    else:
        o_ffn, down = OFfn.PLAIN, Down.PLAIN
    return LayerRoute(attn_norm, qkv, attention, piggyback, tiny and s.split and f.merge, o_ffn, down, s.lora)


_INPUT = {torch.Tensor: Input.TENSOR, SplitKPartials: Input.SLABS, RawResidual: Input.RAW}


class LlamaTransformerLayer:
    def __init__(self, model_config, engine_config, weight, decoding_piggyback_stream, layer_id: int):
        self.model_config = model_config
        self.engine_config = engine_config
        self.weight = weight
        self.decoding_piggyback_stream = decoding_piggyback_stream
        self.layer_id = layer_id
        self.skinny = bool(engine_config.use_skinny_gemm)
        self.moe_tap = None         # tests: a list that receives (layer_id, topk_ids, topk_w) per step (LlamaModel.moe_tap)
        self.refresh_facts()

    def refresh_facts(self):
        """(Re)compute the layer's static facts and forget the routes decided from them: at construction, and again when
        the packed twins of the weights are rebuilt (LlamaModel.repack_decode_weights)."""
        cfg, w = self.model_config, self.weight
        self.moe = getattr(w, "expert_up_gate", None) is not None
        named = dict(qkv=w.qkv_proj, o=w.o_proj, up_gate=getattr(w, "up_gate_proj", None), down=getattr(w, "down_proj", None))
        # bias + QK-norm + rotary in one launch where the model has either (Qwen2 / Qwen3); otherwise swl_rotary
        self.qk_prep = getattr(w, "q_norm", None) is not None or getattr(w, "q_bias", None) is not None
        self.facts = layer_facts(self.engine_config, w.o_proj.dtype, cfg.hidden_size, cfg.num_q_heads, cfg.head_dim,
                                 {**{name: tuple(t.shape) for name, t in named.items() if t is not None},
                                    **(dict(up_gate=tuple(w.expert_up_gate.shape[1:]), down=tuple(w.expert_down.shape[1:]))
                                       if self.moe else {})},
                                 {name for name, t in named.items() if getattr(t, "_swl_packed", None) is not None},
                                 _hip.load(), plain_qkv=self.qk_prep or cfg.num_q_heads * cfg.head_dim != cfg.hidden_size,
                                 moe=self.moe)
        self._routes = {}           # StepFacts -> LayerRoute

    def route(self, input_embds, st) -> LayerRoute:
        kind = Input.RAW_SSQ if getattr(input_embds, "ssq", None) is not None else _INPUT.get(type(input_embds), Input.TENSOR)
        step = StepFacts(kind, st.num_prefill_seqs > 0, st.num_decoding_seqs, bool(st.ignore_kvcache),
                         st.position_indices is not None, st.num_seq_blocks > 1, bool(st.verify),
                         st.prefill_ctx_lens is not None, st.lora is not None)
        route = self._routes.get(step)
        if route is None:
            route = self._routes[step] = decide_route(self.facts, step)
        return route

    def _split_qkv(self, qkv: torch.Tensor):
        cfg = self.model_config
        hq, hkv = cfg.num_q_heads * cfg.head_dim, cfg.num_kv_heads * cfg.head_dim
        t = qkv.shape[0]
        return (qkv[:, :hq].view(t, cfg.num_q_heads, cfg.head_dim),
                qkv[:, hq:hq + hkv].view(t, cfg.num_kv_heads, cfg.head_dim),
                qkv[:, hq + hkv:].view(t, cfg.num_kv_heads, cfg.head_dim))

    def _project_qkv(self, x: torch.Tensor):
        cfg, w, sk = self.model_config, self.weight, self.skinny
        if w.qkv_proj is not None:
            return self._split_qkv(linear(x, w.qkv_proj, sk))   # q/k/v are column slices of one output
        t = x.shape[0]
        return (linear(x, w.q_proj, sk).view(t, cfg.num_q_heads, cfg.head_dim),
                linear(x, w.k_proj, sk).view(t, cfg.num_kv_heads, cfg.head_dim),
                linear(x, w.v_proj, sk).view(t, cfg.num_kv_heads, cfg.head_dim))

    def _rotary(self, q, k, v, st):
        """The launch between the projections and the KV store on the routes that keep the two apart."""
        if not self.qk_prep:
            rotary_embedding_inplace(q, k, st)
            return
        w = self.weight
        qk_prep_rotary_inplace(q, k, v, st, q_bias=w.q_bias, k_bias=w.k_bias, v_bias=w.v_bias, q_norm=w.q_norm,
                               k_norm=w.k_norm, eps=self.model_config.rms_norm_eps)

    def _attn_out_like(self, x: torch.Tensor) -> torch.Tensor:
        """The attention output buffer [tokens, q_size]: the (already consumed) normed activations themselves when they
        have that width, a fresh buffer when q_size != hidden."""
        qs = self.model_config.num_q_heads * self.model_config.head_dim
        return x if x.shape[1] == qs else x.new_empty((x.shape[0], qs))

    def forward(self, input_embds, residual_buf: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, block_table: torch.Tensor, infer_state):
        route = self.route(input_embds, infer_state)
        if route.lora:
            return self._forward_lora(route, input_embds, residual_buf, k_cache, v_cache, block_table, infer_state)
        attn_out = self._norm_qkv_attention(route, input_embds, residual_buf, k_cache, v_cache, block_table, infer_state)
        return self._down_proj(route, self._o_proj_ffn(route, attn_out, residual_buf, infer_state), residual_buf)

    def _add_norm(self, x, residual_buf, norm_w):
        """residual_buf <- x + residual_buf ; returns rmsnorm(residual_buf) * norm_w — x a tensor (in place) or slabs."""
        if isinstance(x, SplitKPartials):
            return fused_add_rmsnorm_from_splitk(x, residual_buf, norm_w, self.model_config.rms_norm_eps)
        fused_add_rmsnorm_inplace(x, residual_buf, norm_w, self.model_config.rms_norm_eps)
        return x

    def _norm_qkv_attention(self, route, x, residual_buf, k_cache, v_cache, block_table, st):
        """Input norm, q/k/v, rotary, KV store, attention. Returns the attention output [tokens, heads * head_dim] — with
        route.merge the fp32 partials of the split flash-decoding instead."""
        cfg, ecfg, w, eps = self.model_config, self.engine_config, self.weight, self.model_config.rms_norm_eps
        at = (k_cache, v_cache, block_table, cfg, ecfg, st, self.layer_id)
        qkv = pend = None
        if route.attn_norm is AttnNorm.FUSED:
            x = self._add_norm(x, residual_buf, w.attn_norm)
        elif route.attn_norm is AttnNorm.SCALE_PENDING:
            pend = add_scale_from_splitk(x, residual_buf, w.attn_norm, eps)
            x = pend.x
        else:
            # the qkv projection normalises its input itself: the slabs of round(r * attn_norm) — RAW_NX: of the exactly
            # normalised rows — of the residual rows r (TINY: r = residual + down slabs, left in the alternate buffer)
            if route.attn_norm is AttnNorm.TINY:
                qkv, ssq = linear_splitk_from_splitk(x, residual_buf, alt_residual_like(residual_buf), w.attn_norm, w.qkv_proj)
                pend = RowScalePending(None, ssq, qkv.k_splits, eps, cfg.hidden_size)
            elif route.attn_norm is AttnNorm.RAW_NF:
                qkv, pend = linear_splitk_nf(residual_buf, w.attn_norm, w.qkv_proj, eps)
            else:
                qkv = linear_splitk_nx(residual_buf, w.attn_norm, w.qkv_proj, eps, x.ssq)
            # (the attention output is [tokens, heads * head_dim], which need not be the residual's width)
            x = None if route.merge else residual_buf.new_empty((residual_buf.shape[0], cfg.num_q_heads * cfg.head_dim))
        # from here on the attention output overwrites the (already consumed) normed activations
        if route.qkv in (QKV.SLABS_ATTN, QKV.SLABS_ROTARY):
            if qkv is None:
                qkv = linear_splitk(x, w.qkv_proj, always=route.qkv is QKV.SLABS_ATTN)
            if not isinstance(qkv, SplitKPartials):     # a batch beyond the slab kernels: the projection came back whole
                assert pend is None, "deferred RMSNorm reached a path that cannot apply it"
                q, k, v = self._split_qkv(qkv)
                rotary_embedding_and_store_kvcache_decode(q, k, v, *at)
            elif route.qkv is QKV.SLABS_ROTARY:
                q, k, v = rotary_embedding_and_store_kvcache_decode_from_splitk(qkv, *at)
            else:
                scratch = paged_attention_from_qkv_splitk(qkv, *at, x, row_scale=pend, merge=not route.merge)
                return scratch if route.merge else x
        else:
            q, k, v = self._project_qkv(x)
            if route.qkv is QKV.FUSED_DECODE:
                rotary_embedding_and_store_kvcache_decode(q, k, v, *at)
            elif route.qkv is QKV.FUSED_PREFILL:
                rotary_embedding_and_store_kvcache_prefill(q, k, v, *at)
            else:
                self._rotary(q, k, v, st)
                if route.qkv is QKV.ROTARY_THEN_STORE:
                    store_kvcache(k, v, *at)
        x = self._attn_out_like(x)
        self._attention(route, q, k, v, x.view(-1, cfg.num_q_heads, cfg.head_dim), k_cache, v_cache, block_table, st)
        return x

    def _attention(self, route, q, k, v, o, k_cache, v_cache, block_table, st):
        """Whole prompts attend to their fresh projections; prompt chunks behind a resident context (chunked prefill) and
        the rows of a verify step attend to the pool, which the store has just extended; decode rows run paged attention —
        on the side stream, fenced by two events, when they ride along with prompt rows (HBM-bound paged attention
        overlaps the MFMA-bound prefill attention)."""
        cfg, ecfg = self.model_config, self.engine_config
        if route.attention is Attn.DECODE:
            paged_attention(q, k_cache, v_cache, block_table, cfg, ecfg, st, self.layer_id, o)
            return
        if route.piggyback:
            stored = torch.cuda.Event()
            stored.record()
        if route.attention is Attn.VERIFY:
            paged_attention_verify(q, k_cache, v_cache, block_table, o, cfg, ecfg, st, self.layer_id)
        elif route.attention is Attn.PAGED:
            prefill_attention_paged(q, k_cache, v_cache, block_table, o, cfg, ecfg, st, self.layer_id)
        else:
            prefill_attention(q, k, v, o, cfg, ecfg, st)
        if route.piggyback:
            p, side = st.num_prefill_tokens, self.decoding_piggyback_stream
            with torch.cuda.stream(side):
                side.wait_event(stored)
                paged_attention(q[p:], k_cache, v_cache, block_table, cfg, ecfg, st, self.layer_id, o[p:])
                decoded = torch.cuda.Event()
                decoded.record()
            torch.cuda.current_stream().wait_event(decoded)

    def _o_proj_ffn(self, route, x, residual_buf, st):
        """Output projection, residual add + FFN norm, up/gate projection, SiLU-gate: returns the [tokens, ffn] activation."""
        cfg, w, eps, sk = self.model_config, self.weight, self.model_config.rms_norm_eps, self.skinny
        if route.o_ffn is OFfn.ROWS_NF:
            linear_rows_add(x, w.o_proj, residual_buf)
            return linear_silu_gate_nf(residual_buf, w.ffn_norm, eps, w.up_gate_proj)
        if route.o_ffn is OFfn.ROWS_NX:
            ssq = linear_rows_add(x, w.o_proj, residual_buf, with_ssq=True)
            return linear_silu_gate_nx(residual_buf, w.ffn_norm, eps, w.up_gate_proj, ssq)
        if route.o_ffn is OFfn.TINY:
            if route.merge:     # split sequences: no phase-2 launch — o_proj merges the partials of its K-chunk of heads
                attn_out = linear_splitk_from_attn_partials(x, st.decoding_seq_lens, residual_buf.shape[0], cfg.num_q_heads,
                                                            cfg.head_dim, st.seq_block_size, st.num_seq_blocks, w.o_proj,
                                                            residual_buf.dtype)
            else:
                attn_out = linear_splitk(x, w.o_proj)
            # alternate buffer + o_proj slabs -> residual_buf ; up * silu(gate) of rmsnorm(residual_buf)
            return linear_silu_gate_from_splitk(attn_out, alt_residual_like(residual_buf), residual_buf, w.ffn_norm, eps,
                                                w.up_gate_proj)
        if route.o_ffn is OFfn.SPLITK_DEFERRED:
            # element-wise add + scale (fills the chip); the FFN norm's 1/rms goes into the SiLU-gate GEMM
            pend = add_scale_from_splitk(linear_splitk(x, w.o_proj), residual_buf, w.ffn_norm, eps)
            return linear_silu_gate(pend.x, w.up_gate_proj, row_scale=pend)
        attn_out = linear_splitk(x, w.o_proj) if route.o_ffn is OFfn.SPLITK_FUSED else linear(x, w.o_proj, sk)
        attn_out = self._add_norm(attn_out, residual_buf, w.ffn_norm)
        if route.down is Down.MOE:
            return attn_out     # the normalised activations: the experts take them from here (_down_proj)
        act = linear_silu_gate(attn_out, w.up_gate_proj) if sk else None
        if act is None:         # (shapes the one-launch form does not take)
            up_gate = linear(attn_out, w.up_gate_proj, sk)
            silu_and_mul_inplace(up_gate)
            act = up_gate[:, :cfg.ffn_inter_dim]
        return act

    def _down_proj(self, route, act, residual_buf):
        w = self.weight
        if route.down is Down.MOE:
            cfg = self.model_config
            return moe_ffn(act, w.router, w.expert_up_gate, w.expert_down, cfg.num_experts_per_tok, cfg.norm_topk_prob,
                           self.skinny, tap=self.moe_tap, layer_id=self.layer_id)
        if route.down is Down.ROWS:
            linear_rows_add(act, w.down_proj, residual_buf)
            return RawResidual(residual_buf)
        if route.down is Down.ROWS_SSQ:
            return RawResidual(residual_buf, linear_rows_add(act, w.down_proj, residual_buf, with_ssq=True))
        if route.down is Down.SPLITK:
            return linear_splitk(act, w.down_proj)
        return linear(act, w.down_proj, self.skinny)

    def _forward_lora(self, route, x, residual_buf, k_cache, v_cache, block_table, st):
        """The layer of a LoRA step: norm, projection + adapter update, rotary, KV store, attention, projection + update,
        norm, projection + update, SiLU-gate, projection + update. None of the fused forms run here — they consume a
        projection's output before a delta could be added — and the layer takes and returns plain tensors."""
        cfg, ecfg, w, sk = self.model_config, self.engine_config, self.weight, self.skinny
        batch, groups = st.lora.batch, st.lora.layers[self.layer_id]
        fused_add_rmsnorm_inplace(x, residual_buf, w.attn_norm, cfg.rms_norm_eps)
        t = x.shape[0]
        if w.qkv_proj is not None:
            qkv = linear(x, w.qkv_proj, sk)
            lora_apply(x, qkv, groups.qkv_proj, batch)
            q, k, v = self._split_qkv(qkv)
        else:
            q, k, v = linear(x, w.q_proj, sk), linear(x, w.k_proj, sk), linear(x, w.v_proj, sk)
            lora_apply(x, q, groups.q_proj, batch)
            lora_apply(x, k, groups.k_proj, batch)
            lora_apply(x, v, groups.v_proj, batch)
            q = q.view(t, cfg.num_q_heads, cfg.head_dim)
            k, v = k.view(t, cfg.num_kv_heads, cfg.head_dim), v.view(t, cfg.num_kv_heads, cfg.head_dim)
        self._rotary(q, k, v, st)
        if route.qkv is QKV.ROTARY_THEN_STORE:
            store_kvcache(k, v, k_cache, v_cache, block_table, cfg, ecfg, st, self.layer_id)
        # attention output overwrites the (already consumed) normed activations (a fresh buffer when q_size != hidden)
        x = self._attn_out_like(x)
        self._attention(route, q, k, v, x.view(-1, cfg.num_q_heads, cfg.head_dim), k_cache, v_cache, block_table, st)
        q = k = v = qkv = None

        attn_out = linear(x, w.o_proj, sk)
        lora_apply(x, attn_out, groups.o_proj, batch)
        fused_add_rmsnorm_inplace(attn_out, residual_buf, w.ffn_norm, cfg.rms_norm_eps)
        up_gate = linear(attn_out, w.up_gate_proj, sk)
        lora_apply(attn_out, up_gate, groups.up_gate_proj, batch)
        silu_and_mul_inplace(up_gate)
        act = up_gate[:, :cfg.ffn_inter_dim]
        down = linear(act, w.down_proj, sk)
        lora_apply(act, down, groups.down_proj, batch)
        return down
