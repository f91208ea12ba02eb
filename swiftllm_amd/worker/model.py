"""LlamaModel — the data-plane worker: weights, rope tables, paged KV pools, and `forward`.

Public surface and call protocol are the reference's (swiftllm/worker/model.py:18-408):

    model = LlamaModel(engine_config); model.load_weights()
    n = model.profile_num_blocks(); model.init_kvcache_and_swap(n)
    tokens = model.forward(input_ids_list, seq_ids_list, decoding_seq_lens_list)
    model.swap_in_seqs(ids) / model.swap_out_seqs(ids) / model.free_seqs_resources(ids)

so examples/offline.py and the Engine drive it unchanged. Inside, the host side is built for MI355X:
  * all per-forward metadata is planned with numpy (batch_plan.py), packed into ONE pinned buffer and
    shipped with ONE async H2D copy (the reference issues ~10 small synchronous `torch.tensor(...,
    device="cuda")` copies, model.py:272-297);
  * block allocation is decided on a host mirror (block_manager.py): no device sync in `forward`
    except the final D2H of the sampled tokens;
  * rope rows are looked up inside the rotary kernel (no cos/sin gather launches);
  * pure-decode forwards can be captured into hipGraphs, one per batch size, and replayed
    (`EngineConfig.use_hip_graph`): ~400 launches per step collapse into one graph launch;
  * KV pools, block tables and scheduler defaults are sized from the 288 GB of one MI355X.
The compute backend is libswiftllm_hip.so only; without a HIP device this class raises.
"""
import functools
import math
import os
import time
import weakref
from typing import List, Optional

import numpy as np
import torch

from swiftllm_amd import _hip
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.guided import GuideStore, TokenVocab
from swiftllm_amd.model_config import LlamaModelConfig
from swiftllm_amd.sampling_params import SamplingParams, is_greedy
from swiftllm_amd.utils import GB

from .batch_plan import BatchPlan, plan_batch, plan_verify
from .block_manager import BlockManager
from . import decode_engine as _decode_engine
from .decode_replay import DecodeReplay, decode_batch_bucket, graph_bucket, plan_decode, stage_plan
from .infer_state import LlamaInferState
from .kernels.block_swapping import swap_blocks
from .kernels.kv_copy import kv_copy_blocks
from .kernels.linear import RawResidual
from .kernels.paged_attn import verify_max_tokens
from .kernels.rmsnorm import fused_add_rmsnorm_from_splitk, rmsnorm_inplace
from .kernels import logits_process
from .lora import LoraBatch, LoraStaging, LoraStep, LoraStore, parse_lora_modules, rows_of_sequences
from .layers.pre_layer import LlamaPreLayer
from .layers.transformer_layer import LlamaTransformerLayer
from .layers.post_layer import LlamaPostLayer
from .step_logits import PLAIN, LogitsStage, StagedInts, StepLogits
from .token_history import TokenHistory, row_entries
from .weight import load_weights, pack_decode_weights

_DTYPES = {"float16": torch.float16, "fp16": torch.float16, "half": torch.float16,
           "bfloat16": torch.bfloat16, "bf16": torch.bfloat16}


def _require_hip_device():
    if not torch.cuda.is_available():
        raise _hip.HipLibraryError(
            "no HIP device visible: swiftllm_amd's data plane runs only on an AMD GPU (gfx950) "
            "through libswiftllm_hip.so; there is no CPU path")
    _hip.load()


class LlamaModel:
    """A LLaMA model resident on one GPU, driven by the control plane (or directly, offline)."""

    @torch.inference_mode()
    def __init__(self, engine_config: EngineConfig):
        self.engine_config = engine_config
        self.model_config = LlamaModelConfig.load_from_model_path(engine_config.model_path)
        self.dtype = _DTYPES[getattr(engine_config, "dtype", "float16")]
        self.device = torch.device("cuda")
        cfg = self.model_config
        # a q/k/v bias, a per-head QK-norm or q_size != hidden: the layers keep q/k/v plain up to the KV store
        self.plain_qkv = bool(cfg.qkv_bias or cfg.qk_norm or cfg.q_size != cfg.hidden_size)
        if self.plain_qkv and getattr(engine_config, "decode_engine", False):
            raise ValueError(f"tuning={{'decode_engine': True}} cannot serve this {cfg.model_type} model: the persistent "
                             "one-sequence step is laid out for Llama's projections (no q/k/v bias, no per-head QK-norm, "
                             "q_proj as wide as hidden_size)")
        # a mixture-of-experts model (Qwen3-MoE, Mixtral): what is not built for it is refused before any memory is touched
        if cfg.is_moe:
            if getattr(engine_config, "decode_engine", False):
                raise ValueError(f"tuning={{'decode_engine': True}} cannot serve this {cfg.model_type} model: the persistent "
                                 "one-sequence step has a dense FFN, no mixture-of-experts routing")
            if int(getattr(engine_config, "max_loras", 0) or 0) > 0:
                raise ValueError(f"max_loras > 0 cannot serve this {cfg.model_type} model: adapters on mixture-of-experts "
                                 "layers (their experts have no adapter update) are not built")
        # element type of the KV pools: the activation dtype, or e4m3fn (EngineConfig.kv_cache_dtype = "fp8_e4m3")
        self.kv_fp8 = getattr(engine_config, "kv_cache_dtype", "auto") == "fp8_e4m3"
        self.kv_dtype = torch.float8_e4m3fn if self.kv_fp8 else self.dtype
        # FP8 pools: fp32 [2, L, KVH] k/v scales (default 1) and, next to them, their reciprocals computed on the host
        self.kv_scales = self.kv_inv_scales = None

        self.weight = None
        self._cos_cached = self._sin_cached = None
        self.pre_layer = None
        self.transformer_layers = None
        self.post_layer = None

        self.num_blocks = None
        self.k_cache = self.v_cache = None
        self.k_swap = self.v_swap = None
        self.cpu_block_manager = self.gpu_block_manager = None

        self._num_slots = 256        # CUs: one 8-wave paged-attention workgroup each
        # optional callable, invoked by forward() in the calling thread once the step's kernels are enqueued and before
        # the host blocks on the sampled tokens (server/engine.py hides its per-request fan-out behind the running step)
        self.after_launch_hook = None
        # SWL_HOST_PROFILE=1: wall-clock split of forward() on the host (plan / blocks / upload / launch / wait for the
        # tokens), summed over calls — tools read it with host_profile()
        self._host_prof = {} if os.environ.get("SWL_HOST_PROFILE") else None
        self._scratch = None
        # the one-sequence persistent decode step (worker/decode_engine.py); None: shape / device / memory / switch say no
        self._engine = None
        self.engine_fallbacks = 0    # steps re-run on the multi-launch path after the engine reported a timed-out hand-off
        # hipGraph replay of pure-decode steps and the decode look-ahead (worker/decode_replay.py: what forgets a captured
        # graph or a prepared step, and why, is listed there). It and the staged buffers below reach the model weakly — a
        # dropped model frees its HBM at once — and look drop_graphs up at the call: tests wrap it on the replay object.
        me = weakref.ref(self)
        graphs_moved = lambda: me().replay.drop_graphs()    # noqa: E731
        # the per-forward metadata (batch_plan.py): pinned int32 staging and its device twin at a fixed address
        self._plan_ints = StagedInts(graphs_moved)
        self.replay = DecodeReplay(lambda *step: me()._stage_decode(*step), lambda *seqs: me()._plan_next_decode(*seqs),
                                   self._plan_ints, engine_config)
        # a step's logits options (seeded sampling, logits processing, per-token logprobs, guided decoding): their persistent
        # device buffers and pinned staging (worker/step_logits.py); one that grows moves, and the captured graphs go
        self._logits = LogitsStage(graphs_moved)
        # logits processing: the token history of every sequence that asks for it (worker/token_history.py; started by its
        # prefill, dropped by free_seqs_resources)
        self._histories = {}
        # what the last forward / forward_verify call learnt about its tokens: None when no row asked, else one
        # TokenLogprob or None per sequence of the batch
        self.last_logprobs = None
        # guided decoding (swiftllm_amd/guided, kernels/guided.py; EngineConfig.guided_max_states > 0): the host bookkeeping
        # of the mask pool (GuideStore; None = off) and the vocabulary its guides are compiled against
        self.guide_store = self._guide_vocab = None
        # speculative decoding: drafts one verify step takes per sequence (forward_verify) = the verify attention kernel's
        # tokens per sequence (16 / G) minus the last accepted token that leads them; 0 with FP8 pools (no instantiation)
        self.max_draft_tokens = 0 if self.kv_fp8 else max(0, verify_max_tokens(self.model_config) - 1)
        # multi-LoRA serving (EngineConfig.max_loras > 0): the slot stacks of every layer's projections (worker/lora.py),
        # allocated by load_weights; None = off
        self.lora_store = None
        self._lora_staging = LoraStaging()      # pinned staging of a LoRA step's tile lists + the t workspace, reused
        self._moe_tap = None

    # what bench.py and the serving tools read of the replay cache (everything else of it: `replay`)
    _decode_graphs = property(lambda self: self.replay.graphs)
    graph_captures = property(lambda self: self.replay.captures)
    graph_capture_s = property(lambda self: self.replay.capture_s)

    def _graph_bucket(self, plan: BatchPlan):
        return graph_bucket(plan)

    @property
    def moe_tap(self):
        """Tests: set to a list and every mixture-of-experts layer appends (layer_id, topk_ids.cpu(), topk_w.cpu()) per step
        (prefill rows first, as the step's rows are ordered). None (the default) costs nothing. A tapped step copies to the
        host, so it runs eager: never captured into, or replayed from, a decode hipGraph."""
        return self._moe_tap

    @moe_tap.setter
    def moe_tap(self, tap):
        self._moe_tap = tap
        for layer in self.transformer_layers or ():
            layer.moe_tap = tap

    # ------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def load_weights(self):
        """Load (or synthesise) the weights, build the rope tables and the layer objects."""
        _require_hip_device()
        self.weight = load_weights(self.model_config, self.dtype, self.engine_config.model_path,
                                   self.engine_config.use_dummy, device=self.device,
                                   fuse_qkv=getattr(self.engine_config, "fuse_qkv", False))
        self.repack_decode_weights()
        self._tune_routes()
        self._init_to_get_rotary()
        self._num_slots = torch.cuda.get_device_properties(self.device).multi_processor_count
        side_stream = torch.cuda.Stream()
        self.pre_layer = LlamaPreLayer(self.model_config, self.weight)
        self.transformer_layers = [
            LlamaTransformerLayer(self.model_config, self.engine_config, self.weight.layers[i],
                                  side_stream, i)
            for i in range(self.model_config.num_layers)
        ]
        self.moe_tap = self._moe_tap
        self.post_layer = LlamaPostLayer(self.model_config, self.weight)
        self.post_layer.skinny = bool(getattr(self.engine_config, "use_skinny_gemm", False))
        if self.kv_fp8 and self.kv_scales is None:
            cfg = self.model_config
            self.kv_scales = torch.ones((2, cfg.num_layers, cfg.num_kv_heads), dtype=torch.float32, device=self.device)
            self.kv_inv_scales = torch.ones_like(self.kv_scales)
        # (allocated before profile_num_blocks measures: the largest replay bucket's rows)
        ecfg = self.engine_config
        # (... as are the guide mask pool and the vocabulary's device form, when guided decoding is on)
        if int(getattr(ecfg, "guided_max_states", 0) or 0) > 0:
            self._init_guided()
        self._logits.reserve(max(decode_batch_bucket(int(ecfg.max_batch_size)), int(ecfg.max_batch_size)))
        # (... and so are the adapter slot stacks: the KV pool is sized with them)
        if int(getattr(ecfg, "max_loras", 0) or 0) > 0:
            self.lora_store = LoraStore(self.model_config, int(ecfg.max_loras), int(ecfg.max_lora_rank), self.dtype,
                                        self.device, fuse_qkv=self.weight.layers[0].qkv_proj is not None)
            print(f"[Model] LoRA: {ecfg.max_loras} adapter slots of rank <= {ecfg.max_lora_rank}, "
                  f"{self.lora_store.nbytes() / 2**20:.1f} MiB", flush=True)
            for name, path in parse_lora_modules(getattr(ecfg, "lora_modules", None)).items():
                self.load_lora(name, path)

    # ---- guided decoding ---------------------------------------------------------------------------------------------
    _guide_masks = property(lambda self: self._logits.guide_masks)      # (the pool, read only: tests hold it to their reference)

    def set_guide_vocab(self, vocab: TokenVocab):
        """The bytes every token id spells, for models without a tokenizer.json (dummy checkpoints, tests): call it before
        load_weights, or afterwards while no guide is resident. It must spell exactly the model's vocab_size ids."""
        if not isinstance(vocab, TokenVocab):
            raise TypeError("set_guide_vocab takes a swiftllm_amd.guided.TokenVocab")
        if len(vocab) != self.model_config.vocab_size:
            raise ValueError(f"the guide vocabulary spells {len(vocab)} ids, the model's vocabulary has "
                             f"{self.model_config.vocab_size}")
        if self.guide_store is not None:
            if self.guide_store.resident():
                raise RuntimeError("set_guide_vocab while guides are resident: their masks were built from the old vocabulary")
            self._logits.set_vocab(vocab, self.model_config.vocab_size, self.device)
            self.guide_store.vocab = vocab
        self._guide_vocab = vocab

    def _init_guided(self):
        """The mask pool and the device vocabulary. No vocabulary: an error here, at start-up, not at the first guided request."""
        ecfg, vocab_size = self.engine_config, self.model_config.vocab_size
        if self._guide_vocab is None:
            path = os.path.join(str(ecfg.model_path), "tokenizer.json")
            if not os.path.exists(path):
                raise RuntimeError(f"guided_max_states = {ecfg.guided_max_states} but there is no vocabulary: {path} does not "
                                   "exist and LlamaModel.set_guide_vocab was not called")
            self._guide_vocab = TokenVocab.from_tokenizer_json(path, vocab_size)
        self.guide_store = store = GuideStore(int(ecfg.guided_max_states), vocab_size, self._guide_vocab)
        self._logits.set_vocab(self._guide_vocab, vocab_size, self.device, mask_shape=(store.max_states, store.words))
        print(f"[Model] guided decoding: {store.max_states} mask rows, {self._guide_masks.numel() * 4 / 2**20:.1f} MiB", flush=True)

    def _check_guides(self, guides, num_seqs: int, ignore_kvcache: bool):
        """The step's cursors, or None when no sequence is guided. Host only: everything is refused before anything is
        allocated or launched."""
        if guides is None:
            return None
        if len(guides) != num_seqs:
            raise ValueError("guides must be aligned with input_ids_list")
        if all(c is None for c in guides):
            return None
        if self.guide_store is None:
            raise ValueError("this model serves no guided requests: EngineConfig.guided_max_states is 0 (or load_weights "
                             "has not run)")
        if ignore_kvcache:
            raise ValueError("guides cannot be combined with ignore_kvcache")
        for c in guides:
            if c is None:
                continue
            g = c.guide
            if g.evicted or g.refs <= 0 or not 0 <= g.base <= c.mask_row < g.base + g.num_states <= self.guide_store.max_states:
                raise ValueError("a guide cursor whose guide is not held in this model's store (acquire it, and release it "
                                 "only when the sequence is done)")
        return list(guides)

    # ---- multi-LoRA serving ------------------------------------------------------------------------------------------
    def _require_lora_store(self) -> LoraStore:
        if self.lora_store is None:
            raise ValueError("this model serves no LoRA adapters: EngineConfig.max_loras is 0 (or load_weights has not run)")
        return self.lora_store

    @torch.inference_mode()
    def load_lora(self, name: str, path: Optional[str] = None, *, state_dict: Optional[dict] = None,
                  config: Optional[dict] = None) -> int:
        """Load a PEFT adapter (a directory, or its state dict + adapter config) into a free slot; returns the slot.
        Raises ValueError (worker/lora.LoraError) with the reason for anything the LoRA layer path cannot serve."""
        return self._require_lora_store().load(name, path, state_dict=state_dict, config=config)

    @torch.inference_mode()
    def unload_lora(self, name: str) -> int:
        """Zero the adapter's slot and free it. The caller makes sure no sequence in flight names it."""
        return self._require_lora_store().unload(name)

    def loras(self) -> dict:
        """Loaded adapters: name -> slot ({} when the model serves none)."""
        return {} if self.lora_store is None else self.lora_store.names()

    def _tune_routes(self):
        """Which side serves the 65..256-token decode projections of THIS model on THIS device is decided here, once, before
        any request (kernels/route_tune.py): the first replica of a node measures the classes the r04 table does not cover
        and writes the answers next to the checkpoint, every other replica reads them."""
        ecfg = self.engine_config
        if not (getattr(ecfg, "use_skinny_gemm", False) and getattr(ecfg, "pack_decode_weights", False)
                and ecfg.max_batch_size > 64):
            return
        from .kernels.linear import tune_wide_routes
        stats = tune_wide_routes(self.weight.projection_tensors(), [lw.up_gate_proj for lw in self.weight.layers[:1] if getattr(lw, "up_gate_proj", None) is not None],
                                 self.dtype, self.device, ecfg.model_path)
        if stats.get("measured") or stats.get("read"):
            print(f"[Model] decode-projection routing: {stats['measured']} (shape, bucket) classes measured, "
                  f"{stats['read']} read from {stats['path']}", flush=True)

    @torch.inference_mode()
    def repack_decode_weights(self):
        """(Re)build the MFMA-fragment-order copies the decode GEMMs stream (EngineConfig.pack_decode_weights). Called
        by load_weights; call again after modifying weights in place."""
        ecfg = self.engine_config
        if getattr(ecfg, "pack_decode_weights", False) and getattr(ecfg, "use_skinny_gemm", False):
            # The packed copies double the projection weights' footprint. If that would leave less than a quarter
            # of the usable HBM for activations + KV pool, keep only the row-major weights and say so (a 70B model
            # is 140 GB: it fits the 288 GB part once, not twice).
            proj_bytes = sum(t.numel() * t.element_size() for t in self.weight.projection_tensors())
            free_b, total_b = torch.cuda.mem_get_info(self.device)
            usable = total_b * float(getattr(ecfg, "gpu_mem_utilization", 0.97)) - (total_b - free_b)
            if proj_bytes > 0.75 * usable:
                print(f"[Model] pack_decode_weights disabled: a second {proj_bytes / 2**30:.1f} GiB copy of the "
                      f"projection weights would leave {max(0.0, usable - proj_bytes) / 2**30:.1f} GiB for the KV "
                      f"pool; decode GEMMs stream the row-major weights instead", flush=True)
                ecfg.pack_decode_weights = False
                return
            pack_decode_weights(self.weight)
        for layer in self.transformer_layers or ():     # (a call after load_weights: the routes follow the packed twins)
            layer.refresh_facts()
        self._build_decode_engine()

    def _build_decode_engine(self):
        """(Re)build the persistent one-sequence decode step's weight stream (EngineConfig tuning `decode_engine`): a
        third copy of the layer weights, laid out per CU in the order the kernel consumes it. Skipped — the multi-launch
        path serves batch 1 then — when the model shape or the device is not what csrc/decode_engine.hip is laid out for,
        or when the copy would leave less than a quarter of the usable HBM."""
        ecfg, cfg = self.engine_config, self.model_config
        self._engine = None
        if not (getattr(ecfg, "decode_engine", False) and getattr(ecfg, "use_skinny_gemm", False)):
            return
        num_cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        if cfg.head_dim != 128 or not _decode_engine.supported(cfg, num_cus):
            return
        need = _decode_engine.stream_bytes(cfg, torch.empty((), dtype=self.dtype).element_size())
        free_b, total_b = torch.cuda.mem_get_info(self.device)
        usable = total_b * float(getattr(ecfg, "gpu_mem_utilization", 0.97)) - (total_b - free_b)
        if need > 0.75 * usable:
            print(f"[Model] decode_engine disabled: its {need / 2**30:.1f} GiB weight stream would leave "
                  f"{max(0.0, usable - need) / 2**30:.1f} GiB for the KV pool", flush=True)
            return
        self._engine = _decode_engine.DecodeEngine(cfg, self.weight, self.dtype, self.device)

    @torch.inference_mode()
    def profile_num_blocks(self) -> int:
        """How many KV blocks fit: run a forged worst-case prefill without touching the KV cache,
        read the device's high-water mark, give the rest (up to gpu_mem_utilization) to the pool.
        Reference: model.py:94-131."""
        ecfg = self.engine_config
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        num_tokens, batch = ecfg.max_tokens_in_batch, ecfg.max_batch_size
        lens = [num_tokens // batch] * batch
        lens[-1] += num_tokens % batch
        self.k_cache = self.v_cache = None
        self.forward([[0] * n for n in lens], list(range(batch)), [], ignore_kvcache=True)
        torch.cuda.synchronize()
        free_memory, total_memory = torch.cuda.mem_get_info()
        peak_memory = total_memory - free_memory
        usable = total_memory * ecfg.gpu_mem_utilization
        print(f"[Model.profile] GPU total memory: {total_memory / GB:.2f} GB, "
              f"runtime peak memory: {peak_memory / GB:.2f} GB")
        if usable < peak_memory:
            raise RuntimeError(
                f"Peak memory {peak_memory / GB:.2f} GB exceeds usable memory {usable / GB:.2f} GB "
                f"({total_memory / GB:.2f} GB * {ecfg.gpu_mem_utilization})")
        block_bytes = ecfg.block_size * self.model_config.get_kvslot_size(self.kv_dtype)
        # the two block tables (GPU + CPU manager) are allocated after this point: budget them
        table_bytes = 2 * ecfg.max_seqs_in_block_table * ecfg.max_blocks_per_seq * 4
        # ... and so is the private memory pool of the decode hipGraphs (captured on first use, AFTER the KV pool took
        # its share): a max_batch_size decode forward's activations, [B, vocab] logits (+ fp32 argmax candidates) and
        # split-K scratch. The eager prefill peak above does not contain it.
        graph_bytes = 0
        if self.replay.on:
            graph_bytes = self._measure_decode_graph_bytes()
            free_memory, _ = torch.cuda.mem_get_info()      # (the measurement may have grown the regular pool as well)
            peak_memory = max(peak_memory, total_memory - free_memory)
        num_blocks = self.blocks_that_fit(usable - peak_memory - table_bytes - graph_bytes, block_bytes)
        torch.cuda.empty_cache()
        return num_blocks

    @staticmethod
    def blocks_that_fit(pool_bytes: float, block_bytes: int) -> int:
        """KV blocks a budget of `pool_bytes` holds; `block_bytes` = block_size * get_kvslot_size(pool dtype), so an FP8
        pool gets the count a 16-bit pool would get with half the block bytes. The block tables and the hipGraph reserve
        were taken off the budget before: they do not shrink with the pool's element size."""
        return max(math.floor(pool_bytes / block_bytes), 0)

    def _measure_decode_graph_bytes(self) -> int:
        """What the private memory pool of the decode hipGraphs will hold: MEASURED (r03-r04 used a formula) as
        the allocator's high-water mark over one eager pure-decode forward at max_batch_size on a throw-away KV pool of one
        block per sequence — a capture allocates what the eager forward allocates, into its own pool, and all captures share
        ONE pool (DecodeReplay.run), so the largest batch sets its size. 25 % + 16 MiB on top for the allocator's
        rounding. Falls back to the r04 formula when the throw-away pool cannot be built."""
        cfg, ecfg = self.model_config, self.engine_config
        # the largest CAPTURED batch: max_batch_size rounded up to its replay bucket (up to 15 inert rows more)
        b = min(decode_batch_bucket(int(ecfg.max_batch_size)), int(ecfg.max_seqs_in_block_table))
        formula = b * cfg.vocab_size * 8 + b * (cfg.hidden_size + cfg.ffn_inter_dim) * 64 + (64 << 20)
        if b <= 0:
            return formula
        saved = (self.k_cache, self.v_cache, self.gpu_block_manager, self.cpu_block_manager, ecfg.use_hip_graph)
        try:
            shape = (b, cfg.num_layers, cfg.num_kv_heads, ecfg.block_size, cfg.head_dim)
            self.k_cache = torch.zeros(shape, dtype=self.kv_dtype, device=self.device)
            self.v_cache = torch.zeros(shape, dtype=self.kv_dtype, device=self.device)
            self.gpu_block_manager = BlockManager("GPU", b, ecfg.max_seqs_in_block_table, ecfg.max_blocks_per_seq,
                                                  ecfg.block_size, self.device)
            ecfg.use_hip_graph = False
            self.forward([[0]] * b, list(range(b)), [1] * b)        # (also sizes the persistent split-K workspace)
            torch.cuda.synchronize()
            self.gpu_block_manager.free_blocks_for_seqs(list(range(b)))
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            self.forward([[0]] * b, list(range(b)), [1] * b)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            # + what every cached graph keeps alive in the shared pool after its capture: its sampled-token tensor (the
            # [B, vocab] logits are retained only while a test taps them — DecodeReplay.run), rounded to the
            # allocator's 512-byte granule, for a full replay cache
            retained = self.replay.max_graphs * (-(-b * 8 // 512) * 512 + 512)
            measured = int(peak * 1.25) + (16 << 20) + retained
            print(f"[Model.profile] decode activations at batch {b}: {peak / 2**20:.1f} MiB "
                  f"(hipGraph pool reserve {measured / 2**20:.1f} MiB; r04 formula: {formula / 2**20:.1f} MiB)")
            return measured
        except Exception as exc:     # noqa: BLE001 — sizing aid only: any failure falls back to the formula
            print(f"[Model.profile] decode-pool measurement failed ({type(exc).__name__}: {exc}); using the formula")
            return formula
        finally:
            self.k_cache, self.v_cache, self.gpu_block_manager, self.cpu_block_manager, ecfg.use_hip_graph = saved
            self.replay.drop_prepared()
            self.replay.drop_graphs()
            torch.cuda.empty_cache()

    @torch.inference_mode()
    def init_kvcache_and_swap(self, num_blocks: int):
        """Allocate the GPU KV pools, the host swap pools and both block managers.
        Reference: model.py:134-175."""
        _require_hip_device()
        cfg, ecfg = self.model_config, self.engine_config
        self.num_blocks = num_blocks
        shape = (num_blocks, cfg.num_layers, cfg.num_kv_heads, ecfg.block_size, cfg.head_dim)
        # zeros, not empty: stale NaNs in never-written slots would poison 0 * NaN products
        self.k_cache = torch.zeros(shape, dtype=self.kv_dtype, device=self.device)
        self.v_cache = torch.zeros(shape, dtype=self.kv_dtype, device=self.device)
        swap_shape = (ecfg.num_cpu_blocks,) + shape[1:]
        pin = getattr(ecfg, "pin_swap_memory", True) and ecfg.num_cpu_blocks > 0
        try:
            self.k_swap = torch.zeros(swap_shape, dtype=self.kv_dtype, device="cpu", pin_memory=pin)
            self.v_swap = torch.zeros(swap_shape, dtype=self.kv_dtype, device="cpu", pin_memory=pin)
        except RuntimeError:    # host cannot pin that much: pageable pools, as the reference has
            self.k_swap = torch.zeros(swap_shape, dtype=self.kv_dtype, device="cpu")
            self.v_swap = torch.zeros(swap_shape, dtype=self.kv_dtype, device="cpu")
        self.gpu_block_manager = BlockManager("GPU", num_blocks, ecfg.max_seqs_in_block_table,
                                              ecfg.max_blocks_per_seq, ecfg.block_size, self.device)
        self.cpu_block_manager = BlockManager("CPU", ecfg.num_cpu_blocks,
                                              ecfg.max_seqs_in_block_table, ecfg.max_blocks_per_seq,
                                              ecfg.block_size, self.device)
        self.replay.drop_graphs()
        self.replay.drop_prepared()

    @torch.inference_mode()
    def set_kv_scales(self, k_scale: torch.Tensor, v_scale: torch.Tensor):
        """FP8 KV pools: one fp32 scale per (layer, kv-head) for K and for V, tensors of shape [L, KVH] (positive, finite).
        A stored code means code * scale, so the scales may only change while no sequence holds blocks: raises otherwise.
        The reciprocals the quantising stores multiply by are fp32(1 / scale), computed here on the host. The tensors are
        updated in place (captured decode graphs read them by address)."""
        if not self.kv_fp8:
            raise RuntimeError("set_kv_scales needs kv_cache_dtype='fp8_e4m3' (16-bit KV pools have no scales)")
        if self.kv_scales is None:
            raise RuntimeError("set_kv_scales before load_weights")
        cfg = self.model_config
        want = (cfg.num_layers, cfg.num_kv_heads)
        ks = torch.as_tensor(k_scale, dtype=torch.float32, device="cpu")
        vs = torch.as_tensor(v_scale, dtype=torch.float32, device="cpu")
        if tuple(ks.shape) != want or tuple(vs.shape) != want:
            raise ValueError(f"k_scale and v_scale must have shape {want}, got {tuple(ks.shape)} and {tuple(vs.shape)}")
        both = torch.stack([ks, vs])
        if not bool((torch.isfinite(both) & (both > 0)).all()):
            raise ValueError("KV scales must be positive and finite")
        for mgr in (self.gpu_block_manager, self.cpu_block_manager):
            if mgr is not None and mgr.host.num_free_blocks < mgr.host.num_blocks:
                raise RuntimeError("set_kv_scales while sequences hold KV blocks: their stored codes were quantised with "
                                   "the old scales (free or finish them first)")
        self.replay.drop_prepared()
        self.kv_scales.copy_(both)
        self.kv_inv_scales.copy_(1.0 / both)        # fp32 division on the host, one rounding

    def _init_to_get_rotary(self):
        """cos/sin tables [positions, head_dim/2] in the model dtype. Formulas (including the
        non-HuggingFace frequency split used for dict-valued rope_scaling) follow the reference,
        model.py:177-225, evaluated in fp32 on the device."""
        cfg = self.model_config
        dev, f32 = self.device, torch.float32
        base, dim = cfg.rope_theta, cfg.head_dim
        scaling = cfg.rope_scaling
        if isinstance(scaling, dict):
            factor = scaling.get("factor", 4.0)
            low = scaling.get("low_freq_factor", 1.0)
            high = scaling.get("high_freq_factor", 1.0)
            orig = scaling.get("original_max_position_embeddings", cfg.max_position_embeddings)
            t = torch.arange(int(orig * factor) + 128, device=dev, dtype=f32)
            split = int((dim // 2) * low / (low + high))
            inv_low = 1.0 / (base ** (torch.arange(0, split * 2, 2, device=dev, dtype=f32) / dim))
            inv_high = 1.0 / (base ** (torch.arange(split * 2, dim, 2, device=dev, dtype=f32) / dim))
            freqs = torch.cat([torch.outer(t / low, inv_low), torch.outer(t / high, inv_high)], dim=-1)
        else:
            inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, device=dev, dtype=f32) / dim))
            rows = cfg.max_position_embeddings * scaling + 128
            if getattr(cfg, "sliding_window", None) is not None:
                rows = cfg.sliding_window   # exactly the window: beyond it full attention is no longer the model's function
            t = torch.arange(rows, device=dev, dtype=f32) / scaling
            freqs = torch.outer(t, inv_freq)
        self._cos_cached = torch.cos(freqs).to(self.dtype).contiguous()
        self._sin_cached = torch.sin(freqs).to(self.dtype).contiguous()

    # ------------------------------------------------------------------------------------------------
    def _make_infer_state(self, plan: BatchPlan, dev: dict, ignore_kvcache: bool, opts: StepLogits = PLAIN,
                          scratch_rows: int = None) -> LlamaInferState:
        """`scratch_rows`: rows whose flash-decoding partials the persistent scratch must hold when the step splits its
        sequences — the decoding sequences (default); a verify step: every row."""
        nsb = plan.num_seq_blocks
        if nsb > 1:
            need = _hip.scratch_bytes(plan.num_decoding_seqs if scratch_rows is None else scratch_rows,
                                      self.model_config.num_q_heads, self.model_config.head_dim, nsb) // 4
            if self._scratch is None or self._scratch.numel() < need:
                self._scratch = torch.empty(need, dtype=torch.float32, device=self.device)
                self.replay.drop_graphs()
        return LlamaInferState(
            batch_size=plan.batch_size, num_tokens=plan.num_tokens,
            seq_ids=dev["seq_ids"], softmax_scale=self.model_config.head_dim ** -0.5,
            num_prefill_seqs=plan.num_prefill_seqs, num_prefill_tokens=plan.num_prefill_tokens,
            prefill_seq_start_locs=dev["prefill_start_locs_with_end"][:plan.num_prefill_seqs],
            prefill_seq_start_locs_with_end=dev["prefill_start_locs_with_end"],
            prefill_seq_lens=dev["prefill_seq_lens"], max_prefill_len=plan.max_prefill_len,
            num_decoding_seqs=plan.num_decoding_seqs, decoding_seq_lens=dev["decoding_seq_lens"],
            max_decoding_len=plan.max_decoding_len,
            seq_block_size=plan.seq_block_size, num_seq_blocks=nsb,
            position_cos=self._cos_cached, position_sin=self._sin_cached,
            ignore_kvcache=ignore_kvcache,
            position_indices=dev["position_indices"], last_token_indices=dev["last_token_indices"],
            paged_attn_scratch=self._scratch if nsb > 1 else None,
            logits=self._logits.args(opts, dev["seq_lengths"]),
            prefill_ctx_lens=dev.get("prefill_ctx_lens"), max_prefill_total_len=plan.max_prefill_total_len,
            kv_scales=self.kv_scales, kv_inv_scales=self.kv_inv_scales,
            verify=plan.verify_row_lens is not None, verify_row_lens=dev.get("verify_row_lens"))

    @torch.inference_mode()
    def _forward(self, input_ids: torch.Tensor, infer_state: LlamaInferState) -> torch.Tensor:
        """Embedding -> L transformer blocks -> final norm / lm_head / argmax.
        Reference: model.py:228-249."""
        if self._engine_applies(infer_state):
            # ONE sequence, pure decode: embedding + all transformer blocks in one persistent launch
            x = self._engine.step(self.k_cache, self.v_cache, self.gpu_block_manager.block_table, input_ids,
                                  infer_state.seq_ids, infer_state.decoding_seq_lens, self._cos_cached, self._sin_cached,
                                  self.engine_config.max_blocks_per_seq)
            rmsnorm_inplace(x, self.weight.final_norm, self.model_config.rms_norm_eps)
            return self.post_layer.forward_normed(x, self._engine.tok_err[:1], infer_state.logits)
        x = self.pre_layer.forward(input_ids)
        residual = torch.zeros_like(x)
        block_table = None if infer_state.ignore_kvcache else self.gpu_block_manager.block_table
        for layer in self.transformer_layers:
            x = layer.forward(x, residual, self.k_cache, self.v_cache, block_table, infer_state)
        if isinstance(x, RawResidual):          # the last down projection added itself into the residual (rows_decode):
            x = residual.clone()                # pure decode, every row a last token — final norm of the residual rows
            rmsnorm_inplace(x, self.weight.final_norm, self.model_config.rms_norm_eps)
        elif not isinstance(x, torch.Tensor) and infer_state.num_prefill_seqs == 0:
            # the last down projection left as split-K partials, pure decode: every row is a last token — reduce +
            # residual add + final norm in one launch
            x = fused_add_rmsnorm_from_splitk(x, residual, self.weight.final_norm, self.model_config.rms_norm_eps)
        else:
            if not isinstance(x, torch.Tensor):     # split-K partials of a step with prompt rows
                x = x.materialize()
            x += residual
            return self.post_layer.forward(x, infer_state)
        return self.post_layer.forward_normed(x, logits=infer_state.logits)

    def _engine_applies(self, st) -> bool:
        return (self._engine is not None and getattr(st, "lora", None) is None and st.num_prefill_seqs == 0 and st.batch_size == 1
                and st.num_decoding_seqs == 1 and not st.ignore_kvcache and self.k_cache is not None)

    def _engine_failed(self, code: int):
        """A hand-off of the persistent step timed out (bounded spins: the launch ended, its results are garbage). Say so,
        clear the workspace, and leave batch 1 to the multi-launch HIP path from here on."""
        print(f"[Model] decode engine reported error {code & 0xff} (CU {code >> 8}): falling back to the multi-launch "
              f"decode path for one-sequence steps", flush=True)
        torch.cuda.synchronize()
        self._engine.reset()
        self._engine = None
        self.replay.drop_graphs()
        self.replay.drop_prepared()
        self.engine_fallbacks += 1

    def _stage_decode(self, plan: BatchPlan, dev: dict, opts: StepLogits):
        """DecodeReplay's way to one eager decode step: its infer state now (the scratch it sizes may move), the launch later."""
        return functools.partial(self._forward, dev["input_ids"], self._make_infer_state(plan, dev, False, opts))

    def _plan_next_decode(self, seq_ids_list: List[int], lens: List[int]) -> Optional[BatchPlan]:
        """DecodeReplay's plan of the step after a decode step; None when a sequence would leave the rotary table."""
        if max(lens) > self._cos_cached.shape[0]:
            return None
        return plan_decode(seq_ids_list, lens, None, True, self.model_config.num_kv_heads, self._num_slots)

    # ------------------------------------------------------------------------------------------------
    def _tokens_to_host(self, tokens: torch.Tensor, scoring=None) -> List[int]:
        """The step's one D2H copy (and its one sync). A step of the persistent decode engine brings its error word back in
        the same copy (DecodeEngine.tok_err = [token, error]). A scored step's results are copied into their pinned buffer
        first, on the same stream: the tokens' sync covers them, and `last_logprobs` is read off that buffer afterwards."""
        read_scores = None if scoring is None else self._logits.fetch_scores(scoring)
        eng = self._engine
        if eng is not None and tokens.data_ptr() == eng.tok_err.data_ptr():
            out, err = eng.tok_err.tolist()
            if err != 0:
                raise _decode_engine.DecodeEngineError(str(err))
            out = [out]
        else:
            out = tokens.tolist()
        if read_scores is not None:
            self.last_logprobs = read_scores()
        return out

    @torch.inference_mode()
    def forward(self, input_ids_list: List[List[int]], seq_ids_list: List[int],
                decoding_seq_lens_list: List[int], ignore_kvcache: bool = False,
                sampling_params: Optional[List[Optional[SamplingParams]]] = None,
                prefill_ctx_lens: Optional[List[int]] = None, lora: Optional[List[Optional[str]]] = None,
                guides: Optional[List[Optional[object]]] = None) -> List[int]:
        """One iteration: prefill sequences first, then decoding sequences (one token each, their
        lengths in `decoding_seq_lens_list` INCLUDE that token). Returns the next token of every
        sequence: greedy (the reference, model.py:252-359), or — for the entries of `sampling_params`
        (aligned with `input_ids_list`) that are not greedy — a seeded draw at the position the token
        takes (a None seed draws a fresh one for this call). All-greedy steps launch what they always did.
        Entries whose `logprobs` is set make the step a scored one: `last_logprobs` then holds, aligned with the batch, a
        TokenLogprob for each of them (the returned token's log-probability and rank, and its top-N alternatives, over
        the logits the token was picked from) and None for the others; after any other step it is None. The tokens are
        those of the same call without the field.

        `prefill_ctx_lens` (chunked prefill; one entry per prefill sequence): tokens of that sequence already resident
        in the KV pool from earlier calls. Its `input_ids` are then the next chunk of its prompt: the chunk is stored
        behind the context and attends to the pool (csrc/prefill_attn_paged.hip). The token returned for it follows the
        chunk's last token — the caller ignores it for every chunk but the last; a sampled draw is keyed by position, so
        the final chunk draws what a whole-prompt prefill draws from the same logits. None or all zeros: today's path.

        `lora` (multi-LoRA serving; aligned with `input_ids_list`): the name of a loaded adapter, or None, per sequence.
        None or all None: today's call, launch for launch. Otherwise the step runs the LoRA layer path eagerly (no
        hipGraph, no look-ahead): every row of a named sequence gets its adapter's low-rank update on every projection.

        `guides` (guided decoding; aligned with `input_ids_list`): a swiftllm_amd.guided.GuideCursor over a guide held in
        `guide_store`, or None, per sequence. None or all None: today's call, launch for launch. Otherwise the logits of a
        guided row are masked to the tokens its cursor's state allows before anything else reads them (csrc/guided.hip);
        a guide that is not built yet is built first, on the step's stream. The model does NOT advance the cursors: the
        caller does, with the returned tokens (and not with the token of a prompt chunk that is not the last). Refused with
        ignore_kvcache and when EngineConfig.guided_max_states is 0; forward_verify takes no guides."""
        self.last_logprobs = None
        if len(input_ids_list) == 0:
            return []   # the reference's idle engine calls forward([], [], []) in a loop
        guides = self._check_guides(guides, len(input_ids_list), ignore_kvcache)
        lora_slots = self._resolve_lora(lora, len(input_ids_list))
        _require_hip_device()
        prefill_ctx_lens = self._check_prefill_ctx(input_ids_list, seq_ids_list, decoding_seq_lens_list, ignore_kvcache,
                                                   prefill_ctx_lens)
        sampling = scoring = None
        if sampling_params is not None:
            if len(sampling_params) != len(input_ids_list):
                raise ValueError("sampling_params must be aligned with input_ids_list")
            if not all(is_greedy(p) for p in sampling_params):
                sampling = [None if is_greedy(p) else p.with_seed() for p in sampling_params]
            # a scored step: the N of every row that asks for logprobs (SamplingParams.logprobs), None for the others
            if not ignore_kvcache and any(p is not None and p.logprobs is not None for p in sampling_params):
                scoring = [None if p is None else p.logprobs for p in sampling_params]
        # logits processing: the histories move ONCE per call, here (the engine fallback below runs the step twice)
        # (a step that raises — block allocation, the rotary table — takes its history updates back: the caller may repeat
        # the call, and the other sequences of the batch stay in step)
        edits, undo = None, []
        if not ignore_kvcache and (self._histories or (sampling_params is not None and any(
                p is not None and p.processes_logits for p in sampling_params))):
            edits = self._track_histories(input_ids_list, seq_ids_list, decoding_seq_lens_list,
                                          sampling_params or [None] * len(input_ids_list), prefill_ctx_lens, undo)
        opts = StepLogits.of(sampling, edits, scoring, guides)
        step = functools.partial(self._forward_step, input_ids_list, seq_ids_list, decoding_seq_lens_list, ignore_kvcache,
                                 opts, prefill_ctx_lens, lora_slots)
        try:
            try:
                return step()
            except _decode_engine.DecodeEngineError as exc:
                # bounded hand-off timed out inside the persistent one-sequence step: its KV writes are re-done below with
                # the same values by the multi-launch HIP path, which serves one-sequence steps from here on
                self._engine_failed(int(str(exc)))
                return step()
        except BaseException:
            self._rollback_histories(undo)
            raise

    def _resolve_lora(self, lora, num_seqs: int):
        """Per-sequence slots (-1 = no adapter) of a LoRA step, or None when no sequence names an adapter. Host only: an
        unknown name is refused before anything is allocated or launched."""
        if lora is None:
            return None
        if len(lora) != num_seqs:
            raise ValueError("lora must be aligned with input_ids_list")
        if all(n is None for n in lora):
            return None
        store = self._require_lora_store()
        return [-1 if n is None else store.slot_of(n) for n in lora]

    def _rollback_histories(self, undo):
        for rec in reversed(undo):
            if rec[0] == "slot":        # a history that was started, replaced or dropped
                _, sid, old = rec
                if old is None:
                    self._histories.pop(sid, None)
                else:
                    self._histories[sid] = old
            else:
                _, hist, mark, words = rec
                hist.rollback(mark, words)

    def _track_histories(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, params, prefill_ctx_lens, undo):
        """Bring the token histories up to this call and return the step's entries: one RowEdits per row whose params
        process logits, None for the others — or None when no row does. Prefill tokens (whole prompts and chunks) are
        prompt tokens, a decode row's input token is an output token. A history starts at a prefill call without a context
        whose params process logits; every tracked sequence is held to its length (ValueError when out of step), and a row
        that processes logits without a history is refused. Everything is checked before anything is changed; what is
        changed is recorded in `undo` (see _rollback_histories: forward takes it back when the step itself raises)."""
        n_pre = len(input_ids_list) - len(decoding_seq_lens_list)
        ctx = prefill_ctx_lens or [0] * n_pre
        vocab = self.model_config.vocab_size
        for i, (ids, sid, p) in enumerate(zip(input_ids_list, seq_ids_list, params)):
            proc = p is not None and p.processes_logits
            h = self._histories.get(sid)
            if i < n_pre and ctx[i] == 0:
                if proc and (any(t >= vocab for t, _ in p.logit_bias or ()) or any(t >= vocab for t in p.stop_token_ids)):
                    raise ValueError(f"sequence {sid}: logit_bias and stop_token_ids must name ids in [0, {vocab})")
                continue
            if h is None:
                if proc:
                    raise ValueError(f"sequence {sid}: its sampling params process logits but it has no token history "
                                     "(the history starts at the sequence's first prefill call with such params)")
                continue
            have = ctx[i] if i < n_pre else decoding_seq_lens_list[i - n_pre] - 1
            if len(h) != have or (i < n_pre and h.num_output):
                raise ValueError(f"sequence {sid}: its token history holds {len(h)} tokens ({h.num_output} generated), "
                                 f"this call places it at {have}: out of step")
        rows, any_row = [], False
        for i, (ids, sid, p) in enumerate(zip(input_ids_list, seq_ids_list, params)):
            proc = p is not None and p.processes_logits
            if i < n_pre and ctx[i] == 0:
                old = self._histories.pop(sid, None)      # (a sequence id that starts over)
                if proc:
                    self._histories[sid] = TokenHistory(max(64, 2 * len(ids)))
                if old is not None or proc:
                    undo.append(("slot", sid, old))
            h = self._histories.get(sid)
            if h is not None:
                words = []
                undo.append(("meta", h, h.mark(), words))
                if i < n_pre:
                    h.add_prompt(ids, words)
                else:
                    h.add_output(ids[0], words)
            if not proc:
                rows.append(None)
                continue
            e_ids, e_meta, e_bias = row_entries(p, h)
            rows.append(logits_process.RowEdits(e_ids, e_meta, e_bias, p.repetition_penalty, p.presence_penalty,
                                                p.frequency_penalty, p.min_p_gap()))
            any_row = True
        return rows if any_row else None

    def _check_prefill_ctx(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, ignore_kvcache, ctx):
        """Host-side refusals of a chunked-prefill call, before anything is launched or allocated. Returns the contexts
        as a list, or None when there are none (None / all zeros: the whole-prompt path, bit for bit)."""
        if ctx is None:
            return None
        ctx = [int(c) for c in ctx]
        num_prefill = len(input_ids_list) - len(decoding_seq_lens_list)
        if len(ctx) != num_prefill:
            raise ValueError(f"prefill_ctx_lens needs one entry per prefill sequence ({num_prefill}), got {len(ctx)}")
        if any(c < 0 for c in ctx):
            raise ValueError("prefill_ctx_lens must be >= 0")
        if not any(ctx):
            return None
        if ignore_kvcache:
            raise ValueError("prefill_ctx_lens with ignore_kvcache=True: a context lives in the KV cache")
        if self.gpu_block_manager is None:
            raise RuntimeError("prefill_ctx_lens before init_kvcache_and_swap: there is no KV pool to hold a context")
        bs = self.engine_config.block_size
        rope_rows = self._cos_cached.shape[0]
        for c, sid, ids in zip(ctx, seq_ids_list, input_ids_list):
            have = self.gpu_block_manager.host.num_allocated(sid) * bs
            if c > have:
                raise ValueError(f"sequence {sid}: a context of {c} tokens, but its allocated KV blocks hold {have}")
            if c + len(ids) > rope_rows:
                raise RuntimeError(f"sequence {sid}: context {c} + {len(ids)} new tokens exceeds the rotary table "
                                   f"({rope_rows} positions)")
        return ctx

    def _begin_step(self, plan: BatchPlan, seq_ids_list, ignore_kvcache: bool = False, opts: StepLogits = PLAIN):
        """What every step does between its plan and its launches: the rotary-table check, KV blocks for the caller's
        sequences, the plan's upload and what the step's logits options read. Returns the plan's device views and the
        host times at which the checked plan and the blocks were ready (host_profile's sections)."""
        num_real = plan.num_real_seqs = len(seq_ids_list)
        longest = max(plan.seq_lengths_list)
        if longest > self._cos_cached.shape[0]:
            # the reference indexes its rope cache out of range here (model.py:350); fail on the host
            raise RuntimeError(
                f"sequence length {longest} exceeds the rotary table ({self._cos_cached.shape[0]} positions = "
                "max_position_embeddings * rope_scaling + 128); use a checkpoint with rope scaling")
        t_plan = time.perf_counter()
        if not ignore_kvcache:
            self.gpu_block_manager.allocate_blocks_for_seqs(seq_ids_list, plan.seq_lengths_list[:num_real])
        t_blocks = time.perf_counter()
        ecfg = self.engine_config       # (pinned memory, one async H2D copy; the buffer's first capacity serves any step)
        dev = stage_plan(self._plan_ints, plan, 2 * ecfg.max_tokens_in_batch + 8 * ecfg.max_batch_size + 64)
        self._logits.upload(opts, plan.batch_size)
        return dev, t_plan, t_blocks

    def _launch_eager(self, plan: BatchPlan, seq_ids_list, ignore_kvcache: bool = False, opts: StepLogits = PLAIN,
                      lora=None, scratch_rows: int = None):
        """The eager step, whoever drives it: _begin_step, the infer state (`lora`, `scratch_rows`: what a LoRA and a verify
        step attach), the forward, after_launch_hook. Returns every row's token and the host times of host_profile's sections."""
        dev, t_plan, t_blocks = self._begin_step(plan, seq_ids_list, ignore_kvcache, opts)
        t_upload = time.perf_counter()
        state = self._make_infer_state(plan, dev, ignore_kvcache, opts, scratch_rows)
        state.lora = lora
        tokens = self._forward(dev["input_ids"], state)
        if self.after_launch_hook is not None:
            self.after_launch_hook()
        return tokens, (t_plan, t_blocks, t_upload)

    def _launch_replay(self, plan: BatchPlan, dev: dict, seq_ids_list, opts: StepLogits):
        """A pure-decode step on the replay path: its graph, then — behind it — the preparation of the step expected next."""
        tokens = self.replay.run(plan, dev, opts, self._engine is not None and plan.batch_size == 1, self.post_layer)
        self.replay.prepare_next(plan, seq_ids_list, tokens, opts)
        if self.after_launch_hook is not None:
            self.after_launch_hook()
        return tokens

    def _forward_step(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, ignore_kvcache, opts: StepLogits = PLAIN,
                      prefill_ctx_lens=None, lora_slots=None):
        prof = self._host_prof
        t0 = time.perf_counter() if prof is not None else 0.0
        if lora_slots is not None:
            return self._forward_step_lora(input_ids_list, seq_ids_list, decoding_seq_lens_list, ignore_kvcache, opts,
                                           prefill_ctx_lens, lora_slots)
        if self._moe_tap is not None:
            self.replay.drop_prepared()     # (tests) a tapped step copies the routing to the host: eager, not a replay
        la = self.replay.take(input_ids_list, seq_ids_list, decoding_seq_lens_list, ignore_kvcache, opts)
        if la is not None:      # the step that was prepared while the previous one ran: blocks, then the launch
            self.gpu_block_manager.allocate_blocks_for_seqs(la.seq_ids, la.lens)   # (the real sequences only)
            self._logits.upload(opts, la.plan.batch_size, hit=True)
            tokens = self._launch_replay(la.plan, la.dev, la.seq_ids, opts)
        else:
            num_real = len(input_ids_list)
            pure_decode = len(decoding_seq_lens_list) == num_real and not ignore_kvcache
            graph_step = pure_decode and self.replay.on and self._moe_tap is None
            in_buckets = pure_decode and self.replay.eager_in_buckets
            if graph_step or in_buckets:
                # pure decode on the replay path: the batch is rounded up to its bucket with inert rows (decode_batch_bucket)
                plan = plan_decode(seq_ids_list, list(decoding_seq_lens_list), input_ids_list, True,
                                   self.model_config.num_kv_heads, self._num_slots)
            else:
                plan = plan_batch(input_ids_list, seq_ids_list, decoding_seq_lens_list,
                                  self.model_config.num_kv_heads, self._num_slots, prefill_ctx_lens=prefill_ctx_lens)
            if graph_step:
                dev, t1, t2 = self._begin_step(plan, seq_ids_list, ignore_kvcache, opts)
                t3 = time.perf_counter()
                tokens = self._launch_replay(plan, dev, list(seq_ids_list), opts)
            else:
                if in_buckets:
                    plan.seq_block_size, plan.num_seq_blocks = graph_bucket(plan)
                tokens, (t1, t2, t3) = self._launch_eager(plan, seq_ids_list, ignore_kvcache, opts)
                tokens = tokens[:num_real]
                tap = self.post_layer.logits_tap
                if tap and plan.batch_size > num_real:      # (tests) a padded eager step: the real rows only, as on replay
                    tap[-1] = tap[-1][:num_real]
        t4 = time.perf_counter() if prof is not None else 0.0
        out = self._tokens_to_host(tokens, opts.scoring)
        self.replay.tokens_known(out)
        if prof is not None:
            t5 = time.perf_counter()
            sections = ((("launch", t4 - t0), ("lookahead_hits", 1.0)) if la is not None else      # (a hit: all of it is launch)
                        (("plan", t1 - t0), ("blocks", t2 - t1), ("upload", t3 - t2), ("launch", t4 - t3)))
            for name, dt in sections + (("wait_tokens", t5 - t4), ("calls", 1.0)):
                prof[name] = prof.get(name, 0.0) + dt
        return out

    def _forward_step_lora(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, ignore_kvcache, opts,
                           prefill_ctx_lens, lora_slots):
        """A step with at least one adapter row: the plain plan of the batch (never padded to a replay bucket), eager
        launches, the prepared look-ahead dropped; the row -> slot tiles go up in a buffer of their own."""
        self.replay.drop_prepared()
        num_real = len(input_ids_list)
        plan = plan_batch(input_ids_list, seq_ids_list, decoding_seq_lens_list,
                          self.model_config.num_kv_heads, self._num_slots, prefill_ctx_lens=prefill_ctx_lens)
        num_prefill = num_real - len(decoding_seq_lens_list)
        row_slots = rows_of_sequences(lora_slots, [len(ids) for ids in input_ids_list[:num_prefill]])
        lora = LoraStep(LoraBatch(row_slots, self.lora_store.max_loras, self.device, self._lora_staging),
                        self.lora_store.layers)
        tokens = self._launch_eager(plan, seq_ids_list, ignore_kvcache, opts, lora=lora)[0][:num_real]
        if self._host_prof is not None:
            self._host_prof["calls"] = self._host_prof.get("calls", 0.0) + 1.0
        return self._tokens_to_host(tokens, opts.scoring)

    @torch.inference_mode()
    def forward_verify(self, input_ids_list: List[List[int]], seq_ids_list: List[int],
                       ctx_lens: List[int], guides: Optional[List[Optional[object]]] = None) -> List[List[int]]:
        """One speculative-decoding verify step (greedy; no reference counterpart). Sequence s has `ctx_lens[s]` tokens
        resident in the KV pool and brings `input_ids_list[s]`: its last accepted token followed by its drafts,
        1 .. max_draft_tokens + 1 tokens. Returns, per sequence, the greedy token after EVERY one of its inputs: the
        caller keeps the longest prefix of drafts that equal the tokens before them (server/speculative.py: accept).
        All inputs' K/V are stored at positions [ctx, ctx + n); what a rejected draft wrote lies past the sequence's
        length afterwards, where every kernel masks it and the next step overwrites it.

        It is the chunked-prefill forward of the same arguments with three differences: the infer state is marked
        `verify`, attention is kernels/paged_attn.paged_attention_verify (the decode kernel's geometry, split over the
        total lengths), and every row is a last token. Eager launches, no hipGraph. A verify step scores nothing:
        `last_logprobs` is None afterwards. It takes no guides either (a verify step picks the argmax of the raw logits):
        `guides` with a cursor in it is refused."""
        self.last_logprobs = None
        if guides is not None and any(c is not None for c in guides):
            raise ValueError("forward_verify takes no guides: a guided sequence is never speculated")
        if len(input_ids_list) == 0:
            return []
        _require_hip_device()
        if len(seq_ids_list) != len(input_ids_list) or len(ctx_lens) != len(input_ids_list):
            raise ValueError("forward_verify needs one sequence id and one context length per sequence")
        limit = self.max_draft_tokens + 1
        if self.kv_fp8 or self.max_draft_tokens <= 0:
            raise RuntimeError("forward_verify is not available for this model: FP8 KV pools, or a q-head / kv-head ratio "
                               "the verify attention kernel does not take (G in {1, 2, 4, 8})")
        for sid, ids in zip(seq_ids_list, input_ids_list):
            if len(ids) == 0:
                raise ValueError(f"sequence {sid}: an empty token list (a verify step brings at least the last accepted "
                                 "token)")
            if len(ids) > limit:
                raise ValueError(f"sequence {sid}: {len(ids)} tokens, a verify step takes at most {limit} "
                                 f"(max_draft_tokens = {self.max_draft_tokens})")
        if self.gpu_block_manager is None or self.k_cache is None:
            raise RuntimeError("forward_verify before init_kvcache_and_swap: there is no KV pool to verify against")
        tracked = [sid for sid in seq_ids_list if sid in self._histories]
        if tracked:
            raise ValueError(f"forward_verify on sequences {tracked} whose logits are processed: a verify step picks the "
                             "argmax of the raw logits")
        ctx = [int(c) for c in ctx_lens]
        self._check_prefill_ctx(input_ids_list, seq_ids_list, [], False, ctx)     # (all-zero contexts pass: None)
        self.replay.drop_prepared()     # a prepared decode step does not survive a verify step
        self.gpu_block_manager.host.surplus_ok.update(seq_ids_list)     # rejected drafts leave their block with the sequence
        plan = plan_verify(input_ids_list, seq_ids_list, ctx, self.model_config.num_kv_heads, self._num_slots)
        flat = self._launch_eager(plan, seq_ids_list, scratch_rows=plan.num_tokens)[0].tolist()
        out, at = [], 0
        for ids in input_ids_list:
            out.append(flat[at:at + len(ids)])
            at += len(ids)
        return out

    def host_profile(self, reset: bool = True) -> dict:
        """Mean host seconds per forward() call by section (SWL_HOST_PROFILE=1), {} when profiling is off."""
        prof = self._host_prof or {}
        n = prof.get("calls", 0.0)
        out = {k: v / n for k, v in prof.items() if k != "calls"} if n else {}
        if reset and self._host_prof is not None:
            self._host_prof.clear()
        return out

    # ---- swapping ----------------------------------------------------------------------------------------
    def _swap(self, seq_ids_list: List[int], is_swap_in: bool):
        """Move every block of the given sequences between the GPU pool and the host swap pool.
        Reference: model.py:361-379. Block ids come from the host mirrors — no device read-back."""
        if len(seq_ids_list) == 0:
            return
        self.replay.drop_prepared()
        src_mgr = self.cpu_block_manager if is_swap_in else self.gpu_block_manager
        dst_mgr = self.gpu_block_manager if is_swap_in else self.cpu_block_manager
        counts = src_mgr.get_num_allocated_blocks_host(seq_ids_list)
        src_ids = [b for s in seq_ids_list for b in src_mgr.get_block_ids_host(s)]
        surplus = [s for s in seq_ids_list if s in src_mgr.host.surplus_ok]    # (a block of rejected drafts moves with its owner)
        src_mgr.gather_allocated_blocks_and_free(seq_ids_list)
        dst_mgr.host.surplus_ok.update(surplus)
        dst_mgr.allocate_blocks_for_seqs(seq_ids_list, [c * self.engine_config.block_size for c in counts])
        dst_ids = [b for s in seq_ids_list for b in dst_mgr.get_block_ids_host(s)]
        swap_blocks(src_ids, dst_ids, is_swap_in, self.k_cache, self.v_cache, self.k_swap, self.v_swap)

    @torch.inference_mode()
    def swap_in_seqs(self, seq_ids_list: List[int]):
        """Bring the sequences' KV blocks back from the host swap pool."""
        self._swap(seq_ids_list, True)

    @torch.inference_mode()
    def swap_out_seqs(self, seq_ids_list: List[int]):
        """Evict the sequences' KV blocks to the host swap pool."""
        self._swap(seq_ids_list, False)

    @torch.inference_mode()
    def free_seqs_resources(self, seq_ids_list: List[int]):
        """Release everything the sequences hold, on both pools. Reference: model.py:402-408."""
        if len(seq_ids_list) == 0:
            return
        self.replay.drop_prepared()
        for sid in seq_ids_list:
            self._histories.pop(sid, None)
        self.gpu_block_manager.free_blocks_for_seqs(seq_ids_list)
        self.cpu_block_manager.free_blocks_for_seqs(seq_ids_list)

    # ---- prefix reuse by block copy --------------------------------------------------------------------------
    @torch.inference_mode()
    def copy_kv_prefix(self, src_seq_ids: List[int], dst_seq_ids: List[int], num_tokens: List[int]):
        """The first num_tokens[i] tokens of sequence src_seq_ids[i] become the first num_tokens[i] tokens of sequence
        dst_seq_ids[i]: the destination gets num_tokens[i] / block_size blocks of its own and the source's blocks are copied
        into them, K and V, by ONE launch on the current stream (csrc/kv_copy.hip; one upload of the id lists, no host
        sync). Whole blocks only; a destination owns nothing before the call. Afterwards
        `forward([rest], [dst], [], prefill_ctx_lens=[num_tokens])` continues the destination behind the copied context.
        Everything is refused on the host (ValueError / RuntimeError) before anything is allocated or launched. Stream
        order makes reuse safe: a source freed by a later call is not overwritten before the copy has read it. Token
        histories are not copied: a sequence whose logits are processed prefills whole (forward refuses it otherwise)."""
        if self.gpu_block_manager is None or self.k_cache is None:
            raise RuntimeError("copy_kv_prefix before init_kvcache_and_swap: there is no KV pool")
        if not (len(src_seq_ids) == len(dst_seq_ids) == len(num_tokens)):
            raise ValueError(f"copy_kv_prefix needs lists of one length, got {len(src_seq_ids)} sources, "
                             f"{len(dst_seq_ids)} destinations and {len(num_tokens)} token counts")
        if len(src_seq_ids) == 0:
            return
        bs = self.engine_config.block_size
        mgr = self.gpu_block_manager
        src_seq_ids, dst_seq_ids = [int(s) for s in src_seq_ids], [int(d) for d in dst_seq_ids]
        num_tokens = [int(n) for n in num_tokens]
        sources = set(src_seq_ids)
        if len(set(dst_seq_ids)) != len(dst_seq_ids):
            raise ValueError(f"copy_kv_prefix names a destination twice: {dst_seq_ids}")
        for src, dst, n in zip(src_seq_ids, dst_seq_ids, num_tokens):
            if n <= 0 or n % bs:
                raise ValueError(f"copy_kv_prefix copies whole blocks: num_tokens must be a positive multiple of {bs}, "
                                 f"got {n}")
            if dst in sources:
                raise ValueError(f"copy_kv_prefix: sequence {dst} is a destination and a source")
            if not 0 <= dst < mgr.host.max_seqs:
                raise RuntimeError(f"sequence id {dst} outside the block table (0..{mgr.host.max_seqs - 1})")
            if mgr.host.num_allocated(src) < n // bs:
                raise ValueError(f"copy_kv_prefix: source sequence {src} owns {mgr.host.num_allocated(src)} GPU blocks, "
                                 f"{n} tokens need {n // bs}")
            if mgr.host.num_allocated(dst):
                raise ValueError(f"copy_kv_prefix: destination sequence {dst} already owns "
                                 f"{mgr.host.num_allocated(dst)} blocks")
        src_blocks = [b for src, n in zip(src_seq_ids, num_tokens) for b in mgr.get_block_ids_host(src)[:n // bs]]
        self.replay.drop_prepared()
        mgr.allocate_blocks_for_seqs(dst_seq_ids, num_tokens)      # (raises before it commits when the pool is short)
        dst_blocks = [b for dst in dst_seq_ids for b in mgr.get_block_ids_host(dst)]
        if len(dst_blocks) != len(src_blocks) or not sources.isdisjoint(dst_seq_ids) or set(dst_blocks) & set(src_blocks):
            raise RuntimeError("copy_kv_prefix: the destinations' new blocks overlap the sources' (allocator state corrupt)")
        d_src, d_dst = mgr._upload(np.asarray(src_blocks, dtype=np.int32), np.asarray(dst_blocks, dtype=np.int32))
        kv_copy_blocks(self.k_cache, self.v_cache, d_src, d_dst)
