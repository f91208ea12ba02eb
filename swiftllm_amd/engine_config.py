"""EngineConfig — the engine-level knobs, field-compatible with the reference.

Mirrors swiftllm/engine_config.py:4-84: the nine original fields keep their names, order and
meaning so `EngineConfig(**vars(args))` (reference api_server.py:97) and the keyword construction in
examples/offline.py:22-33 keep working. Fields after `max_tokens_in_batch` are additions of this
MI355X implementation and all have defaults.

Defaults are re-sized for one MI355X (288 GB HBM3E): the reference's CLI defaults target 24-80 GB
parts (num_cpu_blocks 2048 = 4 GiB of swap for Llama-3-8B); here the swap pool default is 16 Ki
blocks and the scheduler limits admit the larger KV pool.
"""
import argparse
import dataclasses


@dataclasses.dataclass
class EngineConfig:
    # Model loading parameters
    model_path: str
    use_dummy: bool

    # PagedAttention-related parameters
    block_size: int
    gpu_mem_utilization: float
    num_cpu_blocks: int
    max_seqs_in_block_table: int
    max_blocks_per_seq: int

    # Scheduling-related parameters
    max_batch_size: int
    max_tokens_in_batch: int

    # ---- MI355X additions (all optional) -------------------------------------------------------
    # Storage/compute dtype of weights, activations and the KV pool. The reference hard-codes
    # float16 (model.py:70,147); bfloat16 is the headline precision on MI355X. NOTE: float16 keeps the reference's
    # rounding points everywhere, so the bfloat16-only deferred norm (defer_rmsnorm, tiny_decode_batches) is off for it;
    # since r06c its row-owned projections run the EXACT norm on the fly instead (rows_decode: the same 5-6 launches per
    # layer with fused_add_rmsnorm's arithmetic — 3.95 vs 4.10 ms per step at batch 32, 3.11 vs 3.25 at batch 1).
    dtype: str = "float16"
    # One [h + 2*KVH*D, h] GEMM instead of three (the reference left this commented out,
    # weight.py:131). fuse_qkv=False + use_skinny_gemm=False reproduces the reference's exact BLAS calls.
    fuse_qkv: bool = True
    # Capture pure-decode forwards into hipGraphs (one per batch size and split-geometry bucket) and replay them: one
    # graph launch per step instead of ~230 kernel launches (batch 32: 4.0 vs 4.35 ms/step on MI355X). The default;
    # False (CLI: --no-hip-graph) launches every kernel from Python.
    use_hip_graph: bool = True
    # Route decode-sized projections (<= 32 tokens) to the hand-written weight-streaming MFMA GEMM
    # instead of hipBLASLt (prefill-sized calls stay on the BLAS).
    use_skinny_gemm: bool = True
    # Keep a second copy of the projection weights in MFMA-fragment order for the decode GEMMs (+1x projection
    # weights in HBM, ~8 % faster weight streaming; the row-major copy stays for prefill).
    pack_decode_weights: bool = True
    # Overrides of the internal decode-path switches below (TUNING_DEFAULTS), e.g. tuning={"defer_rmsnorm": False}: every
    # one of them selects between two parity-tested implementations of the same arithmetic and defaults to the faster one;
    # they exist so that tests and A/B measurements can hold one path against the other, not as deployment knobs.
    tuning: dict = None
    # Chunked prefill: > 0 caps the PROMPT tokens of one step at min(max_prefill_chunk, max_tokens_in_batch) in total; a
    # longer prompt is fed over several steps (each chunk attends to the paged KV cache: csrc/prefill_attn_paged.hip),
    # running decodes ride along with every chunk step when the scheduler piggybacks, and a prompt longer than
    # max_tokens_in_batch becomes servable. 0 (default): off — a prompt is one forward, as in the reference.
    max_prefill_chunk: int = 0
    # Element type of the paged KV pools (GPU and host swap). "auto": the activation dtype — nothing changes. "fp8_e4m3":
    # OCP e4m3fn, one byte per element with one fp32 k_scale / v_scale per (layer, kv-head) (LlamaModel.set_kv_scales;
    # default 1): the pool holds twice the tokens and decode attention streams half the bytes (csrc/paged_attn_fp8.hip).
    # The layer then runs qkv projection -> rotary -> quantising store -> FP8 paged attention: the slab-fed attention
    # prologue and the paths that hang on it are 16-bit only.
    kv_cache_dtype: str = "auto"
    # Prompt-lookup speculative decoding (server/speculative.py): drafts per sequence per step, taken from the request's
    # own prompt + output by n-gram match and verified in ONE forward (LlamaModel.forward_verify; attention:
    # csrc/paged_attn_verify.hip). 0 (default): off — every step launches what it always did. The effective value is capped
    # by the model (16 / (q heads per kv head) - 1 drafts: 3 at Llama-3-8B). Greedy requests, pure-decode steps, 16-bit pools.
    speculative_ngram: int = 0
    # ... and only for decode batches of at most this many requests: with 3 drafts, 8 x 4 = 32 rows keep every projection
    # of the verify forward inside the weight-streaming GEMMs' range (kernels/linear.py: <= 32 tokens).
    speculative_max_batch: int = 8
    # Multi-LoRA serving (worker/lora.py, csrc/lora.hip): adapter slots resident next to the base weights. 0 (default): off —
    # nothing is allocated and every step launches what it always did. > 0: load_weights allocates zero-filled slot stacks
    # for every projection of every layer (before the KV pool is sized) for adapters of rank <= max_lora_rank (8, 16, 32 or
    # 64), and a request may name an adapter; a step with an adapter row runs the straight-line LoRA layer path, eagerly
    # (16-bit KV pools only). lora_modules: "NAME=PATH" PEFT directories load_weights loads.
    max_loras: int = 0
    max_lora_rank: int = 16
    lora_modules: list = None
    # Guided decoding (swiftllm_amd/guided, csrc/guided.hip): rows of the device pool of per-state
    # token bitmasks, one row (ceil(vocab / 32) int32 words: 16 KiB at Llama-3's vocabulary) per DFA state of a resident
    # guide. 0 (default): off — no pool, no new code path, and a guided request is answered with an error. > 0: load_weights
    # allocates the pool and the vocabulary's flat device form (from model_path/tokenizer.json, or
    # LlamaModel.set_guide_vocab) before the KV pool is sized; a request may then be held to a regex, a choice or a set of
    # token ids (SamplingParams.guided_regex / guided_choice / allowed_token_ids).
    guided_max_states: int = 0
    # Prefix caching by KV block copy (server/prefix_cache.py, csrc/kv_copy.hip). False (default):
    # off — every step launches what it always did. True: a finished request keeps its block-table row and its blocks as a
    # cache entry (reclaimed, least recently used first, whenever the scheduler needs the blocks, a row or an entry slot); a
    # new prompt whose leading whole blocks equal an entry's gets private COPIES of those blocks (one launch) and prefills
    # only the rest behind them, as a chunk behind a context — so it needs max_prefill_chunk > 0. Requests with a LoRA
    # adapter or processed logits neither hit nor donate. prefix_cache_max_seqs: block-table rows the cache may hold.
    enable_prefix_caching: bool = False
    prefix_cache_max_seqs: int = 256

    # Internal switches (all on): set through `tuning`, read by the layer code as plain attributes.
    TUNING_DEFAULTS = dict(
        fuse_rope_kvstore=True,         # rotary + KV store in one launch (decode tokens; r05: prompt tokens too, one pass over k)
        fuse_splitk_consumers=True,     # the next kernel sums a projection's split-K slabs (no reduce launches)
        fuse_rope_into_attention=True,  # ... and rotary + KV store run in the paged-attention kernel's prologue
        # apply the RMSNorm scale AFTER the projection that consumes the normalised activations (a per-token scalar), so the
        # residual-add + norm consumers become element-wise kernels that fill the chip; bfloat16 only
        # (kernels/rmsnorm.py: deferred_norm_ok), hidden % 1024 == 0, batches of <= 32 sequences
        defer_rmsnorm=True,
        # batches of <= 2 sequences: the qkv and up/gate projections sum the previous projection's slabs themselves
        # (csrc/gemm_tiny.hip), 5 launches per layer instead of 7
        tiny_decode_batches=True,
        # decode batches of <= 32 sequences: o_proj — and down_proj up to 16 sequences — finish their rows INSIDE the
        # workgroup that owns them (csrc/gemm_rows.hip: K split across the 8 waves, residual add in the epilogue: no slabs,
        # no consumer launch), and the projection that follows applies the norm weight and the 1/rms itself while it stages
        # the raw residual rows ("norm on the fly", gemm_skinny.hip NF: bfloat16, deferred 1/rms; NX: either dtype, the exact
        # norm from the per-tile sums of squares the row-owned kernel leaves): 6 launches per layer at batch 32, 5 up to 16
        rows_decode=True,
        # ONE decoding sequence: the whole transformer stack of the step as one persistent launch (csrc/decode_engine.hip: a
        # loader wave per CU streams that CU's rows of every projection by LDS-DMA, three consumer waves compute, operator
        # boundaries are in-launch granule hand-offs; the reference's rounding points in BOTH dtypes; every wait bounded).
        # OFF by default: measured on MI355X at Llama-3-8B it is parity-green and SLOWER than the 5-6 launches it replaces
        # (3.29 vs 3.03 ms per step at context 1088: its six all-to-all hand-offs per layer cost ~40 us of which the 7-slot
        # LDS ring covers ~12, the launch seams they replace ~27 — DESIGN.md section 4.9, profiles/r06_engine_*). Costs a
        # third copy of the layer weights (13.9 GB for Llama-3-8B) when on.
        decode_engine=False,
        pin_swap_memory=True,           # host swap pool in pinned memory (falls back to pageable when the host refuses)
        # the serving loop (server/engine.py) keeps the interpreter's cyclic collector out of its busy iterations: the model's
        # long-lived objects are frozen out of the collector's working set when the loop starts, young generations are
        # collected when the loop goes idle (or every 256 busy iterations), a full collection every 4096 — what bench.py's
        # timed region does around its K steps (the benchmark measures what the server does)
        pause_gc_while_serving=True,
    )

    # Tokens per KV block the HIP kernels are built for (csrc/paged_attn.hip kBlk, kvcache.hip): one 16-token block
    # of a 128-wide head is 4 KiB = one wave-wide 16 B/lane load x 4.
    SUPPORTED_BLOCK_SIZE = 16
    KV_CACHE_DTYPES = ("auto", "fp8_e4m3")
    LORA_RANKS = (8, 16, 32, 64)

    def __post_init__(self):
        # The reference takes block_size as a Triton constexpr (paged_attn.py:27) and its CLI default is 16
        # (engine_config.py:37-42). Here the block is a compile-time tile; anything else is refused on the host,
        # before any memory is allocated, instead of surfacing as SWL_ERR_UNSUPPORTED from the first decode step.
        if int(self.block_size) != self.SUPPORTED_BLOCK_SIZE:
            raise ValueError(
                f"block_size={self.block_size} is not supported: the MI355X kernels are built for "
                f"{self.SUPPORTED_BLOCK_SIZE}-token KV blocks (pass --block-size {self.SUPPORTED_BLOCK_SIZE})")
        if self.dtype not in ("float16", "bfloat16"):
            raise ValueError(f"dtype must be 'float16' or 'bfloat16', got {self.dtype!r}")
        if int(self.max_prefill_chunk) < 0:
            raise ValueError(f"max_prefill_chunk must be >= 0 (0 = off), got {self.max_prefill_chunk}")
        if self.kv_cache_dtype not in self.KV_CACHE_DTYPES:
            raise ValueError(f"kv_cache_dtype must be one of {list(self.KV_CACHE_DTYPES)}, got {self.kv_cache_dtype!r}")
        if int(self.speculative_ngram) < 0:
            raise ValueError(f"speculative_ngram must be >= 0 (0 = off), got {self.speculative_ngram}")
        if int(self.speculative_max_batch) < 0:
            raise ValueError(f"speculative_max_batch must be >= 0, got {self.speculative_max_batch}")
        if int(self.max_loras) < 0:
            raise ValueError(f"max_loras must be >= 0 (0 = off), got {self.max_loras}")
        if int(self.max_lora_rank) not in self.LORA_RANKS:
            raise ValueError(f"max_lora_rank must be one of {list(self.LORA_RANKS)}, got {self.max_lora_rank}")
        if self.lora_modules:
            if int(self.max_loras) <= 0:
                raise ValueError("lora_modules needs max_loras > 0")
            names = [str(m).partition("=")[0] for m in self.lora_modules]
            if any("=" not in str(m) or not n or not str(m).partition("=")[2] for m, n in zip(self.lora_modules, names)):
                raise ValueError(f"lora_modules entries are 'NAME=PATH' strings, got {list(self.lora_modules)}")
            if len(set(names)) != len(names):
                raise ValueError(f"lora_modules names an adapter twice: {names}")
            if len(names) > int(self.max_loras):
                raise ValueError(f"lora_modules names {len(names)} adapters, max_loras is {self.max_loras}")
        if isinstance(self.guided_max_states, bool) or int(self.guided_max_states) < 0:
            raise ValueError(f"guided_max_states must be an integer >= 0 (0 = off), got {self.guided_max_states!r}")
        if self.enable_prefix_caching:
            if int(self.max_prefill_chunk) == 0:
                raise ValueError("enable_prefix_caching needs max_prefill_chunk > 0: a prompt that reuses a cached prefix "
                                 "is a prompt chunk behind a context")
            if not 1 <= int(self.prefix_cache_max_seqs) < int(self.max_seqs_in_block_table):
                raise ValueError(f"prefix_cache_max_seqs must be in [1, max_seqs_in_block_table = "
                                 f"{self.max_seqs_in_block_table}), got {self.prefix_cache_max_seqs}")
        elif int(self.prefix_cache_max_seqs) < 1:
            raise ValueError(f"prefix_cache_max_seqs must be >= 1, got {self.prefix_cache_max_seqs}")
        unknown = set(self.tuning or ()) - set(self.TUNING_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown tuning switches {sorted(unknown)}; known: {sorted(self.TUNING_DEFAULTS)}")
        for name, default in self.TUNING_DEFAULTS.items():
            setattr(self, name, bool((self.tuning or {}).get(name, default)))
        if self.kv_cache_dtype == "fp8_e4m3" and self.decode_engine:
            raise ValueError("kv_cache_dtype='fp8_e4m3' cannot be combined with tuning={'decode_engine': True}: the "
                             "persistent one-sequence decode step reads and writes 16-bit KV pools only")
        if int(self.max_loras) > 0 and self.kv_cache_dtype == "fp8_e4m3":
            raise ValueError("max_loras > 0 cannot be combined with kv_cache_dtype='fp8_e4m3': the LoRA layer path stores "
                             "and attends 16-bit KV pools only")
        if int(self.max_loras) > 0 and self.decode_engine:
            raise ValueError("max_loras > 0 cannot be combined with tuning={'decode_engine': True}: the persistent "
                             "one-sequence decode step has no adapter path")
        if int(self.speculative_ngram) > 0 and self.kv_cache_dtype == "fp8_e4m3":
            raise ValueError("speculative_ngram > 0 cannot be combined with kv_cache_dtype='fp8_e4m3': the verify "
                             "attention kernel reads 16-bit KV pools only")
        if self.enable_prefix_caching and self.decode_engine:
            raise ValueError("enable_prefix_caching cannot be combined with tuning={'decode_engine': True}")
        if int(self.speculative_ngram) > 0 and self.decode_engine:
            raise ValueError("speculative_ngram > 0 cannot be combined with tuning={'decode_engine': True}: a verify step "
                             "is a multi-row forward the persistent one-sequence decode step does not run")

    @staticmethod
    def add_cli_args(parser: argparse.ArgumentParser):
        """Add the engine's CLI flags (same flag names as the reference, engine_config.py:25-84)."""
        g = parser.add_argument_group("swiftllm engine")
        g.add_argument("--model-path", type=str, required=True,
                       help="Directory holding config.json and the weights (no downloading)")
        g.add_argument("--use-dummy", action="store_true",
                       help="Random weights instead of loading a checkpoint (profiling)")
        g.add_argument("--block-size", type=int, default=16, help="Tokens per KV block")
        g.add_argument("--gpu-mem-utilization", type=float, default=0.97,
                       help="Fraction of HBM the weights + KV pool may occupy")
        g.add_argument("--num-cpu-blocks", type=int, default=16384,
                       help="Blocks in the host swap pool")
        g.add_argument("--max-seqs-in-block-table", type=int, default=4096,
                       help="Rows of the device block table")
        g.add_argument("--max-blocks-per-seq", type=int, default=32768,
                       help="Columns of the device block table")
        g.add_argument("--max-batch-size", type=int, default=512,
                       help="Sequences per forward, at most")
        g.add_argument("--max-tokens-in-batch", type=int, default=32768,
                       help="Tokens per forward, at most")
        g.add_argument("--dtype", type=str, default="float16", choices=["float16", "bfloat16"])
        g.add_argument("--no-fuse-qkv", dest="fuse_qkv", action="store_false")
        g.add_argument("--use-hip-graph", dest="use_hip_graph", action="store_true", default=True,
                       help="(default) replay captured hipGraphs for pure-decode steps")
        g.add_argument("--no-hip-graph", dest="use_hip_graph", action="store_false")
        g.add_argument("--no-skinny-gemm", dest="use_skinny_gemm", action="store_false")
        g.add_argument("--kv-cache-dtype", type=str, default="auto", choices=list(EngineConfig.KV_CACHE_DTYPES),
                       help="Element type of the KV pools: auto = the activation dtype, fp8_e4m3 = 1 byte per element")
        g.add_argument("--speculative-ngram", type=int, default=0,
                       help="Prompt-lookup speculative decoding: n-gram drafts per sequence per step (0 = off)")
        g.add_argument("--speculative-max-batch", type=int, default=8,
                       help="Speculate only in decode steps of at most this many requests")
        g.add_argument("--max-loras", type=int, default=0,
                       help="Multi-LoRA serving: adapter slots resident next to the base weights (0 = off)")
        g.add_argument("--max-lora-rank", type=int, default=16, choices=list(EngineConfig.LORA_RANKS),
                       help="Largest adapter rank a slot holds (lower ranks are zero-padded)")
        g.add_argument("--lora", dest="lora_modules", action="append", default=None, metavar="NAME=PATH",
                       help="A PEFT adapter directory to load at start-up under NAME (repeatable)")
        g.add_argument("--max-prefill-chunk", type=int, default=0,
                       help="Chunked prefill: prompt tokens per forward, at most (0 = off: a prompt is one forward)")
        g.add_argument("--enable-prefix-caching", dest="enable_prefix_caching", action="store_true",
                       help="Prefix caching by KV block copy: finished requests donate their whole blocks to later "
                            "prompts with the same leading tokens (needs --max-prefill-chunk > 0)")
        g.add_argument("--prefix-cache-max-seqs", type=int, default=256,
                       help="Block-table rows the prefix cache may hold (below --max-seqs-in-block-table)")
        g.add_argument("--guided-max-states", type=int, default=0,
                       help="Guided decoding: rows of the device pool of per-state token bitmasks (0 = off); needs "
                            "tokenizer.json in --model-path")
