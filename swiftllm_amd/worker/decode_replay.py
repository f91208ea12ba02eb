"""hipGraph replay of pure-decode steps and the decode look-ahead: the captured graphs, the step prepared behind the running
one, and the two rules by which either is forgotten (DecodeReplay) — next to the planning both key on: the batch and split
buckets of a replayed step (`decode_batch_bucket`, `graph_bucket`, `plan_decode`) and the plan's one upload (`stage_plan`)."""
import time
from typing import List

import torch

from .batch_plan import BatchPlan, plan_batch
from .step_logits import PLAIN, StagedInts, StepLogits


def graph_bucket(plan: BatchPlan):
    """Captured launch geometry must cover every replay, and the number of distinct geometries a long-running
    server meets must stay small (every new one costs a warm-up run + a capture, and memory): the split width
    — `select_seq_block_size` drifts in 64-token steps as sequences grow — is rounded up to a multiple of
    1/16..1/32 of itself (at most 16 widths per octave), and the split count is taken for the longest sequence
    rounded up to its next 64-token boundary and then to a power of two (surplus workgroups exit on their first
    instruction). A single split stays a single split (its width only has to cover the longest sequence).
    (r01/r02 rounded the width to a POWER of two: at Llama-2-7B dims, 4 x 16.4k tokens, that turned the balanced
    8256 + 8139 split into 16384 + 11 — half the workgroups idle, the attention kernel 224 instead of 175 us and
    graph replay 12 % slower than eager launches.)"""
    sbs = int(plan.seq_block_size)
    if plan.num_seq_blocks > 1:
        quantum = max(64, 1 << max(0, sbs.bit_length() - 5))
        sbs = -(-sbs // quantum) * quantum
    horizon = -(-(plan.max_decoding_len + 1) // 64) * 64
    nsb_cap = -(-horizon // sbs)
    if nsb_cap > 1:
        nsb_cap = 1 << (nsb_cap - 1).bit_length()
    else:
        # one split: any width >= the longest sequence is the same launch; key on a power of two of it
        sbs = max(256, 1 << (horizon - 1).bit_length())
    return sbs, nsb_cap


def decode_batch_bucket(batch: int) -> int:
    """Captured batch size that serves a pure-decode batch of `batch` sequences. The replay cache is keyed on the batch
    size, and a server's batch drifts by one sequence at a time: keyed on the EXACT size (r01-r04) every new size paid a
    warm-up forward plus a capture. Sizes are rounded up — to a multiple of 8 up to 32 sequences, of 16 up to 64, of 32
    beyond (the projections' cost moves in 32-token blocks there) — and the surplus rows are INERT: length-0 sequences, which every
    decode kernel treats as a no-op (paged attention: the workgroup exits before its prologue; rotary / KV store: nothing
    read, nothing stored; the projections, norms and the sampler are row-independent, so whatever an inert row holds
    never reaches a real one). 1 and 2 stay exact (their own launch path). The reference has no graphs
    (swiftllm/worker/model.py:228-249 launches eagerly); results are those of the exact-size launch."""
    if batch <= 2:
        return batch
    # r06b: 16 between 32 and 64 (the medium kernels serve two token blocks whatever the count), 32 beyond 64 (the wide
    # GEMMs and the library work in 32-token blocks: 129 -> 160 costs what 144 did) — 14 buckets up to 256 instead of 22
    step = 8 if batch <= 32 else 16 if batch <= 64 else 32
    return -(-batch // step) * step


def plan_decode(seq_ids_list: List[int], lens: List[int], tokens, pad: bool, num_kv_heads: int, num_slots: int) -> BatchPlan:
    """Plan of a pure-decode step; `pad`: rounded up to its batch bucket with inert rows (token 0, length 0)."""
    b = len(lens)
    bp = decode_batch_bucket(b) if pad else b
    ids = tokens if tokens is not None else [(0,)] * b
    if bp > b:
        ids = list(ids) + [(0,)] * (bp - b)
        seq_ids_list = list(seq_ids_list) + [seq_ids_list[0]] * (bp - b)
        lens = list(lens) + [0] * (bp - b)
    plan = plan_batch(ids, seq_ids_list, lens, num_kv_heads, num_slots)
    plan.num_real_seqs = b
    return plan


def stage_plan(ints: StagedInts, plan: BatchPlan, floor: int = 0) -> dict:
    """Pack the plan's int32 arrays into the pinned side of `ints` and ship them with one async H2D copy; returns the
    device views by name. `floor`: words the buffer holds at least (its first capacity)."""
    layout, total = plan.packed_layout()
    ints.ensure(max(total, floor))
    plan.pack_into(ints.begin())
    ints.ship([(0, total)])
    return {name: ints.staged[off:off + n] for name, off, n in layout}


class _DecodeGraph:
    """A captured pure-decode forward for one batch size."""
    __slots__ = ("graph", "out_tokens", "logits")


class _DecodeLookahead:
    """Everything the NEXT decode step of the same batch needs, prepared while the GPU was still busy with this one."""
    __slots__ = ("seq_ids", "lens", "tokens", "plan", "dev", "logits")

    def __init__(self):
        self.logits = PLAIN     # the StepLogits of the step it was prepared behind


class DecodeReplay:
    """One per model: the captured decode graphs (`graphs`, LRU, with their shared pool, the warmed buckets, `captures` and
    `capture_s`) and the one prepared next step (`prepared`). Both point into device memory they do not own; replayed after
    that memory moved or changed its meaning they read freed or stale memory. Two ways to forget, neither implies the other:
      drop_graphs()    a buffer the graphs read BY ADDRESS moved, or what they were captured against is gone: a staged
                       buffer grew (the plan's or a logits option's: StagedInts.on_move), the flash-decoding scratch grew
                       (_make_infer_state), the KV pools were rebuilt (init_kvcache_and_swap), the one-sequence engine
                       failed (_engine_failed), the sizing run ended (_measure_decode_graph_bytes: workspaces grown on a
                       throw-away pool), a tool flips a live model between configurations.
      drop_prepared()  the prepared plan, or the block table behind it, no longer describes the next call: blocks moved or
                       went (swap in / out, free_seqs_resources, copy_kv_prefix, init_kvcache_and_swap, the sizing run),
                       the K/V codes change meaning (set_kv_scales), another kind of step overwrote the plan's buffer or
                       must run eagerly (forward_verify, a LoRA step, a step under the mixture-of-experts tap), the
                       engine failed and the step is repeated. Every forward drops it too, by `take`: it serves the very
                       next call or none — so a step that moves the plan's buffer has always forgotten it first.
    It reaches the model through what it is given: `stage_eager(plan, dev, opts)` readies one eager decode step — sizing
    its workspaces, which may drop the graphs and so must not happen while the stream is capturing — and returns the
    launch (no arguments; enqueues the step, returns its token tensor); `plan_next(seq_ids, lens)` plans that padded
    pure-decode step (None: past the rotary table); `plan_ints`: the plan's staged buffer; `engine_config.use_hip_graph`."""

    # LRU bound of the replay cache. Since r06b a cached graph pins only its sampled-token tensor in the shared pool (the
    # [B, vocab] logits are kept only under a test's tap), so the bound is about host-side graph objects, not HBM. 48 (r05)
    # thrashed under a serving sweep with ShareGPT-like lengths at max batch 256: 14 batch buckets x ~5 single-split widths
    # + the split geometries of small batches = well over 100 live keys, 23-53 captures per 1000 forwards at 40-200 req/s
    # (profiles/r06b_serve_sweep_sharegpt_*.jsonl).
    max_graphs = 256

    def __init__(self, stage_eager, plan_next, plan_ints: StagedInts, engine_config):
        self.stage_eager, self.plan_next, self.plan_ints, self.engine_config = stage_eager, plan_next, plan_ints, engine_config
        self.graphs = {}        # (batch, split width, split count, logits kept) + StepLogits.flags -> _DecodeGraph, LRU order
        self.pool = None
        self.warmed = set()
        self.captures = 0       # hipGraph captures so far (the first at a batch bucket = one warm-up forward + one capture)
        self.capture_s = 0.0    # host seconds spent in them
        self.prepared = None    # _DecodeLookahead of the step that is expected next (graph replay only)
        self.lookahead = True   # (tests switch it off to hold the fast path to the plain one)
        self.eager_in_buckets = False   # tests: eager launches at the replay path's batch bucket and split geometry

    on = property(lambda self: getattr(self.engine_config, "use_hip_graph", False))    # (read at every use: tools flip it)

    def drop_graphs(self):
        """Forget every captured decode graph (their buffers moved, or the pool / engine they were captured against is gone)
        AND the private memory pool they shared. The pool handle must go with them: once its last graph is destroyed the
        caching allocator marks the pool freeable (use_count 0) but keeps it on its books until the next cache flush, and a
        new capture into that id trips `it->second->use_count > 0` (HIPCachingAllocator.cpp) — met in r06 by the serving
        sweep (tools/serve_bench.py --sweep: the flash-decoding scratch grew after graphs had been captured) and by
        bench.py's engine leg. The next capture opens a fresh pool; the old one's memory returns to the device on the
        allocator's next flush."""
        self.graphs.clear()
        self.pool = None
        self.warmed.clear()     # (workspaces may have been re-sized: warm up again before the next capture)

    def drop_prepared(self):
        self.prepared = None

    def run(self, plan: BatchPlan, dev: dict, opts: StepLogits, use_engine: bool, post) -> torch.Tensor:
        """Replay the graph of this step, capturing it first when its geometry is new; returns the real sequences' tokens.
        `use_engine`: the step runs on the persistent one-sequence engine; `post`: the post layer (its logits tap)."""
        sbs, nsb_cap = graph_bucket(plan)
        tap = post.logits_tap
        tap_len = len(tap) if tap is not None else 0
        # (the engine has one launch geometry; a graph captured while a test taps the logits keeps its [B, vocab] tensor
        # alive in the shared pool, one captured without the tap does not — up to 65 MB per graph at 256 sequences)
        # (each logits option in use makes the step a graph of its own: StepLogits.flags; plain graphs are as they were)
        key = ((1, 0, 0) if use_engine else (plan.batch_size, sbs, nsb_cap)) + (tap is not None,) + opts.flags
        entry = self.graphs.pop(key, None)
        plan.seq_block_size, plan.num_seq_blocks = sbs, nsb_cap
        if entry is None:
            self.captures += 1
            t_cap = time.perf_counter()
            launch = self.stage_eager(plan, dev, opts)
            # one eager run on a side stream first (library handles, workspaces, allocator pools): nothing may be lazily
            # initialised while the stream is capturing. Once per BATCH BUCKET (r06b): a new split geometry at a batch size
            # that has been captured before launches the same kernels on the same shapes — only the attention grid moves.
            warm_key = (key[0], use_engine, tap is not None) + opts.flags
            if warm_key not in self.warmed:
                warm = torch.cuda.Stream()
                warm.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(warm):
                    launch()
                torch.cuda.current_stream().wait_stream(warm)
                self.warmed.add(warm_key)
            while len(self.graphs) >= self.max_graphs:      # least recently used first
                self.graphs.pop(next(iter(self.graphs)))
            if self.pool is None:
                # ONE private memory pool for all captures: graphs never run concurrently (one stream), so they can
                # share their activation memory instead of each pinning its own after the KV pool took the rest
                self.pool = torch.cuda.graph_pool_handle()
            entry = _DecodeGraph()
            entry.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(entry.graph, pool=self.pool):
                entry.out_tokens = launch()
            entry.logits = post.last_logits if tap is not None else None
            if tap is None:
                post.last_logits = None         # (drop the last reference: the buffer returns to the shared pool)
            if tap is not None:
                del tap[tap_len:]               # what the warm-up run and the capture appended
            self.capture_s += time.perf_counter() - t_cap
        self.graphs[key] = entry                # (re)inserted last = most recently used
        entry.graph.replay()
        n = plan.real_seqs
        if tap is not None:                     # (tests) one entry per forward, as on the eager path; a copy: the
            tap.append(entry.logits[:n].clone())    # graph's own tensor is overwritten by the next replay
        return entry.out_tokens[:n]

    # ---- decode look-ahead: the host side of step k+1 runs while the GPU executes step k ---------------------------------
    def prepare_next(self, plan: BatchPlan, seq_ids_list: List[int], tokens_dev: torch.Tensor, opts: StepLogits = PLAIN):
        """Called right after the graph of a pure-decode step was launched, before the host blocks on its tokens. A
        generation loop calls forward again with the same sequences, every length + 1 and the tokens just sampled: plan
        that step now (numpy) and enqueue — behind the running graph, on the same stream — the H2D copy of its metadata and
        a device copy of the sampled tokens into its input-id slots. If the next call is that step (`take` checks), it
        only takes its KV blocks and launches: ~40 us of host work per step the GPU no longer waits for
        (tools/host_overhead.py: plan 18 + upload 24 us at batch 32). If it is not, nothing is lost: the ordinary path
        re-plans and re-uploads. (Blocks are NOT taken early: a scheduler that counts the pool down to its last block must
        find the allocator exactly where its own books say it is.) Nothing is prepared with look-ahead off, or past the rotary table."""
        if not self.lookahead:
            return
        b = plan.real_seqs
        next_lens = [n + 1 for n in plan.seq_lengths_list[:b]]
        nxt = self.plan_next(seq_ids_list, next_lens)
        if nxt is None:
            return
        # (through the plan's own pinned buffer: its last copy, this step's upload or the previous look-ahead's, was
        # enqueued ahead of the graph just launched and is long done — `begin` waits for nothing)
        dev = stage_plan(self.plan_ints, nxt)
        dev["input_ids"][:b].copy_(tokens_dev)  # int64 -> int32 on the device: the host has not seen them yet (inert rows: 0)
        la = _DecodeLookahead()     # (`logits`: what the next step must continue, StepLogits.continues)
        la.seq_ids, la.lens, la.plan, la.dev, la.tokens, la.logits = list(seq_ids_list), next_lens, nxt, dev, None, opts
        self.prepared = la      # (not to be taken before the host knows the tokens it continues: tokens_known)

    def tokens_known(self, tokens: List[int]):
        """The tokens of the step just run, now on the host: the step prepared behind it (if any) may be taken."""
        if self.prepared is not None:
            self.prepared.tokens = tokens

    def take(self, input_ids_list, seq_ids_list, decoding_seq_lens_list, ignore_kvcache, opts: StepLogits = PLAIN):
        """The prepared step, if this call is it (any other call drops the preparation): the same sequences, every length
        + 1, the tokens just returned, and logits options that continue those of the step it was prepared behind."""
        la, self.prepared = self.prepared, None
        if (la is None or la.tokens is None or ignore_kvcache or not self.lookahead or not self.on
                or len(input_ids_list) != len(la.lens) or list(decoding_seq_lens_list) != la.lens
                or list(seq_ids_list) != la.seq_ids or not opts.continues(la.logits)):
            return None
        for ids, tok in zip(input_ids_list, la.tokens):
            if len(ids) != 1 or ids[0] != tok:
                return None
        return la
