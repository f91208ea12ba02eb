"""Engine — the control loop around one LlamaModel replica.

Public surface of the reference's swiftllm/server/engine.py:15-180: `initialize()`,
`add_request_and_stream()`, `add_request_and_wait()`, `start_all_event_loops()`.

The reference runs scheduling on the asyncio loop and hands every `forward` to a thread pool
(engine.py:121-176): two thread wake-ups per decode step (the pool worker, then the event loop: ~170 us when
both slept through a 4 ms step) plus the per-request fan-out (one queue put and one consumer wake-up per
request, ~6 us each) between one step's tokens and the next step's launch — 450-650 us per iteration against a
4 ms decode step (`tools/engine_overhead.py`). Here the critical loop lives on ONE dedicated model thread that
never sleeps while there is work: arrivals are drained from a thread-safe inbox, the scheduler picks the batch,
`LlamaModel.forward` runs in place, and the fan-out of step k is posted to the event loop only when step k+1 has
been LAUNCHED (`LlamaModel.after_launch_hook`, called once the kernels are enqueued and before the host blocks on
the tokens) — it runs on the asyncio thread while the GPU works. The asyncio side keeps what belongs there:
tokenization of arrivals, per-request queues and events, the HTTP layer.
"""
import asyncio
import functools
import gc
import queue
import threading
from typing import AsyncGenerator, List, Optional, Tuple

from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.guided import GuideCursor, GuideStoreFull, GuideViolation, guide_key
from swiftllm_amd.model_config import LlamaModelConfig
from swiftllm_amd.utils import GB

from .scheduler import Scheduler
from .speculative import NgramProposer, accept
from .structs import RawRequest, Request, StepOutput
from .tokenization import TokenizationEngine


class Engine:
    def __init__(self, engine_config: EngineConfig, model=None, piggyback: bool = False):
        """`model`: an object with LlamaModel's methods (tests inject a fake); None = build the real one
        in `initialize()`."""
        self.engine_config = engine_config
        self.model = model
        self.model_config = getattr(model, "model_config", None)
        self.piggyback = piggyback
        self.initialized = False
        self.event_loop = None
        self.scheduler: Optional[Scheduler] = None
        self.tokenization_engine = None
        self.untokenized_raw_requests: List[Tuple[Request, RawRequest]] = []
        self.num_forwards = 0
        self.num_swapped_out = self.num_swapped_in = 0     # sequences moved to / from the host swap pool so far
        # prompt-lookup speculative decoding (EngineConfig.speculative_ngram): effective drafts per sequence per step (set by
        # initialize: capped by the model), verify steps run, drafts proposed and drafts accepted so far
        self.speculative_k = 0
        self.num_verify_steps = self.num_draft_tokens = self.num_accepted_tokens = 0
        # prefix caching by block copy (EngineConfig.enable_prefix_caching): prompts that reused a cached prefix, the prompt
        # tokens they did not prefill, and cache entries reclaimed so far
        self.num_prefix_hits = self.num_prefix_hit_tokens = self.num_prefix_evictions = 0
        # asyncio thread -> model thread: lists of servable requests (the scheduler is touched by the model thread only)
        self._inbox: "queue.SimpleQueue[List[Request]]" = queue.SimpleQueue()
        # model thread only: (request, token, finished, its TokenLogprob or None) of the last step, not fanned out yet
        self._undelivered: List[Tuple[Request, int, bool, object]] = []
        self._stop = threading.Event()
        self._model_thread: Optional[threading.Thread] = None
        # event-loop thread only: requests somebody may still be waiting on (woken with `error` set if the model thread dies)
        self._live: set = set()
        self._dead = None               # why the model thread is gone (set by _fail_live): new requests are refused with it

    async def _run_on_model_async(self, func, *args, **kwargs):
        return await self.event_loop.run_in_executor(None, functools.partial(func, *args, **kwargs))

    async def initialize(self, num_gpu_blocks: Optional[int] = None):
        self.event_loop = asyncio.get_running_loop()
        if self.model is None:
            from swiftllm_amd.worker.model import LlamaModel
            print("[Engine] Initializing model...")
            self.model = LlamaModel(self.engine_config)
            self.model_config = self.model.model_config
            print("[Engine] Loading weights...")
            self.model.load_weights()
            print("[Engine] Profiling kv blocks...")
            num_gpu_blocks = self.model.profile_num_blocks()
            block_bytes = self.engine_config.block_size * self.model_config.get_kvslot_size(self.model.dtype)
            print(f"[Engine] Number of GPU blocks: {num_gpu_blocks} ({num_gpu_blocks * block_bytes / GB:.2f} GB)")
            print(f"[Engine] Number of CPU blocks: {self.engine_config.num_cpu_blocks} "
                  f"({self.engine_config.num_cpu_blocks * block_bytes / GB:.2f} GB)")
            print("[Engine] Allocating kv cache and swap...")
            self.model.init_kvcache_and_swap(num_gpu_blocks)
        elif num_gpu_blocks is None:
            num_gpu_blocks = self.model.num_blocks
        self.scheduler = Scheduler(self.model_config, self.engine_config, num_gpu_blocks, self.piggyback)
        rope = getattr(self.model, "_cos_cached", None)
        if rope is not None:     # a request that would outgrow the rotary table is refused up front (HTTP 400),
            self.scheduler.max_seq_len = int(rope.shape[0])     # not left to raise inside forward mid-flight
        if hasattr(self.model, "loras"):     # a request may only name an adapter that is loaded when it arrives
            self.scheduler.lora_names = lambda: self.model.loras().keys()
        self.tokenization_engine = TokenizationEngine(self.engine_config)
        want_k = int(getattr(self.engine_config, "speculative_ngram", 0) or 0)
        if want_k > 0:
            self.speculative_k = max(0, min(want_k, int(getattr(self.model, "max_draft_tokens", 0) or 0)))
            print(f"[Engine] Prompt-lookup speculative decoding: {self.speculative_k} drafts per sequence per step "
                  f"(asked for {want_k}), decode batches of <= {self.engine_config.speculative_max_batch} greedy requests")
        if self.scheduler.prefix_cache is not None:
            if not hasattr(self.model, "copy_kv_prefix"):
                raise RuntimeError("enable_prefix_caching needs a data plane with copy_kv_prefix")
            print(f"[Engine] Prefix caching by KV block copy: up to {self.engine_config.prefix_cache_max_seqs} cached "
                  f"sequences, reclaimed least recently used first")
        if hasattr(self.model, "after_launch_hook"):
            self.model.after_launch_hook = self._post_undelivered
        self.initialized = True
        print("[Engine] Model initialized")

    # ---- request entry points -----------------------------------------------------------------------------
    def _enqueue(self, raw_request: RawRequest) -> Request:
        request = Request(raw_request)
        if self._dead is not None:      # the model thread is gone: answer at once, nobody will ever serve this
            request.error = self._dead
            request.finished_event.set()
            request.output_q.put_nowait(None)
            return request
        self._live.add(request)         # (event-loop thread; leaves in _deliver / on rejection / in _fail_live)
        self.untokenized_raw_requests.append((request, raw_request))
        return request

    async def add_request_and_stream(self, raw_request: RawRequest) -> AsyncGenerator[StepOutput, None]:
        """Yield a StepOutput per generated token. (Ends after `output_len` deliveries, or at the None that follows the
        last token of a request a stop token ended early — not on `request.is_finished()`: the request's own token list
        runs one step ahead of what has been fanned out.)"""
        request = self._enqueue(raw_request)
        delivered = 0
        while True:
            step_output = await request.output_q.get()
            if step_output is None:     # rejected (request.error says why), or ended early by a stop token
                break
            yield step_output
            request.output_q.task_done()
            delivered += 1
            if delivered >= request.output_len:
                break

    async def add_request_and_wait(self, raw_request: RawRequest) -> Tuple[Request, List[int]]:
        """Wait for the whole generation; returns (request, output token ids)."""
        request = self._enqueue(raw_request)
        await request.finished_event.wait()
        return request, request.output_token_ids

    # ---- LoRA adapters, while serving ---------------------------------------------------------------------------------
    def _on_model_thread(self, func):
        """Run `func` where the model runs: on the model thread between two iterations while the serving loop is alive
        (a callable posted through the inbox), in place otherwise. Blocks the caller until it ran; re-raises what it raised."""
        thread = self._model_thread
        if thread is None or not thread.is_alive() or threading.current_thread() is thread:
            return func()
        done, box = threading.Event(), {}

        def job():
            try:
                box["value"] = func()
            except BaseException as exc:     # noqa: BLE001 — handed to the caller
                box["error"] = exc
            finally:
                done.set()
        self._inbox.put(job)
        while not done.wait(0.05):
            if not thread.is_alive():
                raise RuntimeError("the model thread stopped before the LoRA command ran")
        if "error" in box:
            raise box["error"]
        return box.get("value")

    def _lora_in_use(self, name: str) -> bool:
        sch = self.scheduler
        return any(r.lora == name for q in (sch.waiting_q, sch.running_q, sch.swapped_q) for r in q)

    def load_lora(self, name: str, path: Optional[str] = None, **kwargs) -> int:
        """Load an adapter while serving (LlamaModel.load_lora, on the model thread); returns its slot. Call it from any
        thread but the event loop's (an HTTP handler: `await loop.run_in_executor(None, engine.load_lora, ...)`)."""
        return self._on_model_thread(lambda: self.model.load_lora(name, path, **kwargs))

    def unload_lora(self, name: str) -> int:
        """Unload an adapter (on the model thread). Refused with ValueError while a waiting, running or swapped request
        names it; requests that arrive afterwards are refused by the scheduler (the adapter is not loaded)."""
        def unload():
            self._drain_inbox()     # (arrivals already accepted against the loaded set count as waiting)
            if self._lora_in_use(name):
                raise ValueError(f"LoRA adapter {name!r} is in use by a request that is waiting, running or swapped out")
            return self.model.unload_lora(name)
        return self._on_model_thread(unload)

    # ---- prefix caching ------------------------------------------------------------------------------------------------
    def drop_prefix_cache(self) -> int:
        """Free every cached sequence (on the model thread): its KV blocks go back to the pool, its block-table row to the
        id manager. Returns how many rows were freed. Needed before LlamaModel.set_kv_scales, which refuses while
        sequences hold blocks; harmless with the option off."""
        def drop():
            ids = self.scheduler.drop_prefix_cache()
            if ids:
                self.model.free_seqs_resources(ids)
            return len(ids)
        return self._on_model_thread(drop)

    def _retire(self, finished: List[Request]):
        """Requests that finished in this step, before anyone is told: an eligible one's row becomes a prefix-cache entry
        (it keeps its KV blocks), the others — and the entries that made room — are released as always."""
        for r in finished:
            self._release_guide(r)
        free = [r.request_id for r in finished if not self.scheduler.retire(r)]
        evicted, _ = self.scheduler.take_cache_work()
        self.num_prefix_evictions += len(evicted)
        if free or evicted:
            # release KV blocks before anyone is told: a caller that sees "finished" may tear us down
            self.model.free_seqs_resources(free + evicted)

    # ---- guided decoding ------------------------------------------------------------------------------------------------
    def _acquire_guide(self, req: Request):
        """Compile (cached) and make resident the guide of a guided request, and give the request its cursor. Runs in an
        executor of the event loop, like tokenisation, never on the model thread; whatever is wrong with the guide is the
        request's `error` (a full store: a retryable one), never an exception."""
        sp = req.sampling_params
        store = getattr(self.model, "guide_store", None)
        if store is None:
            req.error = "guided decoding is off: the engine was started with guided_max_states = 0"
            return
        try:
            kind, spec = sp.guide_spec()
            req.guide_cursor = GuideCursor(store.acquire(guide_key(kind, spec, sp.stop_token_ids)))
        except GuideStoreFull as exc:
            req.error, req.error_retryable = f"guided decoding: {exc}", True
        except Exception as exc:     # noqa: BLE001 — GuideSyntaxError, an oversized NFA / DFA, ids outside the vocabulary,
            # a pattern nested too deeply to parse ... whatever it is, it is this request's answer: the submission loop
            # serves every other request and must survive it
            what = str(exc) if isinstance(exc, ValueError) else f"{type(exc).__name__}: {exc}"
            req.error = f"guided decoding: {what}"

    def _acquire_guides(self, requests: List[Request]):
        """One executor job for the guided requests of one batch of arrivals, in arrival order."""
        for req in requests:
            self._acquire_guide(req)

    def _release_guide(self, req: Request):
        """Drop the request's reference on its guide (finished, failed or refused after it was acquired); once only."""
        cur = req.guide_cursor
        if cur is not None and not cur.released:
            cur.released = True
            self.model.guide_store.release(cur.guide)

    # ---- asyncio side -------------------------------------------------------------------------------------------
    async def _tokenize_raw_request_event_loop(self):
        while True:
            if not self.untokenized_raw_requests:
                await asyncio.sleep(0.002)
                continue
            pending, self.untokenized_raw_requests = self.untokenized_raw_requests, []
            texts = [(req, raw.prompt) for req, raw in pending if not req.prompt_token_ids]
            if texts:
                ids = await self.tokenization_engine.batched_tokenize([p for _, p in texts])
                for (req, _), token_ids in zip(texts, ids):
                    req.prompt_token_ids = list(token_ids)
                    req.prompt_len = len(token_ids)
            servable, guided = [], []
            for req, _ in pending:
                req.error = self._dead or self.scheduler.why_unservable(req)      # (reads the engine's limits only)
                if req.error is None and req.sampling_params is not None and req.sampling_params.guided:
                    guided.append(req)      # (its guide is compiled and acquired below, off the event loop)
                elif req.error is None:
                    servable.append(req)
                else:           # answer at once: waiters wake up with no tokens, streams end
                    self._reject([req])
            if servable:        # the requests without a guide do not wait for anybody's compile
                self._inbox.put(servable)
            if guided:
                await self.event_loop.run_in_executor(None, self._acquire_guides, guided)
                self._reject([r for r in guided if r.error is not None])
                servable = [r for r in guided if r.error is None]
                if servable:
                    self._inbox.put(servable)
            await asyncio.sleep(0.001)

    def _deliver(self, outputs: List[Tuple[Request, int, bool, object]]):
        """Fan one step's tokens out to the per-request queues and events (event-loop thread)."""
        for req, tok, finished, lp in outputs:
            if tok is not None:         # (None: a request the engine ended with an error — no token, only the end)
                req.output_q.put_nowait(StepOutput(tok, req, lp))
            if finished:
                self._live.discard(req)
                req.finished_event.set()
                if len(req.output_token_ids) < req.output_len:      # a stop token ended it: streams do not wait for more
                    req.output_q.put_nowait(None)

    def _fail_live(self, why: str):
        """The model thread is gone: wake every caller still waiting (event-loop thread). `add_request_and_wait` returns
        with what was generated so far and `request.error` set; streams end."""
        self._dead = why                # from now on _enqueue and the tokenize loop refuse instead of queueing
        live, self._live = list(self._live), set()
        pending, self.untokenized_raw_requests = self.untokenized_raw_requests, []
        for req in live + [r for r, _ in pending]:
            self._release_guide(req)
            req.error = req.error or why
            req.finished_event.set()
            req.output_q.put_nowait(None)

    # ---- model thread ---------------------------------------------------------------------------------------------
    def _post_undelivered(self):
        """Hand the held-back tokens to the event loop. Called on the model thread: by LlamaModel.forward right after
        a step's kernels were enqueued (`after_launch_hook`), and by `_iterate` when nothing will be launched."""
        if not self._undelivered:
            return
        outputs, self._undelivered = self._undelivered, []
        try:
            self.event_loop.call_soon_threadsafe(self._deliver, outputs)
        except RuntimeError:        # the event loop is gone (shutdown): nobody is listening any more
            pass

    def _drain_inbox(self, wait_s: float = 0.0):
        """Arrivals go to the scheduler; a callable (a LoRA load / unload posted by _on_model_thread) is held back and run
        once the inbox is empty, so that it sees every arrival that was accepted before it."""
        jobs = []
        try:
            if wait_s > 0.0:
                self._take_inbox_item(self._inbox.get(timeout=wait_s), jobs)
            while True:
                self._take_inbox_item(self._inbox.get_nowait(), jobs)
        except queue.Empty:
            pass
        for job in jobs:
            job()

    def _take_inbox_item(self, item, jobs: list):
        if callable(item):
            jobs.append(item)
            return
        # An adapter may have been unloaded between the check on the event loop (why_unservable) and this moment: the
        # name is checked again here, on the thread that loads and unloads, and such a request is answered with an error
        # instead of reaching forward() with an unknown name.
        names = self.scheduler.lora_names
        gone = [r for r in item if r.lora is not None and (names is None or r.lora not in names())]
        if gone:
            item = [r for r in item if r not in gone]
            for r in gone:
                r.error = f"LoRA adapter {r.lora!r} is not loaded"
                self._release_guide(r)
            try:
                self.event_loop.call_soon_threadsafe(self._reject, gone)
            except RuntimeError:        # the event loop is gone (shutdown)
                pass
        self.scheduler.on_requests_arrival(item)

    def _reject(self, requests: List[Request]):
        """Answer requests that will never run (event-loop thread): waiters wake up with `error` set, streams end."""
        for req in requests:
            self._live.discard(req)
            req.finished_event.set()
            req.output_q.put_nowait(None)

    def _iterate(self) -> bool:
        """One scheduling iteration, start to finish, on the calling (model) thread; False when there was nothing
        to do. Reference: engine.py:121-176."""
        self._drain_inbox()
        batch, swap_in, swap_out = self.scheduler.get_next_batch()
        evicted, copies = self.scheduler.take_cache_work()      # (prefix caching; both empty with the option off)
        if not batch:
            self._post_undelivered()        # no launch to hide the fan-out behind
            if not swap_in and not swap_out and not evicted:
                return False
        if swap_out:
            self.model.swap_out_seqs([r.request_id for r in swap_out])
            self.num_swapped_out += len(swap_out)
        if evicted:     # reclaimed cache entries: their blocks are what the swap-in, the copies and the forward were granted
            self.model.free_seqs_resources(evicted)
            self.num_prefix_evictions += len(evicted)
        if swap_in:
            self.model.swap_in_seqs([r.request_id for r in swap_in])
            self.num_swapped_in += len(swap_in)
        if copies:      # the step's hits: private copies of the donors' blocks, one launch, before the forward that attends them
            self.model.copy_kv_prefix([c[0] for c in copies], [c[1] for c in copies], [c[2] for c in copies])
            self.num_prefix_hits += len(copies)
            self.num_prefix_hit_tokens += sum(c[2] for c in copies)
        drafts = self._propose_drafts(batch) if batch and self.speculative_k > 0 else None
        if drafts is not None:
            self._verify_step(batch, drafts)
        elif batch:
            # prefill sequences first (the scheduler orders them so), their whole prompt; decoding ones
            # bring their last token and their length INCLUDING it
            # (chunked prefill: a prefill sequence brings the next `prefill_take` tokens of its prompt and the number of
            # tokens already resident; without chunking that is the whole prompt behind a context of 0)
            prefills = [r for r in batch if not r.is_prompt_resident()]
            takes = {id(r): (r.prefill_take or r.prompt_len - r.num_prefilled) for r in prefills}
            input_ids = [[r.output_token_ids[-1]] if r.is_prompt_resident() else
                         r.prompt_token_ids if r.num_prefilled == 0 and takes[id(r)] == r.prompt_len else
                         r.prompt_token_ids[r.num_prefilled:r.num_prefilled + takes[id(r)]] for r in batch]
            seq_ids = [r.request_id for r in batch]
            decoding_lens = [r.num_tokens() for r in batch if r.is_prompt_resident()]
            sampling = [r.sampling_params for r in batch]
            kwargs = {}
            if any(sp is not None for sp in sampling):     # (all-greedy: the reference's three-argument call)
                kwargs["sampling_params"] = sampling
            if any(r.num_prefilled for r in prefills):      # (no resident context: the call of always)
                kwargs["prefill_ctx_lens"] = [r.num_prefilled for r in prefills]
            if any(r.lora is not None for r in batch):      # (no adapter in the batch: the call of always)
                kwargs["lora"] = [r.lora for r in batch]
            if any(r.guide_cursor is not None for r in batch):      # (no guided request in the batch: the call of always)
                kwargs["guides"] = [r.guide_cursor for r in batch]
            try:
                tokens = self.model.forward(input_ids, seq_ids, decoding_lens, **kwargs)
            finally:
                self._post_undelivered()    # (a data plane without the hook, or a forward that raised before launching)
            self.num_forwards += 1
            # (a step in which some request asks for logprobs: what the data plane learnt about its tokens, aligned with
            # the batch; a data plane that never scores is not asked)
            scores = None
            if any(sp is not None and sp.logprobs is not None for sp in sampling):
                scores = getattr(self.model, "last_logprobs", None)
            outputs, finished = [], []
            for i, (req, tok) in enumerate(zip(batch, tokens)):
                if id(req) in takes:
                    req.num_prefilled += takes[id(req)]
                    req.prefill_take = 0
                    if req.num_prefilled < req.prompt_len:
                        continue        # not the last chunk: its token (and its logprobs) discarded — nothing appended, nothing delivered
                                        # (and a guided request's cursor stays where it is)
                if req.guide_cursor is not None:
                    try:
                        req.guide_cursor.advance(tok)       # (is_finished below reads the state the token led to)
                    except GuideViolation as exc:
                        # the state allows no token at all (the picker's answer to an all -inf row is not allowed either):
                        # the vocabulary cannot spell what the guide needs here. This request ends with an error; the
                        # others of the batch go on. Its token is not delivered.
                        req.error = f"guided decoding: no token is allowed after {bytes(req.guide_cursor.text)!r}: {exc}"
                        req.aborted = True
                        outputs.append((req, None, True, None))
                        finished.append(req)
                        continue
                req.output_token_ids.append(tok)
                lp = None
                if scores is not None and sampling[i] is not None and sampling[i].logprobs is not None:
                    lp = scores[i]
                    req.output_logprobs.append(lp)
                done = req.is_finished()
                outputs.append((req, tok, done, lp))
                if done:
                    finished.append(req)
            if finished:
                self._retire(finished)
            self._undelivered = outputs
            self.scheduler.on_batch_finish(batch)
        return True

    # ---- prompt-lookup speculative decoding ------------------------------------------------------------------------
    def _propose_drafts(self, batch: List[Request]) -> Optional[List[List[int]]]:
        """Drafts for every request of the batch (aligned with it), or None when this step is a plain forward: a prompt
        (chunk) in the batch, more than speculative_max_batch requests, a request with sampling params (sampled, or greedy
        with processed logits or stop tokens: a verify step picks the argmax of the raw logits), a request with a LoRA
        adapter (forward_verify takes none), or no draft at all. Drafts are
        clipped so that the accepted tokens never pass output_len, positions never pass the rotary table or the block
        table row, the step's rows never pass max_tokens_in_batch, and the blocks the drafts need beyond the plain step's
        are free in the allocator right now — drafts are dropped, never swapped for."""
        ecfg = self.engine_config
        if (len(batch) > int(getattr(ecfg, "speculative_max_batch", 0)) or not hasattr(self.model, "forward_verify")
                or any(not r.is_prompt_resident() or r.sampling_params is not None or r.lora is not None for r in batch)):
            return None
        bs = ecfg.block_size
        limit = self.scheduler.max_seq_len
        rows_left = ecfg.max_tokens_in_batch - len(batch)
        mgr = getattr(self.model, "gpu_block_manager", None)
        held = {}
        for r in batch:
            if mgr is not None:
                held[id(r)] = mgr.host.num_allocated(r.request_id)
            else:
                held[id(r)] = -(-max(r.num_tokens() - 1, r.kv_reserved_tokens) // bs)
        if mgr is not None:
            free = mgr.num_free_blocks
        else:
            free = self.scheduler.num_gpu_blocks - sum(held.values())
        # what the plain step takes: every request stores one token
        spare = free - sum(max(0, -(-r.num_tokens() // bs) - held[id(r)]) for r in batch)
        out, any_draft = [], False
        for r in batch:
            n = r.num_tokens()
            k = min(self.speculative_k, r.output_len - len(r.output_token_ids) - 1, rows_left,
                    ecfg.max_blocks_per_seq * bs - n)
            if limit is not None:
                k = min(k, limit - n)
            d: List[int] = []
            if k > 0:
                prop = r.ngram_proposer
                if prop is None:
                    prop = r.ngram_proposer = NgramProposer()
                prop.sync(r.prompt_token_ids, r.output_token_ids)
                d = prop.propose(k)
            if d:
                base = max(held[id(r)], -(-n // bs))
                extra = -(-(n + len(d)) // bs) - base
                if extra > max(spare, 0):       # keep the drafts that fit the blocks the request has (or will take anyway)
                    d = d[:max(0, (base + max(spare, 0)) * bs - n)]
                    extra = max(0, -(-(n + len(d)) // bs) - base)
                spare -= max(extra, 0)
                rows_left -= len(d)
                any_draft = any_draft or bool(d)
            out.append(d)
        return out if any_draft else None

    def _verify_step(self, batch: List[Request], drafts: List[List[int]]):
        """One verify forward for a pure-decode batch: every request brings its last token and its drafts (requests
        without a draft ride with one row), keeps the accepted prefix plus the token after it, and every token is
        delivered in order as its own StepOutput."""
        input_ids = [[r.output_token_ids[-1]] + d for r, d in zip(batch, drafts)]
        seq_ids = [r.request_id for r in batch]
        ctx_lens = [r.num_tokens() - 1 for r in batch]
        try:
            targets = self.model.forward_verify(input_ids, seq_ids, ctx_lens)
        finally:
            self._post_undelivered()
        self.num_forwards += 1
        self.num_verify_steps += 1
        outputs, finished = [], []
        for req, d, tgt, ctx in zip(batch, drafts, targets, ctx_lens):
            a = accept(d, tgt)
            self.num_draft_tokens += len(d)
            self.num_accepted_tokens += a
            req.kv_reserved_tokens = max(req.kv_reserved_tokens, ctx + 1 + len(d))
            for tok in tgt[:a + 1]:
                if req.is_finished():
                    break
                req.output_token_ids.append(tok)
                outputs.append((req, tok, req.is_finished(), None))
            if req.is_finished():
                finished.append(req)
        if finished:
            self._retire(finished)
        self._undelivered = outputs
        self.scheduler.on_batch_finish(batch)

    def _model_loop(self, failed: "asyncio.Future"):
        # Garbage collection around the latency-critical section (EngineConfig tuning `pause_gc_while_serving`): a
        # generation-2 pass over a process that holds an 8 G-parameter model's tensor objects and thousands of request
        # records takes tens of ms — several decode steps. The long-lived heap is frozen out of the collector's working
        # set once, automatic collection is off while the loop runs, and the loop collects where no request waits for it:
        # the young generations whenever it goes idle after work (or every 256 busy iterations), everything every 4096.
        pause_gc = bool(getattr(self.engine_config, "pause_gc_while_serving", False))
        gc_was_enabled = gc.isenabled()
        if pause_gc:
            gc.collect()
            gc.freeze()
            gc.disable()
        busy = total = 0
        try:
            while not self._stop.is_set():
                if self._iterate():
                    busy += 1
                    total += 1
                    if pause_gc and busy >= 256:
                        gc.collect(2 if total >= 4096 else 1)
                        busy, total = 0, (0 if total >= 4096 else total)
                else:
                    if pause_gc and busy:
                        gc.collect(2 if total >= 4096 else 1)
                        busy, total = 0, (0 if total >= 4096 else total)
                    self._drain_inbox(wait_s=0.005)     # idle: block on the inbox (wakes at once on an arrival)
            self._post_undelivered()
        except BaseException as exc:     # noqa: BLE001 — surfaces in start_all_event_loops(), as in the reference
            def report(exc=exc):
                if not failed.done():
                    failed.set_exception(exc)
            try:
                self.event_loop.call_soon_threadsafe(report)
            except RuntimeError:
                pass
        finally:
            if pause_gc:
                gc.unfreeze()
                if gc_was_enabled:
                    gc.enable()

    async def step(self) -> bool:
        """One scheduling iteration (single-stepping for tests and tools; the serving loop is `_model_loop`). Its
        tokens are fanned out before it returns. False when there was nothing to do."""
        if self._model_thread is not None and self._model_thread.is_alive():
            raise RuntimeError("Engine.step() while the serving loop runs: the scheduler belongs to the model thread")

        def one():
            did = self._iterate()
            self._post_undelivered()
            return did
        did = await self._run_on_model_async(one)
        await asyncio.sleep(0)      # the posted fan-out runs before the caller continues
        return did

    async def _main_event_loop(self):
        """Owns the model thread: starts it, re-raises what it dies of, stops it when cancelled."""
        self._stop.clear()
        failed = self.event_loop.create_future()
        thread = threading.Thread(target=self._model_loop, args=(failed,), name="swiftllm-model", daemon=True)
        self._model_thread = thread
        thread.start()
        try:
            await failed
        except BaseException as exc:        # the model thread died (or we are being cancelled): nobody may wait for ever
            self._fail_live(f"engine stopped: {type(exc).__name__}: {exc}")
            raise
        finally:
            self._stop.set()
            self._inbox.put([])     # wake it if it is waiting for arrivals
            # (at most the step in flight) — joined off the event loop: HTTP and the other coroutines keep running
            try:
                await asyncio.shield(self.event_loop.run_in_executor(None, thread.join, 10.0))
            except asyncio.CancelledError:
                pass

    async def start_all_event_loops(self):
        assert self.initialized, "Engine not initialized. Please call `initialize()` before starting the event loop."
        await asyncio.gather(self._tokenize_raw_request_event_loop(), self._main_event_loop())
