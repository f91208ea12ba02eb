"""Iteration-level FCFS scheduler over the paged KV pool, with swapping and (optionally) piggybacking.

Behaviour follows the reference's swiftllm/server/scheduler.py:33-140: strict arrival order; a prefill
batch is admitted while it fits the sequence/token/block budgets; otherwise every running request
decodes one token; when the pool cannot hold the running set the most recent requests are swapped out,
and swapped requests return (oldest first) before any new prompt is admitted.

Chunked prefill (`EngineConfig.max_prefill_chunk > 0`, an addition): a step carries at most that many prompt tokens, a
longer prompt is fed over several steps while it sits in the running queue (`_get_next_batch_chunked`).

Two deliberate differences:
  * `piggyback=True` lets the running (decoding) requests ride along with an admitted prefill batch in
    ONE forward (prefill sequences first, as LlamaModel.forward requires) — the SARATHI-style batch the
    reference's forward supports but its scheduler never emits ("If you want decoding requests to be
    piggybacked, you can do it here", scheduler.py:93-94);
  * `get_next_batch` returns three lists. The reference returns `reversed(...)` for the swapped-out
    requests — an iterator that is always truthy, so its idle engine never sleeps (engine.py:122).
"""
from collections import deque
from typing import Optional, Deque, List, Tuple

from swiftllm_amd.utils import cdiv
from .prefix_cache import PrefixCache
from .structs import Request


class RequestIdManager:
    """Hands out block-table rows [0, max_id); lowest free id first."""

    def __init__(self, max_id: int):
        self.max_id = max_id
        self._free = list(range(max_id - 1, -1, -1))

    def get_id(self) -> int:
        if not self._free:
            raise RuntimeError("No more available request ids. Please try to increase `max_seqs_in_block_table`")
        return self._free.pop()

    def free_id(self, req_id: int):
        self._free.append(req_id)

    def free_ids(self, req_ids: List[int]):
        self._free.extend(req_ids)

    def num_free(self) -> int:
        return len(self._free)


class _CacheConflict(Exception):
    """Room (blocks, a row) could only be made by evicting an entry a prompt admitted in this step copies from."""


class Scheduler:
    def __init__(self, model_config, engine_config, num_gpu_blocks: int, piggyback: bool = False):
        self.model_config = model_config    # unused, kept for the reference's constructor signature
        self.engine_config = engine_config
        self.num_gpu_blocks = num_gpu_blocks
        self.piggyback = piggyback
        self.waiting_q: Deque[Request] = deque()
        self.running_q: List[Request] = []
        self.swapped_q: Deque[Request] = deque()
        self.request_id_manager = RequestIdManager(engine_config.max_seqs_in_block_table)
        # limits of the data plane the Engine fills in once the model exists (None = unknown, not checked):
        # rows of the rotary table (LlamaModel.forward raises past it) and the vocabulary size
        self.max_seq_len: Optional[int] = None
        self.vocab_size: Optional[int] = getattr(model_config, "vocab_size", None)
        # ... and a callable returning the names of the LoRA adapters loaded right now (None: the data plane serves none)
        self.lora_names = None
        # prefix caching by block copy (EngineConfig.enable_prefix_caching; chunked path only): finished requests' rows kept
        # as cache entries, and the step's work for the engine — rows to free in the data plane (already back in the id
        # manager here) and (donor row, new row, tokens) copies. None / always empty with the option off.
        self.prefix_cache: Optional[PrefixCache] = None
        if getattr(engine_config, "enable_prefix_caching", False):
            self.prefix_cache = PrefixCache(engine_config.block_size, int(engine_config.prefix_cache_max_seqs))
        self.cache_evictions: List[int] = []
        self.cache_copies: List[Tuple[int, int, int]] = []
        self._cache_pinned: set = set()     # rows a copy of this step reads: not evictable in this step
        self._kept_ids: set = set()         # rows of finished requests that became entries (on_batch_finish keeps them)

    # ---- budgets -------------------------------------------------------------------------------------
    def _blocks(self, req: Request, extra_tokens: int = 0) -> int:
        # (kv_reserved_tokens: what a speculative verify step allocated for drafts, accepted or not; 0 with the option off)
        return cdiv(max(req.num_tokens() + extra_tokens, req.kv_reserved_tokens), self.engine_config.block_size)

    def _running_blocks(self) -> int:
        # (once per decode iteration over the whole running set: spelled out, no per-request method calls)
        bs = self.engine_config.block_size
        return sum((max(r.prompt_len + len(r.output_token_ids), r.kv_reserved_tokens) + bs - 1) // bs
                   for r in self.running_q)

    # ---- events --------------------------------------------------------------------------------------
    def why_unservable(self, req: Request) -> Optional[str]:
        """None, or the reason this request could never run to completion under the engine's limits. Such a
        request must not enter the queues: strict FCFS would park everything behind it (a prompt over the token
        budget is never admitted) or it would swap in and out forever (a sequence larger than the pool). The
        reference has no such check and hangs (scheduler.py:60-90)."""
        ecfg = self.engine_config
        if req.prompt_len <= 0:
            return "empty prompt"
        if req.output_len <= 0:
            return "output_len must be positive"
        ids = req.prompt_token_ids
        if self.vocab_size is not None and ids is not None:
            # ids index the embedding table on the device: out-of-range values must never reach a kernel
            if not all(isinstance(t, int) and not isinstance(t, bool) and 0 <= t < self.vocab_size for t in ids):
                return f"prompt_token_ids must be integers in [0, {self.vocab_size})"
        sp = getattr(req, "sampling_params", None)
        if self.vocab_size is not None and sp is not None:
            # ... and so must the ids the logits adjustment indexes a row with, and a stop token nobody can generate
            if any(t >= self.vocab_size for t, _ in (sp.logit_bias or ())):
                return f"logit_bias ids must be in [0, {self.vocab_size})"
            if any(t >= self.vocab_size for t in sp.stop_token_ids):
                return f"stop_token_ids must be in [0, {self.vocab_size})"
        name = getattr(req, "lora", None)
        if name is not None:
            loaded = self.lora_names() if self.lora_names is not None else ()
            if not isinstance(name, str) or name not in loaded:
                return f"LoRA adapter {name!r} is not loaded (loaded: {sorted(loaded)})"
        if self.max_seq_len is not None and req.prompt_len + req.output_len > self.max_seq_len:
            return (f"prompt ({req.prompt_len}) + output_len ({req.output_len}) exceeds the model's "
                    f"{self.max_seq_len} rotary positions")
        if req.prompt_len > ecfg.max_tokens_in_batch and self._chunk_cap() == 0:   # (chunked prefill feeds it in pieces)
            return f"prompt of {req.prompt_len} tokens exceeds max_tokens_in_batch ({ecfg.max_tokens_in_batch})"
        blocks = cdiv(req.prompt_len + req.output_len, ecfg.block_size)
        if blocks > ecfg.max_blocks_per_seq:
            return f"sequence needs {blocks} KV blocks, max_blocks_per_seq is {ecfg.max_blocks_per_seq}"
        if blocks > self.num_gpu_blocks:
            return f"sequence needs {blocks} KV blocks, the pool has {self.num_gpu_blocks}"
        return None

    def on_requests_arrival(self, requests: List[Request]):
        self.waiting_q.extend(requests)

    def get_next_batch(self) -> Tuple[List[Request], List[Request], List[Request]]:
        """(batch to forward, requests to swap in first, requests to swap out first)."""
        ecfg = self.engine_config
        if self._chunk_cap() > 0:
            return self._get_next_batch_chunked()
        if not self.swapped_q:
            admitted = self._admit_prefills()
            if admitted:
                for req in admitted:
                    req.request_id = self.request_id_manager.get_id()
                riders = list(self.running_q) if self.piggyback and self._riders_fit(admitted) else []
                self.running_q.extend(admitted)
                return admitted + riders, [], []

        # decode step for everything running; make room first if the pool is over-committed
        swapped_out: List[Request] = []
        used = self._running_blocks()
        while len(self.running_q) > ecfg.max_batch_size or used > self.num_gpu_blocks:
            victim = self.running_q.pop()           # the most recently admitted request yields
            used -= self._blocks(victim)
            swapped_out.append(victim)
        swapped_in: List[Request] = []
        if swapped_out:
            self.swapped_q.extendleft(swapped_out)  # they keep their place ahead of older swapped ones
        else:
            while self.swapped_q:
                cand = self.swapped_q[0]
                need = self._blocks(cand)
                if len(self.running_q) + 1 > ecfg.max_batch_size or used + need > self.num_gpu_blocks:
                    break
                self.running_q.append(self.swapped_q.popleft())
                used += need
                swapped_in.append(cand)
        return list(self.running_q), swapped_in, swapped_out[::-1]

    # ---- chunked prefill (EngineConfig.max_prefill_chunk > 0) ------------------------------------------------
    def _chunk_cap(self) -> int:
        """Prompt tokens one step may carry in total; 0 = chunking off (a prompt is one forward)."""
        ecfg = self.engine_config
        chunk = int(getattr(ecfg, "max_prefill_chunk", 0) or 0)
        return min(chunk, ecfg.max_tokens_in_batch) if chunk > 0 else 0

    def _get_next_batch_chunked(self) -> Tuple[List[Request], List[Request], List[Request]]:
        """The same policy with a prompt fed in pieces. A request whose prompt is partly resident stays in running_q: it
        holds its block-table row and its blocks (reserved for the WHOLE prompt at admission, as without chunking) and
        counts towards max_batch_size, but it is not a decode rider. Every step: make room / swap in exactly as the
        decode step does; hand the step's prompt-token budget to the partly prefilled requests in arrival order, then —
        only when nobody waits swapped out and budget is left — to new prompts from the head of the queue (strict FCFS:
        a partly fed prompt leaves no budget, so nothing overtakes it); the running decodes ride along when
        piggybacking and their tokens and blocks fit, and decode alone in a step that carries no prompt tokens."""
        ecfg = self.engine_config
        swapped_out: List[Request] = []
        used = self._running_blocks()
        while len(self.running_q) > ecfg.max_batch_size or used > self.num_gpu_blocks:
            victim = self.running_q.pop()           # the most recently admitted request yields, partly prefilled or not
            used -= self._blocks(victim)
            swapped_out.append(victim)
        swapped_in: List[Request] = []
        cache = self.prefix_cache
        if cache is not None:
            # cached blocks are reclaimable: every comparison below is made WITHOUT them, exactly as with the option off,
            # and whatever it grants is made room for by evicting entries (least recently used first)
            self._cache_pinned = set()
            self._cache_make_room(used)
        if swapped_out:
            self.swapped_q.extendleft(swapped_out)
        else:
            while self.swapped_q:
                cand = self.swapped_q[0]
                need = self._blocks(cand)
                if len(self.running_q) + 1 > ecfg.max_batch_size or used + need > self.num_gpu_blocks:
                    break
                self.running_q.append(self.swapped_q.popleft())     # (it continues at its num_prefilled)
                used += need
                swapped_in.append(cand)
                if cache is not None:
                    self._cache_make_room(used)

        budget = self._chunk_cap()
        chunks: List[Request] = []
        for req in self.running_q:
            if req.is_prompt_resident():
                continue
            take = min(budget, req.prompt_len - req.num_prefilled)
            if take <= 0:
                break
            req.prefill_take = take
            chunks.append(req)
            budget -= take
        if not self.swapped_q:
            try:
                chunks += self._admit_waiting(budget, used, cache is not None)
            except _CacheConflict:
                # an entry this step copies from stood in the way of a later admission: the step is redone without hits,
                # every entry evictable — what the scheduler without the cache admits
                chunks += self._admit_waiting(budget, used, False)
        decoders = [r for r in self.running_q if r.is_prompt_resident()]
        if not chunks:
            return decoders, swapped_in, swapped_out[::-1]
        riders: List[Request] = []
        if self.piggyback and decoders:
            # blocks: `used` above already holds every decoder at the length this step leaves it with (num_tokens()
            # counts the token it stores now) and every partly fed prompt whole; a decoder that outgrows the pool while a
            # prompt is being fed makes the NEXT step swap out the most recent request — possibly that prompt, which
            # then continues at its num_prefilled after swap-in
            if sum(r.prefill_take for r in chunks) + len(decoders) <= ecfg.max_tokens_in_batch:
                riders = decoders
        return chunks + riders, swapped_in, swapped_out[::-1]

    # ---- prefix caching (EngineConfig.enable_prefix_caching) ----------------------------------------------------
    @staticmethod
    def cache_eligible(req: Request) -> bool:
        """May hit and donate: no LoRA adapter (K/V depend on it) and no processed logits (the data plane's token history
        starts at a context-0 prefill). Plain sampled requests are eligible: their draws depend on seed and position."""
        sp = getattr(req, "sampling_params", None)
        return getattr(req, "lora", None) is None and (sp is None or not sp.processes_logits)

    def _cache_evict_one(self) -> bool:
        entry = self.prefix_cache.evict_lru(self._cache_pinned)
        if entry is None:
            return False
        self.cache_evictions.append(entry.seq_id)
        self.request_id_manager.free_id(entry.seq_id)
        return True

    def _cache_make_room(self, used: int) -> bool:
        """Evict until the running set's `used` blocks and the cache's fit the pool; False: only pinned entries are left."""
        while used + self.prefix_cache.num_blocks_held > self.num_gpu_blocks:
            if not self._cache_evict_one():
                return False
        return True

    def _admit_waiting(self, budget: int, used: int, allow_hits: bool) -> List[Request]:
        """New prompts from the head of the queue while the step's prompt-token budget, the batch and the pool take them
        (the last part of _get_next_batch_chunked). With the prefix cache on, the comparisons are the same, on the same
        numbers — the cache's blocks are not in `used` — and room is then made for what they granted. A prompt that
        matches an entry (`allow_hits`) starts at num_prefilled = the matched tokens, so the budget counts only what is
        fed; its block need is unchanged (private blocks for its whole length). Raises _CacheConflict — with every
        admission of this call undone — when room could only be made by evicting an entry pinned by a hit of this call."""
        ecfg, cache, ids = self.engine_config, self.prefix_cache, self.request_id_manager
        admitted: List[Request] = []
        copies: List[Tuple[int, int, int]] = []
        while budget > 0 and self.waiting_q:
            cand = self.waiting_q[0]
            need = self._blocks(cand)
            if len(self.running_q) + 1 > ecfg.max_batch_size or used + need > self.num_gpu_blocks:
                break       # strict FCFS: nothing may overtake the head of the queue
            entry, tokens = None, 0
            if cache is not None:
                if allow_hits and self.cache_eligible(cand):
                    entry, tokens = cache.match(cand.prompt_token_ids)
                fresh_pin = entry is not None and entry.seq_id not in self._cache_pinned
                if entry is not None:
                    self._cache_pinned.add(entry.seq_id)
                ok = self._cache_make_room(used + need) and (ids.num_free() > 0 or self._cache_evict_one())
                if not ok and fresh_pin:        # the donor itself stands in the way: no hit, the entry goes
                    self._cache_pinned.discard(entry.seq_id)
                    entry, tokens = None, 0
                    ok = self._cache_make_room(used + need) and (ids.num_free() > 0 or self._cache_evict_one())
                if not ok and len(cache) > 0:
                    for r in reversed(admitted):
                        self.running_q.pop()
                        ids.free_id(r.request_id)
                        r.request_id, r.num_prefilled, r.prefill_take = -1, 0, 0
                        self.waiting_q.appendleft(r)
                    self._cache_pinned = set()
                    raise _CacheConflict()
            self.waiting_q.popleft()
            cand.request_id = ids.get_id()
            if entry is not None:
                cand.num_prefilled = tokens
                copies.append((entry.seq_id, cand.request_id, tokens))
            cand.prefill_take = min(budget, cand.prompt_len - cand.num_prefilled)
            budget -= cand.prefill_take
            used += need
            self.running_q.append(cand)
            admitted.append(cand)
        self.cache_copies.extend(copies)
        return admitted

    def retire(self, req: Request) -> bool:
        """A finished request, before on_batch_finish: True when its block-table row became a cache entry — the caller
        then keeps the row's KV blocks — instead of going back to the id manager. The entry covers prompt + output[:-1]
        (the last token's K/V was never stored), whole blocks only. An entry that had to go to make room for it is left in
        `cache_evictions`."""
        cache = self.prefix_cache
        if cache is None or not self.cache_eligible(req) or req.request_id < 0:
            return False
        tokens = list(req.prompt_token_ids) + list(req.output_token_ids[:-1])
        if len(tokens) < cache.block_size or cache.holds(tokens):
            return False
        self._cache_pinned = set()      # (the step's copies were issued before its forward)
        while len(cache) >= cache.max_entries:
            self._cache_evict_one()
        if not cache.insert(req.request_id, tokens, self._blocks(req)):
            return False
        self._kept_ids.add(req.request_id)
        return True

    def take_cache_work(self) -> Tuple[List[int], List[Tuple[int, int, int]]]:
        """(rows of evicted entries: the data plane frees them — they are back in the id manager already; copies of the
        step as (donor row, new row, tokens)). Both empty with the option off."""
        if not self.cache_evictions and not self.cache_copies:
            return [], []
        work = (self.cache_evictions, self.cache_copies)
        self.cache_evictions, self.cache_copies = [], []
        return work

    def drop_prefix_cache(self) -> List[int]:
        """Forget every entry; returns the rows the data plane must free (evictions not yet taken included). The rows go
        back to the id manager here."""
        if self.prefix_cache is None:
            return []
        ids = self.prefix_cache.clear()
        self.request_id_manager.free_ids(ids)
        self._cache_pinned = set()
        evicted, _ = self.take_cache_work()
        return evicted + ids

    def _admit_prefills(self) -> List[Request]:
        ecfg = self.engine_config
        batch: List[Request] = []
        if not self.waiting_q:
            return batch
        blocks = self._running_blocks()
        tokens = 0
        while self.waiting_q:
            cand = self.waiting_q[0]
            need = self._blocks(cand)
            if (len(self.running_q) + len(batch) + 1 > ecfg.max_batch_size
                    or blocks + need > self.num_gpu_blocks
                    or tokens + cand.prompt_len > ecfg.max_tokens_in_batch):
                break       # strict FCFS: nothing may overtake the head of the queue
            batch.append(self.waiting_q.popleft())
            blocks += need
            tokens += cand.prompt_len
        return batch

    def _riders_fit(self, admitted: List[Request]) -> bool:
        """Decoding requests ride along only if their next token fits the token and block budgets."""
        ecfg = self.engine_config
        tokens = sum(r.prompt_len for r in admitted) + len(self.running_q)
        blocks = sum(self._blocks(r) for r in admitted) + sum(self._blocks(r, 1) for r in self.running_q)
        return tokens <= ecfg.max_tokens_in_batch and blocks <= self.num_gpu_blocks

    def on_batch_finish(self, batch: List[Request]):
        kept = self._kept_ids       # (rows that became prefix-cache entries stay out of the id manager; empty: option off)
        self.request_id_manager.free_ids([r.request_id for r in batch if r.is_finished() and r.request_id not in kept])
        if kept:
            kept.difference_update(r.request_id for r in batch)
        self.running_q = [r for r in self.running_q if not r.is_finished()]

    def has_work(self) -> bool:
        return bool(self.waiting_q or self.running_q or self.swapped_q)
