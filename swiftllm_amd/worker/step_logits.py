"""A step's logits options — seeded sampling, logits processing, per-token logprobs, guided decoding — between the call
and the post layer: what one call asked for (StepLogits, host only), the persistent buffers the options' kernels read
(one StagedInts each, owned by the model's LogitsStage) and the views a step hands to the post layer (LogitsArgs)."""
import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

from .kernels import guided as guide_kernels
from .kernels import logits_process
from .kernels import logprobs as token_scores
from .kernels import sampling as sampler


def _hip_ints(words: int, pinned: bool) -> torch.Tensor:
    return torch.empty(words, dtype=torch.int32, **(dict(pin_memory=True) if pinned else dict(device="cuda")))


class StagedInts:
    """Pinned int32 staging, its numpy view, the device twin at a FIXED address (captured hipGraphs read it) and the event
    of the last copy between them. Growing moves the twin: `on_move` is told (the model drops its graphs). `idle`: what the
    twin holds where nothing was shipped yet. `tail`: words per staged word that the twin keeps behind the staged part,
    zeroed, for a kernel to write; `fetch` brings them back through a pinned buffer of their own. `alloc(words, pinned)`
    makes the tensors (tests: ordinary CPU tensors)."""

    def __init__(self, on_move, idle: int = 0, tail: int = 0, alloc=_hip_ints):
        self.on_move, self.idle, self.tail, self.alloc, self.words = on_move, idle, tail, alloc, 0   # (words: staged ones)
        self.host = self.host_np = self.dev = self.staged = self.back = self.back_np = self._done = None

    def resize(self, words: int):
        self.host, self.dev = self.alloc(words, True), self.alloc(words * (1 + self.tail), False)
        self.host_np, self.staged = self.host.numpy(), self.dev[:words]
        self.staged.fill_(self.idle)
        self.dev[words:].zero_()
        self.back = self.alloc(words * self.tail, True)     # (no tail: both are empty)
        self.words, self.back_np, self._done = words, self.back.numpy(), None
        self.on_move()

    def ensure(self, words: int) -> bool:
        """Hold at least `words` staged words: what is asked, or twice what there was. True when the buffer moved."""
        if self.words >= words:
            return False
        self.resize(max(words, 2 * self.words))
        return True

    def begin(self) -> np.ndarray:
        """The view to pack into, once the previous step's copy out of the pinned buffer is done (long since)."""
        if self._done is not None:
            self._done.synchronize()
        return self.host_np

    def ship(self, slices=None):
        """One async H2D copy of the staged part, or one per (lo, hi) of `slices`."""
        if slices is None:
            self.staged.copy_(self.host, non_blocking=True)
        for lo, hi in slices or ():
            self.staged[lo:hi].copy_(self.host[lo:hi], non_blocking=True)
        if self._done is None:
            self._done = torch.cuda.Event()
        self._done.record()

    def send(self, words: int, pack, values):
        self.ensure(words)
        pack(values, self.begin())
        self.ship()

    def fetch(self) -> np.ndarray:
        """One async D2H copy of the tail; the returned view holds it once the stream has been synchronised."""
        self.back.copy_(self.dev[self.words:], non_blocking=True)
        return self.back_np


class StepLogits:
    """What one forward call asked of its logits: per option a list aligned with the batch, or None when no row asks —
    `sampling`: SamplingParams with their seeds resolved (None: a greedy row); `edits`: kernels/logits_process.RowEdits;
    `scoring`: the N of top-N logprobs; `guides`: GuideCursors. Never changed once built."""
    __slots__ = ("sampling", "edits", "scoring", "guides", "flags", "plain")

    def __init__(self, sampling=None, edits=None, scoring=None, guides=None):
        self.sampling, self.edits, self.scoring, self.guides = sampling, edits, scoring, guides
        # (sampled, processed, scored, guided): which kernels the post layer launches, each on a persistent buffer — so
        # each combination is a captured graph of its own and the flags are part of the replay key; the lists are not
        self.flags = (sampling is not None, edits is not None, scoring is not None, guides is not None)
        self.plain = not any(self.flags)

    @classmethod
    def of(cls, sampling=None, edits=None, scoring=None, guides=None) -> "StepLogits":
        """The bundle of these four; the shared PLAIN when none is set (a plain step constructs nothing)."""
        plain = sampling is None and edits is None and scoring is None and guides is None
        return PLAIN if plain else cls(sampling, edits, scoring, guides)

    def continues(self, prev: "StepLogits") -> bool:
        """May this step take the decode step prepared behind `prev`'s? The device still holds the sampling rows (seeds
        resolved) and the rows' N that `prev` shipped, and a hit ships neither: both must be equal, list for list. Entries
        and mask rows go up again on a hit (resend_on_hit): only processed-ness and guided-ness must agree (the graph)."""
        return self is prev or (self.sampling == prev.sampling and self.scoring == prev.scoring
                                and self.flags[1] == prev.flags[1] and self.flags[3] == prev.flags[3])

    @property
    def resend_on_hit(self) -> "StepLogits":
        """The part of this step that a look-ahead hit uploads again before the replay."""
        return StepLogits.of(edits=self.edits, guides=self.guides)


PLAIN = StepLogits()    # a step that asks nothing: argmax of the raw logits, the launches of always


class LogitsArgs(NamedTuple):
    """A step's device views, in the order the post layer uses them; None: that kernel is not launched."""
    guide: Optional[guide_kernels.GuideArgs]
    adjust: Optional[logits_process.AdjustArgs]
    sampling: Optional[sampler.SampleArgs]
    logprobs: Optional[token_scores.LogprobArgs]


class LogitsStage:
    """The device side of the four options, per model; sized for the largest replay bucket at load, grown on demand:
      sampling    5 words per row (kernels/sampling.pack_params); shipped by a sampled step that is not a look-ahead hit
      edits       kernels/logits_process.buffer_len(edit_rows, entries): the row header, then three arrays of a power-of-two
                  entry capacity (a penalised sequence adds at most one entry per step); shipped by every processed step
      scores      a row's N (-1: it does not ask), shipped by a scored step that is not a hit; behind them what
                  kernels/logprobs writes (rank, logprobs, ids), fetched by every scored step
      guide_rows  a row's mask row in the pool (-1: not guided); shipped by every guided step"""
    min_edit_cap = 1024      # entries the edit buffer starts with
    one_copy_words = 16384   # up to this many int32 words the whole edit buffer goes up in one H2D copy

    def __init__(self, on_move):
        self.sampling, self.edits, self.edit_rows = StagedInts(on_move), StagedInts(on_move), 0    # (rows of the edits' header)
        self.scores = StagedInts(on_move, idle=-1, tail=token_scores.buffer_len(1) - 1)
        self.guide_rows = StagedInts(on_move, idle=-1)
        self.guide_masks = self.vocab_dev = None    # guided decoding on: the pool [mask rows, ceil(vocab / 32)], the vocabulary

    def set_vocab(self, vocab, vocab_size: int, device, mask_shape=None):
        self.vocab_dev = guide_kernels.upload_vocab(vocab, vocab_size, device)
        if mask_shape is not None:
            self.guide_masks = torch.zeros(mask_shape, dtype=torch.int32, device=device)

    def reserve(self, rows: int):
        self.sampling.ensure(5 * rows)
        self._ensure_edits(rows, 0)
        self.scores.ensure(rows)
        if self.guide_masks is not None:
            self.guide_rows.ensure(rows)

    def _ensure_edits(self, rows: int, entries: int):
        buf = self.edits
        cap = logits_process.edit_capacity(buf.words, self.edit_rows) if buf.words else 0
        if buf.words and self.edit_rows >= rows and cap >= entries:
            return
        cap = max(cap, self.min_edit_cap)
        while cap < entries:
            cap *= 2
        self.edit_rows = max(rows, self.edit_rows)
        buf.resize(logits_process.buffer_len(self.edit_rows, cap))

    def _ship_edits(self, edits, rows: int):
        self._ensure_edits(rows, sum(len(r.ids) for r in edits if r is not None))
        buf, base = self.edits, 5 * self.edit_rows + 1
        used = logits_process.pack_edits(edits, buf.begin(), self.edit_rows)
        if buf.words <= self.one_copy_words:
            buf.ship()
        else:       # the row header and the used part of each of the three arrays
            cap = logits_process.edit_capacity(buf.words, self.edit_rows)
            buf.ship([(0, base)] + [(base + a * cap, base + a * cap + used) for a in range(3) if used])

    def _build_guide(self, guide):
        """Fill the guide's rows of the pool, on the current stream: behind every earlier step that may still read the rows
        of a guide evicted for it. A DFA guide: one launch of the build kernel; an allowed-token guide: one row, host-made."""
        masks, dev = self.guide_masks, self.guide_masks.device
        if guide.dfa is None:
            masks[guide.base].copy_(torch.from_numpy(guide.host_mask_row(masks.shape[1])))
        else:
            ends = [t for t in guide.end_ids if t < self.vocab_dev.vocab]
            guide_kernels.build_guide_masks(
                masks, guide.base, torch.from_numpy(guide.dfa.trans).to(dev),
                torch.from_numpy(guide.dfa.accepting.view(np.uint8)).to(dev), self.vocab_dev,
                torch.tensor(ends, dtype=torch.int32, device=dev) if ends else None)
        guide.built = True

    def upload(self, opts: StepLogits, rows: int, hit: bool = False):
        """Ship what the kernels of a step of `rows` rows read (rows past the caller's batch: inert) — on a look-ahead hit
        only what `resend_on_hit` names. Guides that are not built yet are built first."""
        if opts.plain:
            return
        if hit:
            opts = opts.resend_on_hit
        if opts.sampling is not None:
            self.sampling.send(5 * rows, sampler.pack_params, opts.sampling)
        if opts.edits is not None:
            self._ship_edits(opts.edits, rows)
        if opts.scoring is not None:
            self.scores.send(rows, token_scores.pack_top_n, opts.scoring)
        if opts.guides is not None:
            for c in opts.guides:
                if c is not None and not c.guide.built:
                    self._build_guide(c.guide)
            self.guide_rows.send(rows, guide_kernels.pack_rows, opts.guides)

    def args(self, opts: StepLogits, seq_lengths_dev: torch.Tensor) -> Optional[LogitsArgs]:
        """The step's views (`seq_lengths_dev`: the index each row's new token takes); None for a plain step."""
        if opts.plain:
            return None
        sampled, processed, scored, guided = opts.flags
        return LogitsArgs(
            guide_kernels.GuideArgs(self.guide_masks, self.guide_rows.dev) if guided else None,
            logits_process.device_args(self.edits.dev, self.edit_rows) if processed else None,
            sampler.device_args(self.sampling.dev, seq_lengths_dev) if sampled else None,
            token_scores.device_args(self.scores.dev, self.scores.words) if scored else None)

    def fetch_scores(self, scoring):
        """Enqueue the D2H copy of a scored step's results; returns the call that reads them (one TokenLogprob or None per
        row of `scoring`) once the tokens' sync has covered the copy."""
        return functools.partial(token_scores.unpack, self.scores.fetch(), self.scores.words, scoring)
