"""worker/step_logits.py on the CPU: what a step's logits options decide about its graph and its look-ahead (StepLogits),
and the growth arithmetic of the staged buffers (StagedInts over ordinary CPU tensors)."""
import itertools

import torch

from swiftllm_amd import SamplingParams
from swiftllm_amd.worker.step_logits import PLAIN, StagedInts, StepLogits


def test_flags_name_the_options_in_use_and_nothing_else():
    for flags in itertools.product((False, True), repeat=4):
        a = StepLogits(*[[None, 1] if on else None for on in flags])
        b = StepLogits(*[["other", "contents", None] if on else None for on in flags])
        assert a.flags == b.flags == flags and a.plain == (not any(flags))
        assert hash(a.flags) == hash(flags)            # (part of the replay key)
        assert StepLogits.of(a.sampling, a.edits, a.scoring, a.guides).flags == flags
    assert PLAIN.flags == (False,) * 4 and PLAIN.plain
    assert StepLogits.of() is PLAIN and StepLogits.of(None, None, None, None) is PLAIN      # a plain step constructs nothing
    assert StepLogits.of(scoring=[None]) is not PLAIN


def test_continues_is_the_lookahead_rule():
    hot = SamplingParams(0.8, seed=5)
    prev = StepLogits([None, hot], ["edits of step k"], [None, 5], ["cursor at state 3"])
    # entries and cursors differ in content: still the continuation
    assert StepLogits([None, SamplingParams(0.8, seed=5)], ["edits of step k + 1"], [None, 5], ["at state 4"]).continues(prev)
    assert PLAIN.continues(PLAIN) and StepLogits().continues(PLAIN) and prev.continues(prev)
    for other in (StepLogits([None, SamplingParams(0.8, seed=6)], ["e"], [None, 5], ["c"]),   # only the resolved seed
                  StepLogits([hot, None], ["e"], [None, 5], ["c"]),                           # another row draws
                  StepLogits(None, ["e"], [None, 5], ["c"]),                                  # no longer sampled
                  StepLogits([None, hot], ["e"], [None, 3], ["c"]),                           # another N
                  StepLogits([None, hot], ["e"], None, ["c"]),                                # no longer scored
                  StepLogits([None, hot], None, [None, 5], ["c"]),                            # no longer processed
                  StepLogits([None, hot], ["e"], [None, 5], None),                            # no longer guided
                  PLAIN):
        assert not other.continues(prev) and not prev.continues(other)
    for one in (dict(sampling=[hot]), dict(edits=["e"]), dict(scoring=[2]), dict(guides=["c"])):
        assert not StepLogits(**one).continues(PLAIN) and not PLAIN.continues(StepLogits(**one)), one


def test_a_hit_resends_entries_and_mask_rows_only():
    full = StepLogits(["s"], ["e"], [5], ["c"])
    again = full.resend_on_hit
    assert (again.sampling, again.edits, again.scoring, again.guides) == (None, ["e"], None, ["c"])
    assert StepLogits(["s"], None, [5], None).resend_on_hit is PLAIN and PLAIN.resend_on_hit is PLAIN


def test_a_lookahead_built_without_arguments_is_a_plain_steps():
    from swiftllm_amd.worker.decode_replay import _DecodeLookahead
    la = _DecodeLookahead()
    assert la.logits is PLAIN and PLAIN.continues(la.logits)
    assert not StepLogits(scoring=[1]).continues(la.logits)
    la.logits = StepLogits(scoring=[1])             # (assignable field by field)
    assert StepLogits(scoring=[1]).continues(la.logits)


def test_staged_ints_grow_by_doubling_and_tell_their_owner():
    moves, made = [], []

    def alloc(words, pinned):
        made.append((words, pinned))
        return torch.full((words,), 12345, dtype=torch.int32)      # (garbage, as fresh memory is)
    for idle, tail in ((0, 0), (-1, 0), (-1, 43)):
        del moves[:], made[:]
        buf = StagedInts(lambda: moves.append(1), idle=idle, tail=tail, alloc=alloc)
        assert buf.words == 0 and buf.dev is None
        assert buf.ensure(20) and moves == [1] and buf.words == 20
        assert made[:2] == [(20, True), (20 * (1 + tail), False)]
        first = buf.dev
        assert not buf.ensure(20) and not buf.ensure(1) and buf.dev is first and moves == [1]      # below capacity: stays
        buf.begin()[:] = 7                                          # (no copy yet: begin waits for nothing)
        assert buf.ensure(21) and moves == [1, 1] and buf.words == 40 and buf.dev is not first    # 21 asked: doubled
        assert buf.ensure(200) and moves == [1, 1, 1] and buf.words == 200                       # beyond twice: what is asked
        assert buf.host.numel() == buf.host_np.size == 200 and buf.dev.numel() == 200 * (1 + tail)
        assert bool((buf.dev[:200] == idle).all()) and bool((buf.dev[200:] == 0).all())
        assert buf.back.numel() == buf.back_np.size == 200 * tail
        buf.resize(8)                                               # the owner's own rule (the edit buffer): exactly this
        assert buf.words == 8 and len(moves) == 4 and bool((buf.dev[:8] == idle).all())


def test_the_staged_plan_moves_only_when_a_plan_outgrows_it(monkeypatch):
    """decode_replay.stage_plan on CPU tensors (the copies' event is a recorder: there is no device to record on): a plan
    within the capacity leaves the twin where it is, a larger one moves it and tells the owner exactly once, and the views
    returned are the plan's packed layout over the twin, holding what the plan holds."""
    from swiftllm_amd.worker.batch_plan import plan_batch
    from swiftllm_amd.worker.decode_replay import plan_decode, stage_plan
    waits = []

    class Event:
        def record(self):
            waits.append("record")

        def synchronize(self):
            waits.append("wait")
    monkeypatch.setattr(torch.cuda, "Event", Event)
    moves = []
    ints = StagedInts(lambda: moves.append(1), alloc=lambda words, pinned: torch.full((words,), 12345, dtype=torch.int32))

    def check(plan, dev):
        layout, total = plan.packed_layout()
        assert list(dev) == [name for name, _, _ in layout] and sum(n for _, _, n in layout) <= total <= ints.words
        for name, off, n in layout:
            assert dev[name].numel() == n and (n == 0 or dev[name].data_ptr() == ints.dev.data_ptr() + 4 * off), name
            assert dev[name].tolist() == ints.host[off:off + n].tolist(), name
        for name in ("input_ids", "seq_ids", "decoding_seq_lens", "position_indices"):
            assert dev[name].tolist() == getattr(plan, name).tolist(), name

    small = plan_decode([7, 3, 9], [1100, 37, 5], [[11], [12], [13]], True, 8, 256)
    total = small.packed_layout()[1]
    check(small, stage_plan(ints, small, floor=total + 40))
    assert moves == [1] and ints.words == total + 40 and waits == ["record"]      # the first capacity: the floor
    assert bool((ints.dev[total:] == 0).all())       # (one copy of the plan's words: past them the fresh twin's zeros)
    twin = ints.dev
    check(small, stage_plan(ints, small, floor=total + 40))
    other = plan_batch([[5, 6, 7], [8]], [2, 1], [9], 8, 256)      # a prompt and a decode: another layout, still within
    assert other.packed_layout()[1] <= ints.words
    check(other, stage_plan(ints, other))
    assert moves == [1] and ints.dev is twin and waits == ["record"] + ["wait", "record"] * 2
    big = plan_decode(list(range(40)), [50] * 40, None, True, 8, 256)
    assert big.packed_layout()[1] > ints.words
    check(big, stage_plan(ints, big, floor=total + 40))
    assert moves == [1, 1] and ints.dev is not twin and ints.words >= big.packed_layout()[1]
    twin = ints.dev
    check(small, stage_plan(ints, small))           # a smaller plan afterwards: stays
    assert moves == [1, 1] and ints.dev is twin
