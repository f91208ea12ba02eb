"""swiftllm_amd/guided/store.py: the host bookkeeping of the mask pool, and the cursor."""
import threading

import numpy as np
import pytest

from swiftllm_amd.guided import (GuideCursor, GuideStore, GuideStoreFull, GuideSyntaxError, TokenVocab, guide_key)

VOCAB = TokenVocab([bytes([b]) for b in range(256)] + [b"ab", b"12", b"yes", b"no", None, None])     # 260: eos, 261: eos2
V = len(VOCAB)
EOS = 260


def store(rows: int) -> GuideStore:
    return GuideStore(rows, V, VOCAB)


def test_first_fit_and_reuse_after_release():
    s = store(16)
    a = s.acquire(guide_key("regex", "abc"))             # 4 states
    b = s.acquire(guide_key("regex", "[0-9]{2}"))        # 3 states
    c = s.acquire(guide_key("regex", "xy"))              # 3 states
    assert (a.base, a.num_states, b.base, b.num_states, c.base, c.num_states) == (0, 4, 4, 3, 7, 3)
    assert not a.built and a.refs == 1
    # a second request with the same key shares the guide
    assert s.acquire(guide_key("regex", "abc")) is a and a.refs == 2
    s.release(a)
    s.release(a)
    s.release(b)
    # released guides stay resident while there is room: the next one goes behind them
    d = s.acquire(guide_key("regex", "pq"))              # 3 states
    assert d.base == 10 and s.num_evictions == 0
    # and are found again, built flag and all
    b.built = True
    assert s.acquire(guide_key("regex", "[0-9]{2}")) is b and b.built and b.refs == 1
    s.release(b)
    # no room at the end (3 rows left): a 4-state guide evicts idle guides, least recently used first — `a` — and takes
    # the first hole that fits
    e = s.acquire(guide_key("regex", "wxy"))             # 4 states
    assert e.base == 0 and a.evicted and not b.evicted and s.num_evictions == 1
    # the evicted guide's key builds a NEW guide (not built). Only `b` is idle now and its 3 rows are not enough: nothing
    # is evicted for nothing
    with pytest.raises(GuideStoreFull):
        s.acquire(guide_key("regex", "abc"))
    assert not b.evicted and s.num_evictions == 1
    s.release(c)                                         # rows 7..9 next to b's 4..6: both go, and the hole fits
    a2 = s.acquire(guide_key("regex", "abc"))
    assert a2 is not a and not a2.built and b.evicted and c.evicted and a2.base == 4 and s.num_evictions == 3


def test_only_the_guides_in_the_hole_that_is_taken_are_evicted():
    s = store(13)
    a = s.acquire(guide_key("regex", "abc"))             # rows 0..3: the least recently used, and not next to any room
    b = s.acquire(guide_key("regex", "xy"))              # rows 4..6, held
    c = s.acquire(guide_key("regex", "pq"))              # rows 7..9; rows 10..12 are free
    for g in (a, c):
        s.release(g)
    a.built = c.built = True
    d = s.acquire(guide_key("regex", "vwxyz"))           # 6 states: `a` alone does not help, `c` next to the free rows does
    assert d.base == 7 and c.evicted and s.num_evictions == 1 and b.refs == 1
    assert not a.evicted and a.built and s.acquire(guide_key("regex", "abc")) is a       # kept its rows and its masks


def test_eviction_takes_idle_guides_only_and_full_raises():
    s = store(8)
    a = s.acquire(guide_key("regex", "abc"))             # rows 0..3, held
    b = s.acquire(guide_key("regex", "xy"))              # rows 4..6, held
    with pytest.raises(GuideStoreFull):
        s.acquire(guide_key("regex", "pq"))
    assert not a.evicted and not b.evicted and a.refs == b.refs == 1
    s.release(b)
    c = s.acquire(guide_key("regex", "pq"))              # takes b's rows
    assert b.evicted and not a.evicted and c.base == 4
    with pytest.raises(GuideStoreFull):
        s.acquire(guide_key("regex", "rs"))
    # a guide larger than the whole pool can never be served: a ValueError, not "try later"
    with pytest.raises(ValueError) as info:
        s.acquire(guide_key("regex", "abcdefghij"))
    assert not isinstance(info.value, GuideStoreFull)
    with pytest.raises(RuntimeError):
        s.release(b)                                     # nobody holds it


def test_one_compile_per_key_and_errors_pass_through():
    s = store(64)
    calls = []
    real = s._compilers["regex"]
    s._compilers["regex"] = lambda p, max_states: (calls.append(p), real(p, max_states=max_states))[1]
    g1 = s.acquire(guide_key("regex", "a+b", (EOS,)))
    g2 = s.acquire(guide_key("regex", "a+b", (EOS,)))
    g3 = s.acquire(guide_key("regex", "a+b", (EOS, 261)))        # other end ids: another guide, the same DFA
    assert g1 is g2 and g3 is not g1 and g3.dfa is g1.dfa and calls == ["a+b"] and s.num_compiles == 1
    for g in (g1, g2, g3):
        s.release(g)
    for _ in range(3):                                   # evicted and acquired again: still one compile
        s.release(s.acquire(guide_key("regex", "a+b", (EOS,))))
    assert calls == ["a+b"]
    with pytest.raises(GuideSyntaxError):
        s.acquire(guide_key("regex", "a(?=b)"))
    with pytest.raises(ValueError, match="more than"):
        GuideStore(64, V, VOCAB, max_dfa_states=8).acquire(guide_key("regex", "[ab]*a[ab]{5}"))
    assert s.acquire(guide_key("choice", ["yes", "no"])).dfa.accepts(b"no")
    with pytest.raises(ValueError):
        s.acquire(guide_key("choice", ["yes", "yes"]))


def test_allowed_token_ids_is_a_one_state_guide_written_by_the_host():
    s = store(4)
    g = s.acquire(guide_key("tokens", [70, 3, 3, 259], (EOS,)))
    assert g.key == ("tokens", (3, 70, 259), ()) and g.num_states == 1 and g.dfa is None and not g.built
    row = g.host_mask_row(s.words).view(np.uint32)
    assert row.dtype == np.uint32 and row.shape == (9,)
    want = np.zeros(9, dtype=np.uint32)
    for t in (3, 70, 259):
        want[t >> 5] |= np.uint32(1 << (t & 31))
    assert (row == want).all()
    cur = GuideCursor(g)
    assert cur.mask_row == g.base and not cur.complete and not cur.accepting
    cur.advance(70)
    cur.advance(259)
    assert cur.mask_row == g.base and not cur.complete and cur.text == b"Fno"
    with pytest.raises(AssertionError):
        cur.advance(4)
    with pytest.raises(ValueError):
        s.acquire(guide_key("tokens", [V]))
    with pytest.raises(ValueError):
        s.acquire(guide_key("tokens", []))


def test_cursor_walks_tokens_and_end_ids():
    s = store(32)
    g = s.acquire(guide_key("regex", "ab(12)?", (EOS,)))
    cur = GuideCursor(g)
    assert cur.mask_row == g.base and cur.text == b"" and not cur.complete
    cur.advance(256)                                     # "ab"
    assert cur.accepting and not cur.complete and cur.text == b"ab" and cur.mask_row == g.base + g.dfa.walk(0, b"ab")
    at = cur.state
    cur.advance(EOS)                                     # an end id in an accepting state: the state stays
    assert cur.state == at and cur.text == b"ab"
    cur.advance(ord("1"))
    assert not cur.accepting
    with pytest.raises(AssertionError):
        cur.advance(EOS)                                 # not accepting here
    with pytest.raises(AssertionError):
        cur.advance(ord("x"))                            # leaves the guide
    with pytest.raises(AssertionError):
        cur.advance(261)                                 # spells nothing and is no end id of this guide
    cur.advance(ord("2"))
    assert cur.complete and cur.text == b"ab12"


def test_acquire_and_release_from_two_threads():
    s = store(64)
    keys = [guide_key("regex", p) for p in ("abc", "x[0-9]y", "(yes|no)", "a{3}")]
    errors = []

    def submit():
        try:
            for i in range(300):
                g = s.acquire(keys[i % len(keys)])
                held.append(g)
        except Exception as exc:     # noqa: BLE001
            errors.append(exc)

    def retire():
        try:
            done = 0
            while done < 300:
                try:
                    g = held.pop()
                except IndexError:
                    continue
                s.release(g)
                done += 1
        except Exception as exc:     # noqa: BLE001
            errors.append(exc)

    held = []
    threads = [threading.Thread(target=submit), threading.Thread(target=retire)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30)
    assert not errors and not held
    assert all(g.refs == 0 for g in s.resident()) and len(s.resident()) == len(keys) and s.num_compiles == len(keys)
    # the resident ranges are disjoint and inside the pool
    spans = sorted((g.base, g.base + g.num_states) for g in s.resident())
    assert spans[0][0] >= 0 and spans[-1][1] <= 64 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
