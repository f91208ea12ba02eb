"""Host bookkeeping of the guided-decoding mask pool, and the cursor a guided request walks through its guide.

The device pool is `masks: int32 [max_states, W]`, W = ceil(vocab_size / 32): bit (t & 31) of word (t >> 5) of row
`guide.base + s` is set when token t may be picked in state s. This module never touches the device: it hands out row
ranges, and the model thread fills the rows of a guide whose `built` is still false (worker/model.py)."""
import threading
from collections import OrderedDict
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from .regex import DEFAULT_MAX_STATES, Dfa, compile_choice, compile_regex
from .vocab import TokenVocab

KINDS = ("regex", "choice", "tokens")


class GuideViolation(AssertionError):
    """A cursor was advanced with a token its state does not allow. With the mask applied this happens only when the state
    allows NO token (its row is empty: the vocabulary spells none of the bytes the guide needs there, or the only such
    token is an end id of a state that does not accept): whatever the picker returns from an all -inf row is not allowed."""


class GuideStoreFull(RuntimeError):
    """Every row the guide would need is held by a live request: try again later."""


def words_per_row(vocab_size: int) -> int:
    return (int(vocab_size) + 31) // 32


def guide_key(kind: str, spec, end_ids: Sequence[int] = ()) -> tuple:
    """(kind, pattern-or-tuple, end_ids): `spec` is the pattern (regex), the choices (choice) or the allowed ids (tokens)."""
    if kind not in KINDS:
        raise ValueError(f"unknown guide kind {kind!r}")
    if kind == "regex":
        if not isinstance(spec, str):
            raise ValueError("a regex guide's pattern must be a str")
    elif kind == "choice":
        spec = tuple(spec)
    else:
        spec = tuple(sorted(set(int(t) for t in spec)))
        end_ids = ()        # (an allowed-token guide is never accepting: its end ids never matter)
    return kind, spec, tuple(sorted(set(int(t) for t in end_ids)))


class Guide:
    """One guide resident in the pool: rows [base, base + num_states)."""
    __slots__ = ("key", "kind", "dfa", "base", "num_states", "end_ids", "allowed", "vocab", "built", "refs", "evicted")

    def __init__(self, key, dfa: Optional[Dfa], base: int, num_states: int, vocab: Optional[TokenVocab]):
        self.key = key
        self.kind = key[0]
        self.dfa = dfa
        self.base = base
        self.num_states = num_states
        self.end_ids: Tuple[int, ...] = key[2]
        self.allowed: Optional[Tuple[int, ...]] = key[1] if self.kind == "tokens" else None
        self.vocab = vocab
        self.built = False      # set by the model thread once the rows hold this guide's masks
        self.refs = 0
        self.evicted = False

    def host_mask_row(self, words: int) -> np.ndarray:
        """The one mask row of an allowed-token guide, int32 [words]."""
        row = np.zeros(words, dtype=np.uint32)
        ids = np.asarray(self.allowed, dtype=np.int64)
        if ids.size and int(ids.max()) >= 32 * words:
            raise ValueError("an allowed token id does not fit the mask row")
        np.bitwise_or.at(row, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
        return row.view(np.int32)


class GuideStore:
    def __init__(self, max_states: int, vocab_size: int, vocab: Optional[TokenVocab] = None,
                 max_dfa_states: Optional[int] = None, dfa_cache_size: int = 256):
        if max_states <= 0:
            raise ValueError("GuideStore needs max_states > 0")
        self.max_states = int(max_states)
        self.vocab_size = int(vocab_size)
        self.words = words_per_row(vocab_size)
        self.vocab = vocab
        self.max_dfa_states = int(max_dfa_states or DEFAULT_MAX_STATES)    # (counted before trimming)
        self._lock = threading.Lock()           # the table: acquire (event-loop side) and release (model thread)
        self._compile_lock = threading.Lock()   # the DFA cache: submitters only — a compile never delays a release
        self._guides: "OrderedDict[tuple, Guide]" = OrderedDict()       # resident guides, least recently used first
        self._dfas: "OrderedDict[tuple, Dfa]" = OrderedDict()
        self._dfa_cache_size = dfa_cache_size
        self.num_compiles = 0
        self.num_evictions = 0
        # (tests replace these to count compiles)
        self._compilers: dict = {"regex": compile_regex, "choice": compile_choice}

    # ---- DFA cache ---------------------------------------------------------------------------------------------------
    def _dfa_for(self, key) -> Dfa:
        ckey = key[:2]
        with self._compile_lock:
            dfa = self._dfas.get(ckey)
            if dfa is not None:
                self._dfas.move_to_end(ckey)
                return dfa
            compiler: Callable = self._compilers[key[0]]
            dfa = compiler(key[1], max_states=self.max_dfa_states)
            self.num_compiles += 1
            self._dfas[ckey] = dfa
            while len(self._dfas) > self._dfa_cache_size:
                self._dfas.popitem(last=False)
            return dfa

    # ---- the pool ----------------------------------------------------------------------------------------------------
    def _first_fit(self, need: int, ignore=()) -> int:
        """The lowest base of a free range of `need` rows, -1 when there is none; the guides in `ignore` count as free."""
        at = 0
        for g in sorted((g for g in self._guides.values() if g not in ignore), key=lambda g: g.base):
            if g.base - at >= need:
                return at
            at = g.base + g.num_states
        return at if self.max_states - at >= need else -1

    def acquire(self, key) -> Guide:
        """Take one reference on the guide of `key`, making it resident if it is not: first fit over the free row ranges;
        when nothing fits, guides no live request holds are evicted, least recently used first; GuideStoreFull after that.
        ValueError (GuideSyntaxError is one): the guide can never be served."""
        kind, spec, end_ids = key
        with self._lock:
            g = self._guides.get(key)
            if g is not None:
                g.refs += 1
                self._guides.move_to_end(key)
                return g
        if kind == "tokens":
            if not spec:
                raise ValueError("allowed_token_ids must name at least one id")
            if spec[0] < 0 or spec[-1] >= self.vocab_size:
                raise ValueError(f"allowed_token_ids must lie in [0, {self.vocab_size})")
            dfa, need = None, 1
        else:
            if self.vocab is None:
                raise ValueError("this store has no vocabulary: only allowed_token_ids guides can be served")
            dfa = self._dfa_for(key)
            need = dfa.num_states
        if need > self.max_states:
            raise ValueError(f"the guide needs {need} mask rows, the pool holds {self.max_states}")
        with self._lock:
            g = self._guides.get(key)       # (another submitter made it resident meanwhile)
            if g is not None:
                g.refs += 1
                self._guides.move_to_end(key)
                return g
            base = self._first_fit(need)
            if base < 0:
                # idle guides are given up, least recently used first, until a hole fits; only those that lie in the hole
                # that is taken are evicted — the others keep their rows and their built masks — and none is, when even
                # all of them would not make the room
                candidates = []
                for victim in [v for v in self._guides.values() if v.refs == 0]:
                    candidates.append(victim)
                    base = self._first_fit(need, candidates)
                    if base >= 0:
                        break
                for victim in candidates if base >= 0 else ():
                    if victim.base < base + need and base < victim.base + victim.num_states:
                        del self._guides[victim.key]
                        victim.evicted = True
                        self.num_evictions += 1
            if base < 0:
                raise GuideStoreFull(f"no room for a guide of {need} states: all {self.max_states} mask rows are held by "
                                     "live requests")
            g = Guide(key, dfa, base, need, self.vocab)
            g.refs = 1
            self._guides[key] = g
            return g

    def release(self, guide: Guide):
        """Drop one reference. The guide stays resident (and built) until its rows are needed for another."""
        with self._lock:
            if guide.refs <= 0:
                raise RuntimeError("release of a guide nobody holds")
            guide.refs -= 1

    def resident(self) -> list:
        with self._lock:
            return list(self._guides.values())


class GuideCursor:
    """Where one request stands in its guide. The caller advances it with every delivered token."""
    __slots__ = ("guide", "state", "text", "released")

    def __init__(self, guide: Guide):
        self.guide = guide
        self.state = 0
        self.text = b""
        self.released = False       # (the holder's note that it gave its reference on the guide back: once only)

    @property
    def mask_row(self) -> int:
        return self.guide.base + self.state

    @property
    def complete(self) -> bool:
        g = self.guide
        return g.dfa is not None and bool(g.dfa.complete[self.state])

    @property
    def accepting(self) -> bool:
        g = self.guide
        return g.dfa is not None and bool(g.dfa.accepting[self.state])

    def advance(self, token_id: int):
        """Walk the token's bytes. A token the state's mask does not allow raises GuideViolation (an AssertionError): with
        the mask applied it cannot be picked unless the state allows nothing at all — the engine ends such a request with
        an error. The cursor is unchanged when it raises."""
        g = self.guide
        if g.dfa is None:
            if token_id not in g.allowed:
                raise GuideViolation(f"token {token_id} is not among the guide's allowed ids")
            data = g.vocab.token_bytes(token_id) if g.vocab is not None else None
            self.text += data or b""
            return
        if token_id in g.end_ids:
            if not g.dfa.accepting[self.state]:
                raise GuideViolation(f"end token {token_id} in state {self.state}, which is not accepting")
            return
        data = g.vocab.token_bytes(token_id)
        if not data:
            raise GuideViolation(f"token {token_id} spells nothing: a guide never allows it")
        nxt = g.dfa.walk(self.state, data)
        if nxt < 0:
            raise GuideViolation(f"token {token_id} ({data!r}) leaves the guide from state {self.state}")
        self.state = nxt
        self.text += data
