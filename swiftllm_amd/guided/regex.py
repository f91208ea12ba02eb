"""Pattern -> trimmed byte-level DFA, for guided decoding.

The semantics are those of `re.fullmatch(pattern.encode("utf-8"), data)` on `bytes`, for the subset below; anything else
raises GuideSyntaxError with the offending position.

    literals; `\\` + a metacharacter; \\d \\D \\w \\W \\s \\S \\n \\t \\r \\f \\v \\xHH; `.` (any byte but \\n);
    classes [...] / [^...] with ranges and the escapes above; groups (...) and (?:...); `|`;
    the greedy quantifiers * + ? {m} {m,} {m,n}; an optional leading ^ and trailing $.

A non-ASCII literal is its UTF-8 byte sequence. Two refusals keep the byte semantics honest: a non-ASCII character inside
a class (a class matches ONE byte), and a quantifier directly behind a non-ASCII literal (on bytes it would bind to the last
byte only: the author groups the character). `.` is one byte, not one character.

Pipeline: recursive-descent parser -> Thompson NFA -> subset construction -> trim (every state from which no accepting
state can be reached is removed, so a surviving state always has a way to finish) -> renumber with the start state as 0.
"""
from collections import deque
from typing import List, NamedTuple, Sequence

import numpy as np

DEFAULT_MAX_STATES = 4096
_MAX_REPEAT = 1000      # (re's own limit is far higher; a bound keeps the NFA of a{m,n} small enough to build)
_NFA_STATES_PER_DFA_STATE = 8   # nested bounded repeats multiply: the NFA is refused beyond this many times max_states

_META = set(b"\\.[]()|*+?{}^$")
_DIGIT = frozenset(range(0x30, 0x3a))
_WORD = frozenset(list(range(0x30, 0x3a)) + list(range(0x41, 0x5b)) + list(range(0x61, 0x7b)) + [0x5f])
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_SIMPLE = {"n": 0x0a, "t": 0x09, "r": 0x0d, "f": 0x0c, "v": 0x0b}
_SETS = {"d": _DIGIT, "D": _ALL - _DIGIT, "w": _WORD, "W": _ALL - _WORD, "s": _SPACE, "S": _ALL - _SPACE}


class GuideSyntaxError(ValueError):
    """The pattern uses something outside the supported subset. `pos`: index into the pattern (characters)."""

    def __init__(self, msg: str, pos: int):
        super().__init__(f"{msg} at position {pos}")
        self.pos = pos


class Dfa(NamedTuple):
    trans: np.ndarray       # int32 [S, 256]: next state, -1 = dead
    accepting: np.ndarray   # bool [S]
    complete: np.ndarray    # bool [S]: accepting and no live outgoing edge — nothing can follow

    @property
    def num_states(self) -> int:
        return int(self.trans.shape[0])

    def walk(self, state: int, data: bytes) -> int:
        """The state after `data` from `state`, -1 once the walk is dead."""
        trans = self.trans
        for b in data:
            state = int(trans[state, b])
            if state < 0:
                return -1
        return state

    def accepts(self, data: bytes) -> bool:
        s = self.walk(0, data)
        return s >= 0 and bool(self.accepting[s])


# ---- parser: pattern -> AST -------------------------------------------------------------------------------------------
# nodes: ("set", frozenset of bytes) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, lo, hi or None) | ("eps",)

class _Parser:
    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0

    def fail(self, msg: str, pos: int = None):
        raise GuideSyntaxError(msg, self.i if pos is None else pos)

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        if self.peek() == "^":
            self.i += 1
        node = self.alt(top=True)
        if self.i < len(self.p):
            self.fail("unbalanced ')'" if self.peek() == ")" else f"unexpected {self.peek()!r}")
        return node

    def alt(self, top: bool = False):
        branches = [self.cat(top)]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat(top))
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self, top: bool):
        items = []
        while self.i < len(self.p):
            c = self.peek()
            if c in "|)":
                break
            if c == "$":
                # only as the pattern's last character (a top-level alternation's `a$|b` is an anchor elsewhere)
                if top and self.i == len(self.p) - 1:
                    self.i += 1
                    break
                self.fail("'$' is supported only at the end of the pattern")
            if c == "^":
                self.fail("'^' is supported only at the start of the pattern")
            start = self.i
            atom, quantifiable = self.atom()
            items.append(self.quantified(atom, quantifiable, start))
        if not items:
            return ("eps",)
        return items[0] if len(items) == 1 else ("cat", items)

    def atom(self):
        c = self.peek()
        if c == "(":
            open_at = self.i
            self.i += 1
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] == "?:":
                    self.i += 2
                else:
                    self.fail("only (?:...) groups are supported (no look-around, flags or named groups)", open_at)
            node = self.alt()
            if self.peek() != ")":
                self.fail("missing ')'", open_at)
            self.i += 1
            return node, True
        if c == "[":
            return self.cls(), True
        if c == ".":
            self.i += 1
            return ("set", _ALL - {0x0a}), True
        if c == "\\":
            return ("set", self.escape(in_class=False)), True
        if c in "*+?":
            self.fail("nothing to repeat")
        if c == "{":
            if self.brace(self.i) is not None:
                self.fail("nothing to repeat")
            self.i += 1
            return ("set", frozenset([0x7b])), True
        self.i += 1
        data = c.encode("utf-8")
        if len(data) == 1:
            return ("set", frozenset(data)), True
        return ("cat", [("set", frozenset([b])) for b in data]), False

    def escape(self, in_class: bool) -> frozenset:
        """At a backslash: consume the escape, return the set of bytes it stands for."""
        at = self.i
        self.i += 1
        c = self.peek()
        if not c:
            self.fail("pattern ends in a backslash", at)
        self.i += 1
        if c in _SETS:
            return _SETS[c]
        if c in _SIMPLE:
            return frozenset([_SIMPLE[c]])
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(d not in "0123456789abcdefABCDEF" for d in h):
                self.fail("\\x needs two hex digits", at)
            self.i += 2
            return frozenset([int(h, 16)])
        if ord(c) < 128 and not c.isalnum():     # (re: a backslash before ASCII punctuation is that character)
            return frozenset([ord(c)])
        self.fail(f"unsupported escape \\{c}", at)

    def cls(self):
        open_at = self.i
        self.i += 1
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        members = set()
        first = True
        while True:
            c = self.peek()
            if not c:
                self.fail("missing ']'", open_at)
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo_at = self.i
            lo = self.cls_item()
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.cls_item()
                if len(lo) != 1 or len(hi) != 1:
                    self.fail("a class range needs single characters at both ends", lo_at)
                a, b = next(iter(lo)), next(iter(hi))
                if a > b:
                    self.fail("class range out of order", lo_at)
                members.update(range(a, b + 1))
            else:
                members.update(lo)
        out = frozenset(members)
        return ("set", _ALL - out if negate else out)

    def cls_item(self) -> frozenset:
        c = self.peek()
        if not c:
            self.fail("missing ']'")
        if c == "\\":
            return self.escape(in_class=True)
        if ord(c) >= 128:
            self.fail("a non-ASCII character inside a class (a class matches one byte)")
        if c == "[" and self.p[self.i + 1:self.i + 2] in (":", ".", "="):
            self.fail("POSIX classes are not supported")
        self.i += 1
        return frozenset([ord(c)])

    def brace(self, at: int):
        """(lo, hi, end) when the text at `at` is a {m} / {m,} / {m,n} quantifier, None when it is a literal brace (re
        treats `{` that opens no quantifier — `{,n}` included here — as itself)."""
        j = at + 1
        k = j
        while k < len(self.p) and self.p[k].isdigit() and self.p[k].isascii():
            k += 1
        if k == j:
            if self.p[k:k + 1] == ",":         # {,n}: re reads it as {0,n}; refuse instead of guessing
                m = k + 1
                while m < len(self.p) and self.p[m].isdigit():
                    m += 1
                if self.p[m:m + 1] == "}":
                    self.fail("{,n} is not supported: write {0,n}", at)
            return None
        lo = int(self.p[j:k])
        if self.p[k:k + 1] == "}":
            return lo, lo, k + 1
        if self.p[k:k + 1] != ",":
            return None
        m = k + 1
        while m < len(self.p) and self.p[m].isdigit() and self.p[m].isascii():
            m += 1
        if self.p[m:m + 1] != "}":
            return None
        hi = int(self.p[k + 1:m]) if m > k + 1 else None
        return lo, hi, m + 1

    def quantified(self, atom, quantifiable: bool, start: int):
        c = self.peek()
        q = None
        at = self.i
        if c == "*":
            q, end = (0, None), self.i + 1
        elif c == "+":
            q, end = (1, None), self.i + 1
        elif c == "?":
            q, end = (0, 1), self.i + 1
        elif c == "{":
            b = self.brace(self.i)
            if b is not None:
                q, end = (b[0], b[1]), b[2]
        if q is None:
            return atom
        if not quantifiable:
            self.fail("a quantifier directly behind a non-ASCII literal binds to its last byte: group the character", at)
        lo, hi = q
        if hi is not None and hi < lo:
            self.fail("repeat bounds out of order", at)
        if lo > _MAX_REPEAT or (hi or 0) > _MAX_REPEAT:
            self.fail(f"repeat counts above {_MAX_REPEAT} are not supported", at)
        self.i = end
        nxt = self.peek()
        if nxt == "?":
            self.fail("lazy quantifiers are not supported")
        if nxt == "+":
            self.fail("possessive quantifiers are not supported")
        if nxt == "*" or (nxt == "{" and self.brace(self.i) is not None):
            self.fail("multiple repeat")
        return ("rep", atom, lo, hi)


# ---- Thompson NFA -----------------------------------------------------------------------------------------------------

class _Nfa:
    def __init__(self, max_nfa_states: int):
        self.eps: List[List[int]] = []
        self.edges: List[List[tuple]] = []      # per state: (frozenset of bytes, target)
        self.max_nfa_states = max_nfa_states

    def state(self) -> int:
        # (checked while the fragments are built: `((a{1000}){1000}){1000}` is refused after a few thousand states, not
        # after the billion it expands to)
        if len(self.eps) >= self.max_nfa_states:
            raise ValueError(f"the pattern expands to more than {self.max_nfa_states} NFA states (nested repeats multiply)")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(start, end) of a fragment for `node`."""
        kind = node[0]
        if kind == "eps":
            s = self.state()
            return s, s
        if kind == "set":
            s, e = self.state(), self.state()
            self.edges[s].append((node[1], e))
            return s, e
        if kind == "cat":
            s, e = self.build(node[1][0])
            for item in node[1][1:]:
                s2, e2 = self.build(item)
                self.eps[e].append(s2)
                e = e2
            return s, e
        if kind == "alt":
            s, e = self.state(), self.state()
            for br in node[1]:
                s2, e2 = self.build(br)
                self.eps[s].append(s2)
                self.eps[e2].append(e)
            return s, e
        _, inner, lo, hi = node
        s = self.state()
        e = s
        for _ in range(lo):
            s2, e2 = self.build(inner)
            self.eps[e].append(s2)
            e = e2
        if hi is None:
            s2, e2 = self.build(inner)
            loop = self.state()
            self.eps[e].append(loop)
            self.eps[loop].append(s2)
            self.eps[e2].append(loop)
            e = loop
        else:
            end = self.state()
            for _ in range(hi - lo):
                self.eps[e].append(end)
                s2, e2 = self.build(inner)
                self.eps[e].append(s2)
                e = e2
            self.eps[e].append(end)
            e = end
        return s, e

    def closure(self, states) -> frozenset:
        seen = set(states)
        stack = list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


def _determinise(nfa: _Nfa, start: int, end: int, max_states: int):
    start_set = nfa.closure([start])
    index = {start_set: 0}
    order = [start_set]
    rows = []
    queue = deque([start_set])
    while queue:
        cur = queue.popleft()
        targets = [set() for _ in range(256)]
        for s in cur:
            for byteset, t in nfa.edges[s]:
                for b in byteset:
                    targets[b].add(t)
        row = np.full(256, -1, dtype=np.int32)
        cache = {}
        for b in range(256):
            if not targets[b]:
                continue
            key = frozenset(targets[b])
            nxt = cache.get(key)
            if nxt is None:
                nxt = cache[key] = nfa.closure(key)
            j = index.get(nxt)
            if j is None:
                j = index[nxt] = len(order)
                if j >= max_states:
                    raise ValueError(f"the pattern's DFA has more than {max_states} states")
                order.append(nxt)
                queue.append(nxt)
            row[b] = j
        rows.append(row)
    trans = np.stack(rows)
    accepting = np.array([end in s for s in order], dtype=np.bool_)
    return trans, accepting


def _trim(trans: np.ndarray, accepting: np.ndarray, what: str) -> Dfa:
    """Drop every state from which no accepting state can be reached; renumber, start = 0, in BFS order from the start."""
    n = trans.shape[0]
    preds = [[] for _ in range(n)]
    for s in range(n):
        for t in set(trans[s][trans[s] >= 0].tolist()):
            preds[t].append(s)
    live = np.zeros(n, dtype=np.bool_)
    stack = [int(s) for s in np.flatnonzero(accepting)]
    live[stack] = True
    while stack:
        for p in preds[stack.pop()]:
            if not live[p]:
                live[p] = True
                stack.append(p)
    if not live[0]:
        raise ValueError(f"{what} matches nothing")
    new_id = np.full(n, -1, dtype=np.int32)
    order = [0]
    new_id[0] = 0
    for s in order:     # (grows while it is walked: BFS)
        for t in trans[s].tolist():
            if t >= 0 and live[t] and new_id[t] < 0:
                new_id[t] = len(order)
                order.append(t)
    out = trans[order]
    out = np.where(out >= 0, new_id[np.maximum(out, 0)], -1).astype(np.int32)
    acc = accepting[order].copy()
    complete = acc & ~(out >= 0).any(axis=1)
    return Dfa(np.ascontiguousarray(out), acc, complete)


def compile_regex(pattern: str, max_states: int = DEFAULT_MAX_STATES) -> Dfa:
    """The trimmed byte DFA of `pattern`. GuideSyntaxError: outside the subset; ValueError: matches nothing, or more than
    `max_states` DFA states (counted before trimming), or an NFA of more than 8 * max_states + 64 states."""
    if not isinstance(pattern, str):
        raise GuideSyntaxError("the pattern must be a str", 0)
    ast = _Parser(pattern).parse()
    nfa = _Nfa(_NFA_STATES_PER_DFA_STATE * max(int(max_states), 1) + 64)
    start, end = nfa.build(ast)
    trans, accepting = _determinise(nfa, start, end, max_states)
    return _trim(trans, accepting, "the pattern")


def compile_choice(choices: Sequence[str], max_states: int = DEFAULT_MAX_STATES) -> Dfa:
    """The DFA that accepts exactly the given strings (UTF-8): a trie."""
    choices = list(choices)
    if not choices:
        raise ValueError("guided_choice needs at least one choice")
    if any(not isinstance(c, str) for c in choices):
        raise ValueError("guided_choice entries must be str")
    if any(c == "" for c in choices):
        raise ValueError("guided_choice entries must not be empty")
    if len(set(choices)) != len(choices):
        raise ValueError("guided_choice names a choice twice")
    rows = [np.full(256, -1, dtype=np.int32)]
    accepting = [False]
    for c in choices:
        s = 0
        for b in c.encode("utf-8"):
            t = int(rows[s][b])
            if t < 0:
                t = len(rows)
                if t >= max_states:
                    raise ValueError(f"the choices' trie has more than {max_states} states")
                rows.append(np.full(256, -1, dtype=np.int32))
                accepting.append(False)
                rows[s][b] = t
            s = t
        accepting[s] = True
    return _trim(np.stack(rows), np.array(accepting, dtype=np.bool_), "the choice list")
