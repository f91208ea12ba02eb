"""swiftllm_amd/guided/regex.py against Python's `re` on bytes: for every pattern, every byte string over a small alphabet
up to length 6 is accepted exactly when re.fullmatch(pattern.encode(), s) matches. Then what the DFA promises beyond that:
it is trimmed, `complete` is its definition, the unsupported constructs are refused, the state cap holds."""
import itertools
import re
from collections import deque

import numpy as np
import pytest

from swiftllm_amd.guided import Dfa, GuideSyntaxError, compile_choice, compile_regex

# (pattern, alphabet as bytes: 4-6 symbols chosen to hit both sides of the pattern)
PATTERNS = [
    ("abc", b"abcd"),
    ("a|b|cd", b"abcd"),
    ("a*", b"ab\n "),
    ("a+b?", b"abc\n"),
    ("(ab)*c", b"abc "),
    ("(?:ab|c)+", b"abcd"),
    ("((a|b)(c|d))*", b"abcd"),
    ("(a(b(c)?)?)?d", b"abcd"),
    ("a{2}", b"ab\n0"),
    ("a{2,}", b"ab\n0"),
    ("a{1,3}b", b"ab\n0"),
    ("(ab){0,2}", b"abc "),
    ("a{0}b", b"ab\n0"),
    ("[abc]+", b"abcd"),
    ("[^abc]+", b"abd\n"),
    ("[a-c]x", b"abcxd"),
    ("[^a-c\\n]", b"abd\n "),
    ("[]a]+", b"]a[b"),
    ("[a\\-c]+", b"a-cb"),
    ("[a-]+", b"a-b "),
    ("[\\d.]+", b"09.a "),
    ("\\d+", b"09a "),
    ("\\D", b"09a\n"),
    ("\\w+", b"a_9- "),
    ("\\W", b"a_9-\n"),
    ("\\s+", b" \t\na\x0b"),
    ("\\S\\s", b" \ta\n"),
    ("a.b", b"ab\n\xff"),
    (".*", b"a\n\xc3\xa9"),
    ("\\n\\t\\r", b"\n\t\r "),
    ("\\f\\v?", b"\x0c\x0b a"),
    ("\\x41\\x0a", b"A\na "),
    ("[\\x00-\\x1f]+", b"\x00\x1f\x20a"),
    ("\\.\\*\\+\\?", b".*+?a"),
    ("\\(a\\)\\[\\]", b"()a[]"),
    ("\\{\\}|a{b|{}", b"{}ab"),
    ("a\\|b\\\\", b"a|b\\"),
    ("^ab$", b"ab\n "),
    ("^(a|b)+$", b"ab\n "),
    ("é", b"\xc3\xa9a "),
    ("caf(é)+", b"caf\xc3\xa9"),
    ("a(?:é|b)*", b"ab\xc3\xa9 "),
    ("-?(0|[1-9]\\d*)", b"-019 "),
    ("(yes|no|maybe)", b"yesnom"),
    ("(yes|no|maybe)", b"maybe"),
    ("|a", b"ab\n "),
    ("(|a)b", b"ab\n "),
    ("x{2}y{1,2}(z|x{0,1})", b"xyz "),
]


def all_strings(alphabet: bytes, max_len: int = 6):
    syms = [bytes([b]) for b in alphabet]
    for n in range(max_len + 1):
        for combo in itertools.product(syms, repeat=n):
            yield b"".join(combo)


@pytest.mark.parametrize("pattern,alphabet", PATTERNS, ids=[repr(p[0]) + "/" + p[1].hex() for p in PATTERNS])
def test_dfa_agrees_with_re_fullmatch_on_every_short_string(pattern, alphabet):
    assert 4 <= len(alphabet) <= 6
    dfa = compile_regex(pattern)
    oracle = re.compile(pattern.encode("utf-8"))
    reached = set()
    for s in all_strings(alphabet):
        want = oracle.fullmatch(s) is not None
        st = dfa.walk(0, s)
        assert (st >= 0 and bool(dfa.accepting[st])) == want == dfa.accepts(s), (pattern, s)
        if st >= 0:
            reached.add(st)
    check_shape(dfa)
    # trimmed: from every state some enumerated prefix reaches (and from every state there is), an accepting state is
    # reachable (BFS over the transitions)
    for st in reached | set(range(dfa.num_states)):
        assert can_finish(dfa, st), (pattern, st)


def check_shape(dfa: Dfa):
    s = dfa.num_states
    assert dfa.trans.dtype == np.int32 and dfa.trans.shape == (s, 256) and dfa.trans.flags.c_contiguous
    assert dfa.accepting.dtype == np.bool_ and dfa.accepting.shape == (s,)
    assert dfa.complete.dtype == np.bool_ and dfa.complete.shape == (s,)
    assert int(dfa.trans.min()) >= -1 and int(dfa.trans.max()) < s
    # `complete`: accepting and no live outgoing edge
    for st in range(s):
        assert bool(dfa.complete[st]) == (bool(dfa.accepting[st]) and not (dfa.trans[st] >= 0).any())
    # every state is reachable from state 0 (the start)
    seen, queue = {0}, deque([0])
    while queue:
        for t in set(dfa.trans[queue.popleft()].tolist()) - {-1}:
            if t not in seen:
                seen.add(t)
                queue.append(t)
    assert seen == set(range(s))


def can_finish(dfa: Dfa, state: int) -> bool:
    seen, queue = {state}, deque([state])
    while queue:
        st = queue.popleft()
        if dfa.accepting[st]:
            return True
        for t in set(dfa.trans[st].tolist()) - {-1}:
            if t not in seen:
                seen.add(t)
                queue.append(t)
    return False


def test_complete_states_of_known_patterns():
    dfa = compile_regex("ab?")
    assert not dfa.complete[0]
    a = dfa.walk(0, b"a")
    assert dfa.accepting[a] and not dfa.complete[a]         # 'b' may still follow
    ab = dfa.walk(0, b"ab")
    assert dfa.accepting[ab] and dfa.complete[ab]
    assert not compile_regex("a*").complete.any()


def test_trimming_removes_states_that_cannot_finish():
    # `[^\x00-\xff]` matches no byte: the branch behind it is dead and must not survive as states
    dfa = compile_regex("ab|a[^\\x00-\\xff]c")
    assert dfa.num_states == 3 and dfa.walk(0, b"a") >= 0 and dfa.walk(0, b"ac") == -1


REFUSED = [
    ("(a)\\1", "back-reference"), ("a(?=b)", "look-ahead"), ("a(?!b)", "negative look-ahead"), ("(?<=a)b", "look-behind"),
    ("a*?", "lazy"), ("a+?", "lazy"), ("a??", "lazy"), ("a{1,2}?", "lazy"), ("a*+", "possessive"), ("a++", "possessive"),
    ("(?i)a", "flags"), ("(?P<n>a)", "named group"), ("a^b", "anchor elsewhere"), ("a$b", "anchor elsewhere"),
    ("(a$)", "anchor elsewhere"), ("a|^b", "anchor elsewhere"), ("\\bword", "\\b"), ("a\\B", "\\B"), ("\\Aa", "\\A"),
    ("a\\Z", "\\Z"), ("[é]", "non-ASCII in a class"), ("[a-é]", "non-ASCII in a class"), ("é+", "quantified non-ASCII"),
    ("é{2}", "quantified non-ASCII"), ("é?", "quantified non-ASCII"), ("*a", "nothing to repeat"), ("(+a)", "nothing to repeat"),
    ("a**", "multiple repeat"), ("a{2}{3}", "multiple repeat"), ("(a", "unbalanced"), ("a)", "unbalanced"), ("[a", "unbalanced"),
    ("a\\", "trailing backslash"), ("\\xg1", "bad hex"), ("[z-a]", "range out of order"), ("a{3,2}", "bounds out of order"),
    ("[\\d-z]", "set as a range end"), ("a{,2}", "{,n}"), ("\\p{L}", "unicode property"), ("[[:alpha:]]", "POSIX class"),
    ("a{2000}", "repeat count"),
]


@pytest.mark.parametrize("pattern,what", REFUSED, ids=[r[1] + ": " + repr(r[0]) for r in REFUSED])
def test_unsupported_constructs_are_refused_with_a_position(pattern, what):
    with pytest.raises(GuideSyntaxError) as info:
        compile_regex(pattern)
    assert isinstance(info.value, ValueError)
    assert 0 <= info.value.pos <= len(pattern) and "position" in str(info.value)


def test_a_pattern_that_matches_nothing_is_refused():
    with pytest.raises(ValueError, match="matches nothing"):
        compile_regex("a[^\\x00-\\xff]")
    with pytest.raises(ValueError, match="matches nothing"):
        compile_regex("[^\\d\\D]+")


def test_nested_repeats_are_refused_before_they_are_expanded():
    # bounded repeats multiply when nested: the NFA is bounded while it is built (8 * max_states + 64 states), with the
    # ValueError of an oversized DFA, long before memory or time are spent
    for pattern in ("(a{1000}){1000}", "((a{1000}){1000}){1000}", "((((a{9}){9}){9}){9}){9}", "(a{0,1000}){0,1000}"):
        with pytest.raises(ValueError, match="NFA states") as info:
            compile_regex(pattern)
        assert not isinstance(info.value, GuideSyntaxError)
    with pytest.raises(ValueError, match="NFA states"):
        compile_regex("(a{10}){10}", max_states=4)           # the bound follows max_states: 96 here
    assert compile_regex("(a{10}){10}").num_states == 101
    assert compile_regex("([a-z0-9 ]{89}){23}").num_states == 2048


def test_the_state_cap_raises():
    compile_regex("[ab]*a[ab]{6}", max_states=200)          # 2^7 = 128 subsets
    with pytest.raises(ValueError, match="more than 100 states") as info:
        compile_regex("[ab]*a[ab]{6}", max_states=100)
    assert not isinstance(info.value, GuideSyntaxError)
    with pytest.raises(ValueError, match="more than 4 states"):
        compile_choice(["abcdef"], max_states=4)


CHOICES = [["yes", "no"], ["a", "ab", "abc"], ["maybe", "may", "be"], ["é", "e", "caf.é"], ["a|b", "(c)", "d*"], ["x"]]


@pytest.mark.parametrize("choices", CHOICES, ids=["-".join(c) for c in CHOICES])
def test_choice_agrees_with_the_regex_of_the_escaped_alternation(choices):
    trie = compile_choice(choices)
    check_shape(trie)
    oracle = re.compile("|".join(re.escape(c) for c in choices).encode("utf-8"))
    # (re.escape leaves non-ASCII alone and escapes only ASCII punctuation: inside the supported subset)
    dfa = compile_regex("|".join("(?:" + re.escape(c) + ")" for c in choices))
    alphabet = bytes((sorted(set(b"".join(c.encode() for c in choices))) + list(b"zqw"))[:5])
    for s in list(all_strings(alphabet)) + [c.encode() for c in choices]:
        want = oracle.fullmatch(s) is not None
        assert trie.accepts(s) == want == dfa.accepts(s), (choices, s)
    for c in choices:
        assert trie.accepts(c.encode())
        # a choice that is no prefix of another is complete
        st = trie.walk(0, c.encode())
        assert bool(trie.complete[st]) == (not any(o != c and o.startswith(c) for o in choices))


@pytest.mark.parametrize("bad", [[], [""], ["a", ""], ["a", "a"], ["a", 3]])
def test_choice_refuses_empty_lists_empty_strings_and_duplicates(bad):
    with pytest.raises(ValueError):
        compile_choice(bad)
