"""Guided decoding, host side: pattern -> byte DFA (regex.py), the bytes each token spells (vocab.py), and the bookkeeping
of the device mask pool with the cursor a request walks through its guide (store.py). Pure Python + numpy: importing it
needs no GPU. The kernels that build and apply the masks are csrc/guided.hip (worker/kernels/guided.py)."""
from .regex import DEFAULT_MAX_STATES, Dfa, GuideSyntaxError, compile_choice, compile_regex
from .vocab import TokenVocab
from .store import Guide, GuideCursor, GuideStore, GuideStoreFull, GuideViolation, guide_key, words_per_row

__all__ = ["DEFAULT_MAX_STATES", "Dfa", "GuideSyntaxError", "compile_choice", "compile_regex", "TokenVocab", "Guide",
           "GuideCursor", "GuideStore", "GuideStoreFull", "GuideViolation", "guide_key", "words_per_row"]
