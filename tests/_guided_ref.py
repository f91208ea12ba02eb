"""The reference of the guided-decoding tests: the mask contract of csrc/guided.hip as a plain Python double loop, and the
mask application with torch.where. Also the small synthetic vocabularies the tests share."""
import numpy as np
import torch

from swiftllm_amd.guided import TokenVocab


def ref_masks(dfa, vocab, end_ids, words=None) -> np.ndarray:
    """uint32 [S, W]: bit (t & 31) of word (t >> 5) of row s is set when token t may be picked in state s. `dfa` None: an
    error; `vocab`: a TokenVocab."""
    tokens = vocab.tokens
    v = len(tokens)
    words = (v + 31) // 32 if words is None else words
    s_count = dfa.trans.shape[0]
    out = np.zeros((s_count, words), dtype=np.uint32)
    ends = set(int(t) for t in end_ids)
    trans = dfa.trans.tolist()
    for s in range(s_count):
        for t in range(v):
            if t in ends:
                ok = bool(dfa.accepting[s])
            else:
                data = tokens[t]
                ok = bool(data)
                st = s
                for b in data or b"":
                    st = trans[st][b]
                    if st < 0:
                        ok = False
                        break
            if ok:
                out[s, t >> 5] |= np.uint32(1 << (t & 31))
    return out


def allowed_ids(mask_row: np.ndarray, n: int) -> list:
    """The token ids < n whose bit is set in one uint32 / int32 mask row."""
    bits = np.unpackbits(np.ascontiguousarray(mask_row).view(np.uint8), bitorder="little")[:n]
    return np.flatnonzero(bits).tolist()


def ref_apply(logits: torch.Tensor, mask_rows, row_index) -> torch.Tensor:
    """A copy of [rows, n] logits in which row r, with k = row_index[r] inside [0, len(mask_rows)), keeps the elements whose
    bit in mask row k is set and holds -inf elsewhere; any other row is unchanged."""
    out = logits.clone()
    n = logits.shape[1]
    masks = np.ascontiguousarray(np.asarray(mask_rows)).view(np.uint32).reshape(len(mask_rows), -1)
    for r, k in enumerate(row_index):
        k = int(k)
        if k < 0 or k >= masks.shape[0]:
            continue
        bits = np.unpackbits(masks[k].view(np.uint8), bitorder="little")[:n].astype(bool)
        keep = torch.from_numpy(bits).to(logits.device)
        out[r] = torch.where(keep, logits[r], torch.full_like(logits[r], float("-inf")))
    return out


def bits_of(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def synthetic_vocab(size: int, seed: int = 0, end_ids=(), alphabet: bytes = None) -> TokenVocab:
    """All 256 single bytes first, then tokens of 2..24 bytes (drawn from `alphabet`, default: printable ASCII heavy on
    digits and the letters the test patterns use), tokens that split the UTF-8 characters 'é' / '€' / '😀', and every 37th id
    empty (None). The ids in `end_ids` are None too (special tokens spell nothing)."""
    rng = np.random.default_rng(seed)
    alphabet = alphabet or b"0123456789abcdefyesnomaybe-:., \"{}[]xyzTZ"
    tokens = [bytes([b]) for b in range(256)]
    utf = ["é".encode(), "€".encode(), "😀".encode()]
    split = []
    for u in utf:
        for cut in range(1, len(u)):
            split += [b"a" + u[:cut], u[cut:] + b"b", u[:cut], u[cut:]]
    split += [u for u in utf] + [b"caf" + utf[0], utf[1] + b"5"]
    i = 0
    while len(tokens) < size:
        t = len(tokens)
        if t % 37 == 0:
            tokens.append(None)
        elif t % 5 == 0 and i < len(split):
            tokens.append(split[i])
            i += 1
        else:
            n = int(rng.integers(2, 25)) if t % 3 == 0 else int(rng.integers(2, 5))
            tokens.append(bytes(alphabet[j] for j in rng.integers(0, len(alphabet), n)))
    tokens = tokens[:size]
    for e in end_ids:
        tokens[e] = None
    return TokenVocab(tokens)
