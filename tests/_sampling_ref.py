"""numpy reference of the sampling contract (swiftllm_amd/csrc/sampling.hip): Philox4x32-10, the top-k / top-p sets
with ties kept, and the Gumbel-max draw. Test helper only: the product never imports it."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: uint [..., 4], key: uint [..., 2] (broadcast) -> uint32 [..., 4]. uint64 arithmetic throughout."""
    c = [np.asarray(counter, dtype=np.uint64)[..., j] for j in range(4)]
    k0 = np.asarray(key, dtype=np.uint64)[..., 0].copy()
    k1 = np.asarray(key, dtype=np.uint64)[..., 1].copy()
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _MASK, p1 & _MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _MASK,
             p0 & _MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(seed: int, pos: int, n: int) -> np.ndarray:
    """u_i for i < n: (word >> 9) * 2^-23 + 2^-24, word = word i & 3 of Philox(counter (i >> 2, pos, 0, 0))."""
    groups = (n + 3) // 4
    ctr = np.zeros((groups, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(groups)
    ctr[:, 1] = pos
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    words = philox4x32_10(ctr, key).reshape(-1)[:n]
    return (words >> 9).astype(np.float64) * 2.0 ** -23 + 2.0 ** -24


def kept_set(f: np.ndarray, temperature: float, top_k: int = 0, top_p: float = 1.0, p_shift: float = 0.0):
    """Boolean mask of the kept elements of one row (f: float64 values of the stored logits), fp64 weights."""
    n = f.size
    ok = ~np.isnan(f)
    m = f[ok].max()
    keep = ok.copy()
    if 1 <= top_k < n:
        vals = np.sort(f[ok])[::-1]
        if top_k <= vals.size:
            keep &= f >= vals[top_k - 1]
    p = top_p + p_shift
    if 0.0 < top_p < 1.0:
        w = np.where(keep, np.exp((np.where(ok, f, -np.inf) - m) / temperature), 0.0)
        total = w.sum()
        idx = np.flatnonzero(keep)
        order = idx[np.argsort(-f[idx], kind="stable")]
        fs, cs = f[order], np.cumsum(w[order])
        ends = np.flatnonzero(np.append(fs[1:] != fs[:-1], True))      # last position of every distinct value
        j = int(np.argmax(cs[ends] >= p * total))                      # the largest value whose mass reaches p
        keep &= f >= fs[ends[j]]
    return keep


def scores(f: np.ndarray, temperature: float, seed: int, pos: int) -> np.ndarray:
    """s_i + G_i for every element (fp64; NaN elements -inf)."""
    ok = ~np.isnan(f)
    m = f[ok].max()
    s = (np.where(ok, f, -np.inf) - m) / temperature
    u = uniforms(seed, pos, f.size)
    return s - np.log(-np.log(u))


def sample_row(f, temperature, top_k, top_p, seed, pos):
    """The token of one row (greedy when temperature == 0) and the margin between its score and the runner-up's."""
    f = np.asarray(f, dtype=np.float64)
    if temperature == 0 or np.all(np.isnan(f) | (f == -np.inf)):
        g = np.where(np.isnan(f), -np.inf, f)
        return (int(np.argmax(g)) if np.any(g > -np.inf) else 0), np.inf
    keep = kept_set(f, temperature, top_k, top_p)
    sc = np.where(keep, scores(f, temperature, seed, pos), -np.inf)
    tok = int(np.argmax(sc))
    second = np.max(np.delete(sc, tok)) if sc.size > 1 else -np.inf
    return tok, sc[tok] - second


def filtered_softmax(f, temperature, top_k, top_p):
    f = np.asarray(f, dtype=np.float64)
    keep = kept_set(f, temperature, top_k, top_p)
    m = f[keep].max()
    w = np.where(keep, np.exp((f - m) / temperature), 0.0)
    return w / w.sum()
