"""The contract of csrc/logits_adjust.hip in torch on the CPU, in fp32, one IEEE operation per step in the kernel's order:
the GPU tests hold the kernel to it bit for bit."""
import math

import torch

COUNT_MASK = 0x7fffffff


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def adjust_ref(x, offsets, ids, meta, bias, row_params):
    """x: [rows, n] fp16/bf16 CPU tensor; offsets int32 [rows + 1]; ids / meta int32 [E]; bias float32 [E]; row_params
    float32 [rows, 4]. Returns the adjusted copy of x."""
    out = x.clone()
    rows, n = x.shape
    for r in range(rows):
        rep, pres, freq, gap = (row_params[r, k].clone() for k in range(4))
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        if hi > lo:
            i, mt, b = ids[lo:hi].long(), meta[lo:hi], bias[lo:hi]
            ok = (i >= 0) & (i < n)
            i, mt, b = i[ok], mt[ok], b[ok]
            count = mt & COUNT_MASK
            f = out[r, i].float()
            if float(rep) != 1.0:
                f = torch.where((count > 0) | (mt < 0), torch.where(f > 0, f / rep, f * rep), f)
            f = f - freq * count.to(torch.float32)
            f = torch.where(count > 0, f - pres, f)
            f = f + b
            out[r, i] = f.to(x.dtype)
        if float(gap) > -math.inf:
            row = out[r].float()
            valid = ~torch.isnan(row)
            if bool(valid.any()):
                m = row[valid].max()
                out[r, (row - m) < gap] = -math.inf
    return out


def same_bits(a, b):
    """Bit equality of two 16-bit float tensors, except that any NaN equals any NaN."""
    ai, bi = a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)
    return bool(((ai == bi) | (torch.isnan(a) & torch.isnan(b))).all())


def min_p_gap(temperature, min_p):
    """fp32(T * ln(min_p)) computed in double precision; -inf when min-p is off."""
    if min_p <= 0 or temperature <= 0:
        return -math.inf
    return float(f32(temperature * math.log(min_p)))


def history_entries(prompt, outputs):
    """(ids, meta) of a sequence from scratch: first-seen order, the words the kernel reads."""
    from collections import Counter
    seen_p, cnt = set(prompt), Counter(outputs)
    order = list(dict.fromkeys(list(prompt) + list(outputs)))
    ids = torch.tensor(order, dtype=torch.int32)
    meta = torch.tensor([(cnt[t] | (-2 ** 31 if t in seen_p else 0)) for t in order], dtype=torch.int64).to(torch.int32)
    return ids, meta
