"""Timing of the KV-store family (csrc/kvcache.hip, csrc/rotary.hip, csrc/kv_store.h) on the GPU, entry by entry.

    [SWIFTLLM_HIP_LIB=<library>] python tools/kv_store_micro.py [--iters 200] [--out FILE]

Llama-3-8B shape (H 32, KVH 8, D 128, L 32, block 16), float16 and bfloat16, q / k / v as column slices of one fused qkv row:
  prefill  swl_store_kv_prefill[_at], swl_rotary_store_kv_prefill[_at], swl_store_kv_prefill_at_fp8 on one prompt of 4096
           tokens, on 8 x 512, and on a 2048-token chunk behind a 16 000-token context (the `_at` entries; the first two
           workloads run the plain entries and, for FP8, null contexts)
  decode   swl_store_kv_decode, swl_rotary_store_kv_decode, swl_splitk_rotary_store_kv_decode (4 slabs),
           swl_store_kv_decode_fp8 at 1, 32 and 256 sequences
Device events around `--iters` back-to-back launches; µs per launch. Prints one JSON line (and appends it to --out).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from swiftllm_amd import _hip  # noqa: E402

H, KVH, D, L, LAYER, BS = 32, 8, 128, 32, 5, 16
QKV = (H + 2 * KVH) * D
NB, MBPS = 2048, 1152            # pool blocks (1 MiB each per 16-bit pool); block-table row: 18 048 tokens
ROPE_ROWS = 18048
PREFILL = {"1x4096": ([0], [4096]), "8x512": ([0] * 8, [512] * 8), "2048_behind_16000": ([16000], [2048])}
DECODE = (1, 32, 256)
KS = 4


def _timed(fn, iters):
    for _ in range(10):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1) * 1000.0 / iters, 3)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def _tables(g, totals):
    """A block table whose row i holds distinct random blocks for `totals[i]` tokens; sequence ids 0..n-1."""
    need = [-(-t // BS) for t in totals]
    assert sum(need) <= NB and max(need) <= MBPS
    perm = torch.randperm(NB, generator=g).to(torch.int32)
    bt = torch.zeros(len(totals), MBPS, dtype=torch.int32)
    off = 0
    for i, n in enumerate(need):
        bt[i, :n] = perm[off:off + n]
        off += n
    return bt.cuda(), _i32(list(range(len(totals))))


def run(iters):
    P = _hip.ptr
    g = torch.Generator().manual_seed(0)
    res = {"lib": os.path.basename(_hip.library_path())}
    for dtype in (torch.float16, torch.bfloat16):
        name = "f16" if dtype == torch.float16 else "bf16"
        code, stream = _hip.dtype_code(dtype), _hip.stream()
        kc = vc = kc8 = vc8 = None      # (the other dtype's pools go before these come)
        kc, vc = (torch.zeros(NB, L, KVH, BS, D, dtype=dtype, device="cuda") for _ in range(2))
        kc8, vc8 = (torch.zeros(NB, L, KVH, BS, D, dtype=torch.uint8, device="cuda") for _ in range(2))
        ang = torch.rand(ROPE_ROWS, D // 2, generator=g) * 6.28
        cos, sin = torch.cos(ang).to(dtype).cuda(), torch.sin(ang).to(dtype).cuda()
        inv = (0.5 + torch.rand(2, L, KVH, generator=g)).cuda()

        for label, (ctxs, lens) in PREFILL.items():
            T, n, at = sum(lens), len(lens), any(ctxs)
            qkv = torch.randn(T, QKV, generator=g).to(dtype).cuda()
            q, k, v = qkv[:, :H * D], qkv[:, H * D:(H + KVH) * D], qkv[:, (H + KVH) * D:]
            bt, ids = _tables(g, [c + m for c, m in zip(ctxs, lens)])
            lens_d, starts = _i32(lens), _i32([sum(lens[:i]) for i in range(n)])
            ctx = (_i32(ctxs),) if at else ()
            pos = _i32([c + t for c, m in zip(ctxs, lens) for t in range(m)])
            tables = (P(bt), P(ids), P(starts), P(lens_d))
            geom = (LAYER, L, KVH, BS, D, MBPS)
            sfx = "_at" if at else ""
            res[f"{name}_prefill_{label}_store_us"] = _timed(lambda: _hip.call(
                "swl_store_kv_prefill" + sfx, P(kc), P(vc), P(k), P(v), *tables, *map(P, ctx), n, max(lens), *geom, QKV, QKV,
                code, stream), iters)
            res[f"{name}_prefill_{label}_rotary_store_us"] = _timed(lambda: _hip.call(
                "swl_rotary_store_kv_prefill" + sfx, P(q), P(k), P(v), P(cos), P(sin), P(pos), P(kc), P(vc), *tables,
                *map(P, ctx), n, max(lens), LAYER, L, H, KVH, BS, D, MBPS, QKV, QKV, QKV, code, stream), iters)
            res[f"{name}_prefill_{label}_store_fp8_us"] = _timed(lambda: _hip.call(
                "swl_store_kv_prefill_at_fp8", P(kc8), P(vc8), P(k), P(v), P(inv), *tables, P(ctx[0]) if at else 0, n,
                max(lens), *geom, QKV, QKV, code, stream), iters)

        for bd in DECODE:
            lens = torch.randint(1, 112, (bd,), generator=g).tolist()
            qkv = torch.randn(bd, QKV, generator=g).to(dtype).cuda()
            q, k, v = qkv[:, :H * D], qkv[:, H * D:(H + KVH) * D], qkv[:, (H + KVH) * D:]
            slabs = (torch.randn(KS, bd, QKV, generator=g) * 0.5).cuda()
            bt, ids = _tables(g, lens)
            lens_d = _i32(lens)
            pos = lens_d - 1
            tables = (P(bt), P(ids), P(lens_d), bd)
            res[f"{name}_decode_{bd}_store_us"] = _timed(lambda: _hip.call(
                "swl_store_kv_decode", P(kc), P(vc), P(k), P(v), *tables, LAYER, L, KVH, BS, D, MBPS, QKV, QKV, code, stream),
                iters)
            res[f"{name}_decode_{bd}_rotary_store_us"] = _timed(lambda: _hip.call(
                "swl_rotary_store_kv_decode", P(q), P(k), P(v), P(cos), P(sin), P(pos), P(kc), P(vc), *tables, H, KVH, D,
                LAYER, L, BS, MBPS, QKV, QKV, QKV, code, stream), iters)
            res[f"{name}_decode_{bd}_splitk_rotary_store_us"] = _timed(lambda: _hip.call(
                "swl_splitk_rotary_store_kv_decode", P(q), P(k), P(v), P(slabs), KS, P(cos), P(sin), P(pos), P(kc), P(vc),
                *tables, H, KVH, D, LAYER, L, BS, MBPS, QKV, QKV, QKV, code, stream), iters)
            res[f"{name}_decode_{bd}_store_fp8_us"] = _timed(lambda: _hip.call(
                "swl_store_kv_decode_fp8", P(kc8), P(vc8), P(k), P(v), P(inv), *tables, LAYER, L, KVH, BS, D, MBPS, QKV, QKV,
                code, stream), iters)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    line = json.dumps(run(a.iters))
    print(line)
    if a.out:
        with open(a.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
