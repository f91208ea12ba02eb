"""Where the kernels read and write: every entry point of tests/_contract.py run through the arena harness
(tests/_arena.py) — operands at their minimum legal alignment, strides padded by the smallest legal amount, scratch /
workspace / slab buffers at exactly their advertised size and pre-filled with 0xFF. Per case: a control on plain tensors,
a 0xFF arena and a 0x00 arena; outputs bit-identical across the three, no byte outside the declared outputs changed.
What the kernels compute is checked elsewhere (test_gpu_kernels.py, test_gpu_rows.py, ...); here only that it does not
depend on, or spill into, the surroundings. See tests/_arena.py for what this method cannot see.

Calls are made by field name through the rows of tests/_contract.py, so an argument cannot land in the wrong slot.
Unused block-table entries name a spare pool block that no sequence owns (never -1: the control runs on plain tensors);
the spare block must come back unchanged."""
import math

import pytest
import torch

import _contract as C
from _arena import MIN_MARGIN, Op, run_case
from swiftllm_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DEV = "cuda"
F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, *shape, dtype=F32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def i32(x):
    return torch.tensor(x, dtype=I32)


def kcall(name, **kw):
    """Call `name` with its arguments given by field name (tests/_contract.py); tensors become device pointers."""
    fields = [f for f in C.ROWS[name].args if f != "stream"]
    assert set(kw) == set(fields), (name, set(kw) ^ set(fields))
    vals = []
    for f in fields:
        a = kw[f]
        if isinstance(a, torch.dtype):
            a = _hip.dtype_code(a)
        elif isinstance(a, torch.Tensor):
            assert a.is_cuda
            a = a.data_ptr()
        elif a is None:
            a = 0
        vals.append(a)
    _hip.call(name, *vals, _hip.stream())


def run(ops, call, margin=MIN_MARGIN, finite=()):
    want = run_case(ops, call, DEV, margin, sync=torch.cuda.synchronize)
    assert want, "a case declares at least one output"
    for name in finite:
        t = want[name].float()
        assert torch.isfinite(t).all() and t.abs().max() > 0, f"{name}: the control's output is not a usable result"
    return want


def pad8(t):
    return t[0].numel() + 8


# ---- element-wise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden", [8, 136, 4096])
def test_rmsnorm_family(hidden, dtype):
    g, T, ks = gen(hidden), 3, 2
    x, res, w = rnd(g, T, hidden, dtype=dtype), rnd(g, T, hidden, dtype=dtype), rnd(g, hidden, dtype=dtype)
    slabs = rnd(g, ks, T, hidden)
    run({"x": Op(x, out=True), "w": Op(w)},
        lambda v: kcall("swl_rmsnorm", x=v["x"], w=v["w"], eps=1e-5, num_tokens=T, hidden=hidden, dtype=dtype), finite=["x"])
    run({"x": Op(x, out=True), "residual": Op(res, out=True), "w": Op(w)},
        lambda v: kcall("swl_fused_add_rmsnorm", x=v["x"], residual=v["residual"], w=v["w"], eps=1e-5, num_tokens=T,
                        hidden=hidden, dtype=dtype), finite=["x", "residual"])
    run({"x_out": Op(torch.zeros_like(x), out=True), "residual": Op(res, out=True), "w": Op(w), "slabs": Op(slabs)},
        lambda v: kcall("swl_splitk_fused_add_rmsnorm", x_out=v["x_out"], residual=v["residual"], w=v["w"], eps=1e-5,
                        slabs=v["slabs"], k_splits=ks, num_tokens=T, hidden=hidden, dtype=dtype), finite=["x_out", "residual"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_splitk_add_scale(dtype):
    g, T, ks, hidden = gen(7), 3, 2, 1024      # the smallest multiple of its 1024-column chunk
    res, w, slabs = rnd(g, T, hidden, dtype=dtype), rnd(g, hidden, dtype=dtype), rnd(g, ks, T, hidden)
    run({"x_scaled": Op(torch.zeros_like(res), out=True), "residual": Op(res, out=True), "w": Op(w), "slabs": Op(slabs),
         "ssq_out": Op(torch.zeros(hidden // 1024, T), skew=4, out=True)},
        lambda v: kcall("swl_splitk_add_scale", x_scaled=v["x_scaled"], residual=v["residual"], w=v["w"], slabs=v["slabs"],
                        k_splits=ks, ssq_out=v["ssq_out"], num_tokens=T, hidden=hidden, dtype=dtype),
        finite=["x_scaled", "residual", "ssq_out"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inter", [8, 264])
def test_silu_mul(inter, dtype):
    x = rnd(gen(inter), 3, 2 * inter, dtype=dtype)
    run({"x": Op(x, out=True)},
        lambda v: kcall("swl_silu_mul", x=v["x"], num_tokens=3, ffn_inter_dim=inter, dtype=dtype), finite=["x"])


TABLE_ROWS = 128


def rope_tables(g, D, dtype):
    ang = torch.rand(TABLE_ROWS, D // 2, generator=g) * 6.28
    return ang.cos().to(dtype), ang.sin().to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_rotary(D, with_pos, dtype):
    """q and k are column slices of one qkv row of pitch (H + 2 KVH) D + 8; the v columns and the padding stay as they were."""
    g, T, H, KVH = gen(D), 5, 4, 2
    width = (H + 2 * KVH) * D
    qkv = rnd(g, T, width, dtype=dtype)
    cos, sin = rope_tables(g, D, dtype)
    ops = {"qkv": Op(qkv, stride=width + 8, out=True), "cos": Op(cos), "sin": Op(sin)}
    if with_pos:
        ops["pos"] = Op(i32([7, 0, 3, 3, 127]), skew=4)
    run(ops, lambda v: kcall("swl_rotary", q=v["qkv"], k=v["qkv"][:, H * D:], cos_table=v["cos"], sin_table=v["sin"],
                             pos_idx=v.get("pos"), num_tokens=T, num_q_heads=H, num_kv_heads=KVH, head_dim=D,
                             q_tok_stride=width + 8, k_tok_stride=width + 8, dtype=dtype), finite=["qkv"])


# ---- paged state ------------------------------------------------------------------------------------------------------------------
class Paged:
    """A block table for sequences of `totals` tokens: shuffled blocks, table rows picked by seq_ids, unused entries -> spare."""

    def __init__(self, g, totals, L, KVH, D, mbps, fp8=False, dtype=torch.float16):
        self.L, self.KVH, self.D, self.mbps = L, KVH, D, mbps
        need = [-(-t // 16) for t in totals]
        assert max(need) <= mbps
        self.nb = sum(need) + 2
        self.spare = self.nb - 1
        order = torch.randperm(self.nb - 1, generator=g).tolist()
        rows = len(totals) + 2
        self.seq_ids = torch.randperm(rows, generator=g)[:len(totals)].to(I32)
        bt = torch.full((rows, mbps), self.spare, dtype=I32)
        for s, n in enumerate(need):
            for j in range(n):
                bt[self.seq_ids[s], j] = order.pop()
        self.block_table = bt
        shape = (self.nb, L, KVH, 16, D)
        if fp8:
            self.k = rnd(g, *shape).to(torch.float8_e4m3fn).view(U8)
            self.v = rnd(g, *shape).to(torch.float8_e4m3fn).view(U8)
        else:
            self.k, self.v = rnd(g, *shape, dtype=dtype), rnd(g, *shape, dtype=dtype)
        self.block_bytes = L * KVH * 16 * D * self.k.element_size()
        self.margin = max(MIN_MARGIN, 2 * self.block_bytes)

    def ops(self, out):
        return {"k_cache": Op(self.k, out=out), "v_cache": Op(self.v, out=out), "block_table": Op(self.block_table, skew=4),
                "seq_ids": Op(self.seq_ids, skew=4)}

    def spare_untouched(self, want):
        for name, pool in (("k_cache", self.k), ("v_cache", self.v)):
            assert torch.equal(want[name][self.spare].view(U8), pool[self.spare].view(U8)), f"{name}: the spare block changed"


# ---- KV stores --------------------------------------------------------------------------------------------------------------------
STORE_LENS = [1, 16, 17, 33]
STORE_CTX = [3, 0, 5, 20]          # the first chunk starts and ends inside a block
STORE_ENTRIES = ["swl_store_kv_prefill", "swl_store_kv_prefill_at", "swl_store_kv_decode", "swl_rotary_store_kv_prefill",
                 "swl_rotary_store_kv_prefill_at", "swl_rotary_store_kv_decode", "swl_splitk_rotary_store_kv_decode",
                 "swl_store_kv_prefill_at_fp8", "swl_store_kv_decode_fp8"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", STORE_ENTRIES)
def test_kv_store(entry, dtype):
    g = gen(len(entry))
    L, layer, H, KVH, D, mbps, ks = 2, 1, 4, 2, 64, 4, 2
    fp8, rotary, decode, at = entry.endswith("fp8"), "rotary" in entry, "decode" in entry, "_at" in entry
    ctx = STORE_CTX if at else [0] * 4
    totals = STORE_LENS if decode else [c + n for c, n in zip(ctx, STORE_LENS)]
    pg = Paged(g, totals, L, KVH, D, mbps, fp8=fp8, dtype=dtype)
    P = len(STORE_LENS) if decode else sum(STORE_LENS)
    starts = [sum(STORE_LENS[:i]) for i in range(4)]
    k, v, q = rnd(g, P, KVH * D, dtype=dtype), rnd(g, P, KVH * D, dtype=dtype), rnd(g, P, H * D, dtype=dtype)
    ops = pg.ops(out=True)
    ops["seq_lens"] = Op(i32(STORE_LENS), skew=4)
    if not decode:
        ops["start_locs"] = Op(i32(starts), skew=4)
    if at:
        ops["ctx_lens"] = Op(i32(ctx), skew=4)
    if fp8:
        ops["inv_scales"] = Op(torch.rand(2, L, KVH, generator=g) + 0.5, skew=4)
    slabbed = entry == "swl_splitk_rotary_store_kv_decode"
    if slabbed:
        ops["slabs"] = Op(rnd(g, ks, P, (H + 2 * KVH) * D))
        k, v, q = torch.zeros_like(k), torch.zeros_like(v), torch.zeros_like(q)
    ops["k"] = Op(k, stride=pad8(k), out=rotary)
    ops["v"] = Op(v, stride=pad8(v), out=slabbed)
    if rotary:
        ops["q"] = Op(q, stride=pad8(q), out=True)
        ops["cos"], ops["sin"] = (Op(t) for t in rope_tables(g, D, dtype))
        ops["pos"] = Op(i32([n - 1 for n in STORE_LENS]) if decode else torch.randint(0, TABLE_ROWS, (P,), generator=g).to(I32),
                        skew=4)
    common = dict(cur_layer=layer, num_layers=L, num_kv_heads=KVH, block_size=16, head_dim=D, max_blocks_per_seq=mbps,
                  k_tok_stride=pad8(k), v_tok_stride=pad8(v), dtype=dtype)

    def call(t):
        kw = dict(common, k_cache=t["k_cache"], v_cache=t["v_cache"], block_table=t["block_table"], seq_ids=t["seq_ids"],
                  seq_lens=t["seq_lens"])
        if decode:
            kw["num_decoding_seqs"] = 4
        else:
            kw.update(start_locs=t["start_locs"], num_prefill_seqs=4, max_prefill_len=max(STORE_LENS))
        if at:
            kw["ctx_lens"] = t["ctx_lens"]
        if fp8:
            kw["inv_scales"] = t["inv_scales"]
        if rotary:
            kw.update(cos_table=t["cos"], sin_table=t["sin"], pos_idx=t["pos"], num_q_heads=H, q_tok_stride=pad8(q))
        if slabbed:
            kw.update(q_out=t["q"], k_out=t["k"], v_out=t["v"], qkv_slabs=t["slabs"], k_splits=ks)
        else:
            kw.update(k=t["k"], v=t["v"])
            if rotary:
                kw["q"] = t["q"]
        kcall(entry, **kw)

    want = run(ops, call, margin=pg.margin, finite=["q", "k"] if rotary else [])
    pg.spare_untouched(want)
    assert not torch.equal(want["k_cache"].view(U8), pg.k.view(U8)) and not torch.equal(want["v_cache"].view(U8), pg.v.view(U8))


# ---- paged decode attention -----------------------------------------------------------------------------------------------------
DECODE_LENS = [1, 16, 17, 100]
DECODE_ENTRIES = ["swl_paged_attn_decode", "swl_paged_attn_phase1", "swl_paged_attn_phase2", "swl_paged_attn_decode_qkv",
                  "swl_paged_attn_decode_qkv_rs", "swl_paged_attn_decode_qkv_rs_partials", "swl_paged_attn_decode_fp8",
                  "swl_paged_attn_phase1_fp8"]


def scratch_floats(bd, H, D, nsb):
    nbytes = _hip.scratch_bytes(bd, H, D, nsb)
    assert nbytes == bd * H * nsb * (D + 1) * 4
    return nbytes // 4


# (phase 2 only runs on split sequences: seq_block_size 64)
DECODE_CASES = [(e, h, kvh, d, sbs) for e in DECODE_ENTRIES for h, kvh, d in [(8, 8, 32), (8, 2, 64), (8, 1, 128)]
                for sbs in (64, 1024) if not (e == "swl_paged_attn_phase2" and sbs == 1024)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry,H,KVH,D,sbs", DECODE_CASES)
def test_paged_decode(entry, H, KVH, D, sbs, dtype):
    g = gen(H + KVH + D + sbs)
    L, layer, mbps, bd, ks, parts = 2, 1, 8, 4, 2, 2
    nsb = -(-max(DECODE_LENS) // sbs)
    fp8, qkv, rs = entry.endswith("fp8"), "qkv" in entry, "_rs" in entry
    pg = Paged(g, DECODE_LENS, L, KVH, D, mbps, fp8=fp8, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ops = pg.ops(out=qkv)
    ops["seq_lens"] = Op(i32(DECODE_LENS), skew=4)
    o = torch.zeros(bd, H * D, dtype=dtype)
    nfl = scratch_floats(bd, H, D, nsb)
    geom = dict(num_decoding_seqs=bd, num_q_heads=H, head_dim=D, seq_block_size=sbs, num_seq_blocks=nsb, dtype=dtype)
    full = dict(geom, softmax_scale=scale, num_kv_heads=KVH, num_layers=L, block_size=16, cur_layer=layer, max_blocks_per_seq=mbps)

    def pools(t):
        return dict(k_cache=t["k_cache"], v_cache=t["v_cache"], block_table=t["block_table"], seq_ids=t["seq_ids"],
                    seq_lens=t["seq_lens"])

    if entry == "swl_paged_attn_phase2":
        assert nsb > 1
        # partials as phase 1 leaves them: slots of splits past a sequence are never written and must not be read (NaN)
        mid_o, mid_lse = rnd(g, bd, H, nsb, D), rnd(g, bd, H, nsb)
        for s, n in enumerate(DECODE_LENS):
            used = -(-n // sbs)
            mid_o[s, :, used:], mid_lse[s, :, used:] = float("nan"), float("nan")
        ops = {"o": Op(o, stride=H * D + 8, out=True), "mid_o": Op(mid_o, skew=4), "mid_lse": Op(mid_lse, skew=4),
               "seq_lens": ops["seq_lens"]}
        run(ops, lambda t: kcall(entry, o=t["o"], mid_o=t["mid_o"], mid_lse=t["mid_lse"], seq_lens=t["seq_lens"],
                                 o_tok_stride=H * D + 8, **geom), finite=["o"])
        return

    partials_out = entry == "swl_paged_attn_decode_qkv_rs_partials" and nsb > 1
    if "phase1" in entry:
        if nsb > 1:
            ops["mid_o"] = Op(torch.zeros(bd, H, nsb, D), skew=4, out=True)
            ops["mid_lse"] = Op(torch.zeros(bd, H, nsb), skew=4, out=True)
        else:
            ops["o"] = Op(o, stride=H * D + 8, out=True)
    else:
        if not partials_out:
            ops["o"] = Op(o, stride=H * D + 8, out=True)
        if nsb > 1:     # exactly the advertised size; the partials entry leaves its result there
            ops["scratch"] = Op(torch.zeros(nfl), out=True) if partials_out else Op(torch.zeros(nfl), scratch=True)
    if fp8:
        ops["kv_scales"] = Op(torch.rand(2, L, KVH, generator=g) + 0.5, skew=4)
    if qkv:
        ops["slabs"] = Op(rnd(g, ks, bd, (H + 2 * KVH) * D, scale=0.5))
        ops["cos"], ops["sin"] = (Op(t) for t in rope_tables(g, D, dtype))
        ops["pos"] = Op(i32([n - 1 for n in DECODE_LENS]), skew=4)
        if rs:
            ops["row_ssq"] = Op(torch.rand(parts, bd, generator=g) * 500 + 100, skew=4)
    else:
        q = rnd(g, bd, H * D, dtype=dtype)
        ops["q"] = Op(q, stride=pad8(q))

    def call(t):
        kw = dict(full, **pools(t))
        if qkv:
            kw.update(o=t.get("o"), qkv_slabs=t["slabs"], k_splits=ks, cos_table=t["cos"], sin_table=t["sin"], pos_idx=t["pos"],
                      scratch=t.get("scratch"), o_tok_stride=H * D + 8)
            if rs:
                kw.update(row_ssq=t["row_ssq"], ssq_parts=parts, hidden=1024, eps=1e-5)
        else:
            kw.update(q=t["q"], q_tok_stride=H * D + 8, o_tok_stride=H * D + 8)
            if fp8:
                kw["kv_scales"] = t["kv_scales"]
            if "phase1" in entry:
                kw.update(o_direct=t.get("o"), mid_o=t.get("mid_o"), mid_lse=t.get("mid_lse"))
            else:
                kw.update(o=t["o"], scratch=t.get("scratch"))
        kcall(entry, **kw)

    want = run(ops, call, margin=pg.margin, finite=[n for n in ("o", "mid_o") if n in ops and ops[n].out])
    if qkv:
        pg.spare_untouched(want)


# ---- prefill attention ------------------------------------------------------------------------------------------------------------
PREFILL_LENS, PREFILL_CTX = [1, 33, 70], [0, 5, 40]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 64, 128])
def test_prefill_varlen(D, dtype):
    g, H, KVH = gen(D), 4, 2
    P = sum(PREFILL_LENS)
    q, k, v = rnd(g, P, H * D, dtype=dtype), rnd(g, P, KVH * D, dtype=dtype), rnd(g, P, KVH * D, dtype=dtype)
    cu = i32([0] + [sum(PREFILL_LENS[:i + 1]) for i in range(3)])
    ops = {"o": Op(torch.zeros_like(q), stride=pad8(q), out=True), "q": Op(q, stride=pad8(q)), "k": Op(k, stride=pad8(k)),
           "v": Op(v, stride=pad8(v)), "cu": Op(cu, skew=4)}
    run(ops, lambda t: kcall("swl_prefill_attn_varlen", o=t["o"], q=t["q"], k=t["k"], v=t["v"], cu_seqlens=t["cu"],
                             num_prefill_seqs=3, max_prefill_len=max(PREFILL_LENS), num_q_heads=H, num_kv_heads=KVH, head_dim=D,
                             softmax_scale=1.0 / math.sqrt(D), q_tok_stride=pad8(q), k_tok_stride=pad8(k), v_tok_stride=pad8(v),
                             o_tok_stride=pad8(q), dtype=dtype), finite=["o"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("entry", ["swl_prefill_attn_paged", "swl_prefill_attn_paged_fp8"])
def test_prefill_paged(entry, D, dtype):
    g, H, KVH, L, layer, mbps = gen(D + 1), 4, 2, 2, 1, 8
    fp8 = entry.endswith("fp8")
    totals = [c + n for c, n in zip(PREFILL_CTX, PREFILL_LENS)]
    pg = Paged(g, totals, L, KVH, D, mbps, fp8=fp8, dtype=dtype)
    P = sum(PREFILL_LENS)
    q = rnd(g, P, H * D, dtype=dtype)
    ops = pg.ops(out=False)
    ops.update(o=Op(torch.zeros_like(q), stride=pad8(q), out=True), q=Op(q, stride=pad8(q)),
               cu=Op(i32([0] + [sum(PREFILL_LENS[:i + 1]) for i in range(3)]), skew=4), ctx=Op(i32(PREFILL_CTX), skew=4))
    if fp8:
        ops["kv_scales"] = Op(torch.rand(2, L, KVH, generator=g) + 0.5, skew=4)

    def call(t):
        kw = dict(o=t["o"], q=t["q"], k_cache=t["k_cache"], v_cache=t["v_cache"], block_table=t["block_table"],
                  seq_ids=t["seq_ids"], cu_seqlens=t["cu"], ctx_lens=t["ctx"], num_prefill_seqs=3,
                  max_new_len=max(PREFILL_LENS), max_total_len=max(totals), num_q_heads=H, num_kv_heads=KVH, head_dim=D,
                  num_layers=L, block_size=16, cur_layer=layer, max_blocks_per_seq=mbps, softmax_scale=1.0 / math.sqrt(D),
                  q_tok_stride=pad8(q), o_tok_stride=pad8(q), dtype=dtype)
        if fp8:
            kw["kv_scales"] = t["kv_scales"]
        kcall(entry, **kw)

    run(ops, call, margin=pg.margin, finite=["o"])


# ---- sampling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 1000])
def test_argmax(n, dtype):
    g, rows = gen(n), 3
    x = rnd(g, rows, n, dtype=dtype)
    nbytes = int(_hip.load().swl_argmax_scratch_bytes(rows))
    ops = {"out": Op(torch.full((rows,), -7, dtype=I64), skew=8, out=True), "x": Op(x, stride=n + 8),
           "scratch": Op(torch.zeros(nbytes // 4), scratch=True)}
    want = run(ops, lambda t: kcall("swl_argmax", out=t["out"], x=t["x"], scratch=t["scratch"], scratch_bytes=nbytes,
                                    num_rows=rows, n=n, row_stride=n + 8, dtype=dtype))
    assert torch.equal(want["out"], x.float().argmax(dim=1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 1000, 4097])
def test_sample(n, dtype):
    """x at 2 mod 4 with row_stride = n + 1: the element-wise load path in all three runs (the control has the same stride)."""
    g, rows = gen(n), 3
    x = rnd(g, rows, n, dtype=dtype, scale=3.0)
    ops = {"out": Op(torch.full((rows,), -7, dtype=I64), skew=8, out=True), "x": Op(x, skew=2, stride=n + 1),
           "temperature": Op(torch.tensor([0.0, 0.8, 1.3]), skew=4), "top_k": Op(i32([0, 50, 0]), skew=4),
           "top_p": Op(torch.tensor([1.0, 0.9, 0.5]), skew=4), "seed": Op(i32([[1, 2], [3, 4], [5, 6]]), skew=4),
           "pos": Op(i32([0, 9, 300]), skew=4)}
    want = run(ops, lambda t: kcall("swl_sample", out=t["out"], x=t["x"], num_rows=rows, n=n, row_stride=n + 1, dtype=dtype,
                                    temperature=t["temperature"], top_k=t["top_k"], top_p=t["top_p"], seed=t["seed"],
                                    pos=t["pos"]))
    assert ((want["out"] >= 0) & (want["out"] < n)).all() and want["out"][0] == x[0].float().argmax()


# ---- GEMMs ------------------------------------------------------------------------------------------------------------------------
_packed = {}


def weight(n, k, dtype, packed, seed=0):
    """W[n, k] (CPU), row-major or packed by swl_gemm_pack_weight (run once on plain tensors)."""
    key = (n, k, dtype, seed)
    if key not in _packed:
        w = rnd(gen(n * 7 + k + seed), n, k, dtype=dtype, scale=0.05)
        src, dst = w.to(DEV), torch.zeros(n, k, dtype=dtype, device=DEV)
        kcall("swl_gemm_pack_weight", dst=dst, src=src, N=n, K=k, dtype=dtype)
        torch.cuda.synchronize()
        _packed[key] = (w, dst.cpu())
    return _packed[key][1 if packed else 0]


def legal_splits(k, tile=128, uneven=False):
    out = [s for s in (1, 2, 4, 8, 16) if k % (tile * s) == 0]
    if uneven:
        out += [s for s in (2, 4, 8, 16) if k % (tile * s) and (k // tile) // s >= 8]
    return sorted(out)


SHAPES = [(32, 128), (96, 384), (160, 1280), (64, 1536)]
PACKED_SHAPES = SHAPES + [(256, 11008)]                  # uneven splits
DEEP = (32, 2048)                                        # an addition: the only K here that 8 and 16 split evenly
MS = [1, 5, 32]


def gemm_io(g, m, n, k, dtype):
    x = rnd(g, m, k, dtype=dtype)
    return {"x": Op(x, stride=k + 8), "out": Op(torch.zeros(m, n, dtype=dtype), skew=8, stride=n + 4, out=True)}


def gemm_cases(entries, shapes):
    """(entry, N, K): K = 11008 (uneven splits) for the packed entries only; the _nx entries run the ring kernel only, K / 128 >= 8."""
    return [(e, n, k) for e in entries for n, k in shapes
            if ("packed" in e or k != 11008) and not (e.endswith("_nx") and k < 1024)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("entry,n,k", gemm_cases(["swl_gemm_skinny", "swl_gemm_skinny_packed"], PACKED_SHAPES + [DEEP]))
def test_gemm_skinny(entry, n, k, m, dtype):
    packed = "packed" in entry
    lib = _hip.load()
    for ks in [0] + legal_splits(k, uneven=packed):
        if (n, k) == DEEP and ks not in (8, 16):
            continue
        ops = gemm_io(gen(n + k + m + ks), m, n, k, dtype)
        ops["w"] = Op(weight(n, k, dtype, packed))
        nbytes = int(lib.swl_gemm_skinny_workspace_bytes(m, n, k)) if ks == 0 else (ks * m * n * 4 if ks > 1 else 0)
        if nbytes:
            ops["ws"] = Op(torch.zeros(nbytes // 4), scratch=True)
        run(ops, lambda t: kcall(entry, out=t["out"], x=t["x"], w=t["w"], workspace=t.get("ws"), workspace_bytes=nbytes, M=m,
                                 N=n, K=k, x_row_stride=k + 8, out_row_stride=n + 4, k_splits=ks, dtype=dtype), finite=["out"])


PARTIAL_ENTRIES = ["swl_gemm_skinny_partial", "swl_gemm_skinny_packed_partial", "swl_gemm_skinny_packed_partial_nf",
                   "swl_gemm_skinny_packed_partial_nx"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("entry,n,k", gemm_cases(PARTIAL_ENTRIES, PACKED_SHAPES + [DEEP]))
def test_gemm_partial_and_reduce(entry, n, k, m, dtype):
    """The slab-writing entries at every legal split; swl_splitk_reduce then runs on the control's slabs."""
    packed, nf, nx = "packed" in entry, entry.endswith("_nf"), entry.endswith("_nx")
    for ks in legal_splits(k, uneven=packed and not (nf or nx)):
        if (n, k) == DEEP and ks not in (8, 16):
            continue
        g = gen(n + k + m + ks)
        x = rnd(g, m, k, dtype=dtype)
        ops = {"x": Op(x, stride=k + 8), "w": Op(weight(n, k, dtype, packed)), "slabs": Op(torch.zeros(ks, m, n), out=True)}
        kw = dict(M=m, N=n, K=k, x_row_stride=k + 8, k_splits=ks, dtype=dtype, slabs_bytes=ks * m * n * 4)
        if nf or nx:
            ops["norm_w"] = Op(rnd(g, k, dtype=dtype))
        if nf:
            ops["ssq_out"] = Op(torch.zeros(ks, m), skew=4, out=True)
        if nx:
            ops["ssq_in"] = Op(torch.rand(m, 64, generator=g) * 20 + 1)
        want = run(ops, lambda t: kcall(entry, slabs=t["slabs"], x=t["x"], w=t["w"], **kw,
                                        **({"norm_w": t["norm_w"]} if nf or nx else {}),
                                        **({"ssq_out": t["ssq_out"]} if nf else {}),
                                        **({"ssq_in": t["ssq_in"], "ssq_parts": 64, "eps": 1e-5} if nx else {})),
                   finite=["slabs"])
        if entry == "swl_gemm_skinny_packed_partial":
            run({"slabs": Op(want["slabs"]), "out": Op(torch.zeros(m, n, dtype=dtype), skew=8, stride=n + 4, out=True)},
                lambda t: kcall("swl_splitk_reduce", out=t["out"], slabs=t["slabs"], k_splits=ks, M=m, N=n, out_row_stride=n + 4,
                                dtype=dtype), finite=["out"])


SILU_ENTRIES = ["swl_gemm_skinny_silu_gate", "swl_gemm_skinny_packed_silu_gate", "swl_gemm_skinny_packed_silu_gate_rs",
                "swl_gemm_skinny_packed_silu_gate_nf", "swl_gemm_skinny_packed_silu_gate_nx"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("entry,n,k", gemm_cases(SILU_ENTRIES, PACKED_SHAPES))
def test_gemm_silu_gate(entry, n, k, m, dtype):
    packed = "packed" in entry
    g = gen(n + k + m)
    ops = gemm_io(g, m, n, k, dtype)
    ops["w"] = Op(weight(2 * n, k, dtype, packed, seed=1))
    extra = {}
    if entry.endswith("_rs"):
        ops["row_ssq"] = Op(torch.rand(2, m, generator=g) * k + 1, skew=4)
        extra = lambda t: dict(row_ssq=t["row_ssq"], ssq_parts=2, eps=1e-5)
    elif entry.endswith("_nf"):
        ops["norm_w"] = Op(rnd(g, k, dtype=dtype))
        extra = lambda t: dict(norm_w=t["norm_w"], eps=1e-5)
    elif entry.endswith("_nx"):
        ops["norm_w"] = Op(rnd(g, k, dtype=dtype))
        ops["ssq_in"] = Op(torch.rand(m, 64, generator=g) * 20 + 1)
        extra = lambda t: dict(norm_w=t["norm_w"], eps=1e-5, ssq_in=t["ssq_in"], ssq_parts=64)
    else:
        extra = lambda t: {}
    run(ops, lambda t: kcall(entry, out=t["out"], x=t["x"], w=t["w"], M=m, I=n, K=k, x_row_stride=k + 8, out_row_stride=n + 4,
                             dtype=dtype, **extra(t)), finite=["out"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k", SHAPES)
def test_gemm_pack_weight(n, k, dtype):
    w = weight(n, k, dtype, False)
    want = run({"src": Op(w), "dst": Op(torch.zeros_like(w), out=True)},
               lambda t: kcall("swl_gemm_pack_weight", dst=t["dst"], src=t["src"], N=n, K=k, dtype=dtype))
    assert torch.equal(want["dst"].view(torch.int16), weight(n, k, dtype, True).view(torch.int16))
    assert torch.equal(want["dst"].view(torch.int16).flatten().sort()[0], w.view(torch.int16).flatten().sort()[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [33, 64])
@pytest.mark.parametrize("n,k", [(96, 384), (64, 1536)])
@pytest.mark.parametrize("entry", ["swl_gemm_packed_mid", "swl_gemm_packed_mid_partial", "swl_gemm_packed_mid_silu_gate"])
def test_gemm_mid(entry, n, k, m, dtype):
    lib = _hip.load()
    silu, partial = entry.endswith("silu_gate"), entry.endswith("partial")
    for ks in ([None] if silu else ([] if partial else [0]) + legal_splits(k)):
        g = gen(n + k + m)
        ops = gemm_io(g, m, n, k, dtype)
        ops["w"] = Op(weight(2 * n if silu else n, k, dtype, True, seed=int(silu)))
        if silu:
            call = lambda t: kcall(entry, out=t["out"], x=t["x"], w=t["w"], M=m, I=n, K=k, x_row_stride=k + 8,
                                   out_row_stride=n + 4, dtype=dtype)
        elif partial:
            del ops["out"]
            ops["slabs"] = Op(torch.zeros(ks, m, n), out=True)
            call = lambda t: kcall(entry, slabs=t["slabs"], slabs_bytes=ks * m * n * 4, x=t["x"], w=t["w"], M=m, N=n, K=k,
                                   x_row_stride=k + 8, k_splits=ks, dtype=dtype)
        else:
            chosen = ks or int(lib.swl_gemm_packed_mid_choose_splits(m, n, k))
            nbytes = chosen * m * n * 4 if chosen > 1 else 0
            if nbytes:
                ops["ws"] = Op(torch.zeros(nbytes // 4), scratch=True)
            call = lambda t: kcall(entry, out=t["out"], x=t["x"], w=t["w"], workspace=t.get("ws"), workspace_bytes=nbytes, M=m,
                                   N=n, K=k, x_row_stride=k + 8, out_row_stride=n + 4, k_splits=ks, dtype=dtype)
        run(ops, call, finite=["slabs" if partial else "out"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wpg", [4, 8])
@pytest.mark.parametrize("k", [64, 1024])
@pytest.mark.parametrize("m", [65, 129, 256])
@pytest.mark.parametrize("entry", ["swl_gemm_packed_wide", "swl_gemm_packed_wide_partial", "swl_gemm_packed_wide_silu_gate"])
def test_gemm_wide(entry, m, k, wpg, dtype):
    lib, n = _hip.load(), 96
    silu, partial = entry.endswith("silu_gate"), entry.endswith("partial")
    for ks in ([None] if silu else ([] if partial else [0]) + legal_splits(k, tile=64)[:3]):
        g = gen(k + m + wpg)
        ops = gemm_io(g, m, n, k, dtype)
        ops["w"] = Op(weight(2 * n if silu else n, k, dtype, True, seed=int(silu)))
        if silu:
            call = lambda t: kcall(entry, out=t["out"], x=t["x"], w=t["w"], M=m, I=n, K=k, x_row_stride=k + 8,
                                   out_row_stride=n + 4, waves_per_group=wpg, dtype=dtype)
        elif partial:
            del ops["out"]
            ops["slabs"] = Op(torch.zeros(ks, m, n), out=True)
            call = lambda t: kcall(entry, slabs=t["slabs"], slabs_bytes=ks * m * n * 4, x=t["x"], w=t["w"], M=m, N=n, K=k,
                                   x_row_stride=k + 8, waves_per_group=wpg, k_splits=ks, dtype=dtype)
        else:
            # k_splits = 0 with a forced workgroup width: the plan may differ from the advertised one, so size it for any
            nbytes = (ks * m * n * 4 if ks > 1 else 0) if ks else 16 * m * n * 4
            if ks == 0 and wpg == 4:
                nbytes = int(lib.swl_gemm_packed_wide_workspace_bytes(m, n, k))      # the library's own plan: exactly that
            if nbytes:
                ops["ws"] = Op(torch.zeros(nbytes // 4), scratch=True)
            call = lambda t: kcall(entry, out=t["out"], x=t["x"], w=t["w"], workspace=t.get("ws"), workspace_bytes=nbytes, M=m,
                                   N=n, K=k, x_row_stride=k + 8, out_row_stride=n + 4, waves_per_group=wpg, k_splits=ks,
                                   dtype=dtype)
        run(ops, call, finite=["slabs" if partial else "out"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 16, 17, 32])         # x from fragments (M <= 8) and through LDS (M > 8), one and two token blocks
@pytest.mark.parametrize("n,k", [(32, 5120), (64, 1024), (96, 3072)])
@pytest.mark.parametrize("entry", ["swl_gemm_rows_add", "swl_gemm_rows_add_ssq"])
def test_gemm_rows_add(entry, n, k, m, dtype):
    g = gen(n + k + m)
    x, res = rnd(g, m, k, dtype=dtype), rnd(g, m, n, dtype=dtype)
    ops = {"residual": Op(res, skew=2, out=True), "x": Op(x, stride=k + 8), "w": Op(weight(n, k, dtype, True))}
    if entry.endswith("ssq"):
        ops["ssq_out"] = Op(torch.zeros(m, n // 16), skew=4, out=True)
    run(ops, lambda t: kcall(entry, residual=t["residual"], x=t["x"], w=t["w"], M=m, N=n, K=k, x_row_stride=k + 8, dtype=dtype,
                             **({"ssq_out": t["ssq_out"]} if "ssq_out" in t else {})), finite=list(o for o in ops if ops[o].out))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("entry", ["swl_gemm_tiny_partial_from_attn", "swl_gemm_tiny_partial_from_splitk",
                                   "swl_gemm_tiny_silu_gate_from_splitk"])
def test_gemm_tiny(entry, m, dtype):
    """The smallest geometry the kernel takes: one workgroup column (N = 32, I = 64), K = 256 = two 128-column tiles."""
    g, k, kso, ksi = gen(m + len(entry)), 256, 2, 2
    if entry == "swl_gemm_tiny_partial_from_attn":
        n, H, D, sbs, nsb = 32, 8, 32, 64, 2
        lens = [100, 17, 1, 70][:m]
        mid_o, mid_lse = rnd(g, m, H, nsb, D), rnd(g, m, H, nsb)
        for s, ln in enumerate(lens):                       # splits past a sequence are never written by phase 1: not to be read
            used = -(-ln // sbs)
            mid_o[s, :, used:], mid_lse[s, :, used:] = float("nan"), float("nan")
        scratch = torch.cat([mid_o.flatten(), mid_lse.flatten()])
        assert scratch.numel() == scratch_floats(m, H, D, nsb)
        ops = {"slabs_out": Op(torch.zeros(kso, m, n), out=True), "attn": Op(scratch), "seq_lens": Op(i32(lens), skew=4),
               "w": Op(weight(n, k, dtype, True))}
        run(ops, lambda t: kcall(entry, slabs_out=t["slabs_out"], slabs_out_bytes=kso * m * n * 4, k_splits_out=kso,
                                 attn_scratch=t["attn"], seq_lens=t["seq_lens"], num_q_heads=H, head_dim=D, seq_block_size=sbs,
                                 num_seq_blocks=nsb, w=t["w"], M=m, N=n, dtype=dtype), finite=["slabs_out"])
        return
    ops = {"slabs_in": Op(rnd(g, ksi, m, k, scale=0.5)), "residual_in": Op(rnd(g, m, k, dtype=dtype)),
           "residual_out": Op(torch.zeros(m, k, dtype=dtype), out=True), "norm_w": Op(rnd(g, k, dtype=dtype))}
    if entry == "swl_gemm_tiny_partial_from_splitk":
        n = 32
        ops.update(slabs_out=Op(torch.zeros(kso, m, n), out=True), ssq_out=Op(torch.zeros(kso, m), skew=4, out=True),
                   w=Op(weight(n, k, dtype, True)))
        run(ops, lambda t: kcall(entry, slabs_out=t["slabs_out"], slabs_out_bytes=kso * m * n * 4, k_splits_out=kso,
                                 ssq_out=t["ssq_out"], slabs_in=t["slabs_in"], k_splits_in=ksi, residual_in=t["residual_in"],
                                 residual_out=t["residual_out"], norm_w=t["norm_w"], w=t["w"], M=m, N=n, K=k, dtype=dtype),
            finite=["slabs_out", "ssq_out", "residual_out"])
    else:
        inter = 64
        ops.update(out=Op(torch.zeros(m, inter, dtype=dtype), skew=8, stride=inter + 4, out=True),
                   w=Op(weight(2 * inter, k, dtype, True, seed=1)))
        run(ops, lambda t: kcall(entry, out=t["out"], slabs_in=t["slabs_in"], k_splits_in=ksi, residual_in=t["residual_in"],
                                 residual_out=t["residual_out"], norm_w=t["norm_w"], eps=1e-5, w=t["w"], M=m, I=inter, K=k,
                                 out_row_stride=inter + 4, dtype=dtype), finite=["out", "residual_out"])


# ---- integer kernels ------------------------------------------------------------------------------------------------------------
def test_block_table_and_positions():
    g, rows, mbps, nblocks = gen(3), 6, 4, 24
    ids, have, need = i32([4, 0, 3]), [1, 0, 2], [2, 1, 1]          # batch of three sequences
    bt = torch.full((rows, mbps), nblocks - 1, dtype=I32)
    nalloc = torch.zeros(rows, dtype=I32)
    free = torch.ones(nblocks, dtype=U8)
    pool = torch.randperm(nblocks - 1, generator=g).to(I32)
    for s, n in zip(ids.tolist(), have):
        bt[s, :n] = pool[:n]
        free[pool[:n].long()] = 0
        pool, nalloc[s] = pool[n:], n
    cand = pool[:sum(need)]
    ops = {"nalloc": Op(nalloc, skew=4, out=True), "bt": Op(bt, skew=4, out=True), "cand": Op(cand, skew=4), "ids": Op(ids, skew=4),
           "need": Op(i32(need), skew=4), "cum": Op(i32([0, 2, 3]), skew=4), "free": Op(free, skew=1, out=True)}
    want = run(ops, lambda t: kcall("swl_block_table_set", num_seq_allocated_blocks=t["nalloc"], block_table=t["bt"],
                                    candidate_blocks=t["cand"], seq_ids=t["ids"], block_needed=t["need"],
                                    block_needed_excl_cumsum=t["cum"], is_block_free=t["free"], batch_size=3,
                                    max_blocks_per_seq=mbps))
    assert want["nalloc"][ids.long()].tolist() == [3, 1, 3] and int(want["free"].sum()) == nblocks - 7
    bt2, nalloc2, free2 = want["bt"], want["nalloc"], want["free"]
    tail = {"nalloc": Op(nalloc2, skew=4, out=True), "bt": Op(bt2, skew=4), "ids": Op(ids, skew=4), "free": Op(free2, skew=1, out=True)}
    want = run(tail, lambda t: kcall("swl_block_table_unset", num_seq_allocated_blocks=t["nalloc"], block_table=t["bt"],
                                     seq_ids=t["ids"], is_block_free=t["free"], batch_size=3, max_blocks_per_seq=mbps))
    assert int(want["nalloc"].sum()) == 0 and int(want["free"].sum()) == nblocks
    tail.update(cum=Op(i32([0, 3, 4]), skew=4), gathered=Op(torch.full((7,), -7, dtype=I32), skew=4, out=True))
    want = run(tail, lambda t: kcall("swl_block_table_gather", num_seq_allocated_blocks=t["nalloc"], block_table=t["bt"],
                                     seq_ids=t["ids"], is_block_free=t["free"], out_excl_cumsum=t["cum"],
                                     gathered_block_ids=t["gathered"], batch_size=3, max_blocks_per_seq=mbps))
    assert want["gathered"].tolist() == [int(b) for s, n in zip(ids.tolist(), [3, 1, 3]) for b in bt2[s, :n]]
    lens = i32([1, 16, 17, 100, 5])
    want = run({"pos": Op(torch.full((5,), -7, dtype=I32), skew=4, out=True), "lens": Op(lens, skew=4)},
               lambda t: kcall("swl_decode_positions", pos_idx=t["pos"], seq_lens=t["lens"], num_decoding_seqs=5))
    assert torch.equal(want["pos"], lens - 1)


@pytest.mark.parametrize("swap_in", [1, 0])
def test_swap_blocks_device_side(swap_in):
    """The device pools sit in the arena (the host swap pools are plain pinned tensors): runs of blocks land where the id
    lists say and nowhere else."""
    g, nb, block = gen(5), 8, 4096
    kd, vd = torch.randint(0, 255, (nb, block), generator=g, dtype=U8), torch.randint(0, 255, (nb, block), generator=g, dtype=U8)
    kh = torch.randint(0, 255, (nb, block), generator=g, dtype=U8).pin_memory()
    vh = torch.randint(0, 255, (nb, block), generator=g, dtype=U8).pin_memory()
    src, dst = torch.tensor([1, 2, 5], dtype=I64), torch.tensor([4, 5, 0], dtype=I64)       # one run of two, one single
    kh0, vh0 = kh.clone(), vh.clone()
    lib = _hip.load()

    def call(t):
        kh.copy_(kh0), vh.copy_(vh0)
        rc = lib.swl_swap_blocks(src.data_ptr(), dst.data_ptr(), 3, swap_in, t["k"].data_ptr(), t["v"].data_ptr(),
                                 kh.data_ptr(), vh.data_ptr(), block, _hip.stream())
        assert rc == 0
        torch.cuda.synchronize()

    want = run_case({"k": Op(kd, out=True), "v": Op(vd, out=True)}, call, DEV, sync=torch.cuda.synchronize)
    if swap_in:
        exp = kd.clone()
        exp[dst] = kh0[src]
        assert torch.equal(want["k"], exp)
    else:
        exp = kh0.clone()
        exp[dst] = kd[src]
        assert torch.equal(kh, exp) and torch.equal(want["k"], kd) and torch.equal(want["v"], vd)
