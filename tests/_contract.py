"""The argument contract of every entry point of include/swiftllm_hip.h as a table: one row per name in
`_hip.SIGNATURES` with a small legal call (the baseline) and the one-field changes that must be refused (the violations).

Pointers are fake: 256-byte aligned addresses inside one host buffer, so a row can only be *called* where no HIP device
exists (an accepted call then fails at the launch with SWL_ERR_LAUNCH, or SWL_ERR_RUNTIME for the host-side copy of
swl_swap_blocks — never -1 / -2). tests/test_abi_contract.py does that; tests/test_gpu_contract.py uses the same shapes.

A row is written with the field helpers below, in the order of the C prototype; most violations follow from the kind of
a field:
  P(name, align)        pointer: NULL (unless nullable) and the base moved by align / 2 bytes (the largest step that breaks
                        the documented alignment and nothing else) -> SWL_ERR_BAD_ARG
  C(name, value)        count: -1 -> SWL_ERR_BAD_ARG
  S(name, v, width, m)  stride of rows `width` wide that must be a multiple of m: -m, width - m (one unit short) and
                        v + m / 2 (off the multiple, m > 1) -> SWL_ERR_BAD_ARG
  DT()                  dtype code: 7 -> SWL_ERR_BAD_ARG
  V(name, value)        anything else; its violations are listed explicitly as (label, field, value, expected code).
"""
import ctypes

from swiftllm_amd import _hip

BAD, UNSUP = -1, -2

_BUF = ctypes.create_string_buffer(1 << 20)
_BASE = (ctypes.addressof(_BUF) + 255) // 256 * 256
_SLOT = 4096          # bytes between two fake operands (swl_swap_blocks really copies block_bytes between two of them)


class _Field:
    def __init__(self, kind, name, value=None, **kw):
        self.kind, self.name, self.value, self.kw = kind, name, value, kw


def P(name, align=16, nullable=False):
    return _Field("ptr", name, align=align, nullable=nullable)


def C(name, value):
    return _Field("count", name, value)


def S(name, value, width, mult=8):
    return _Field("stride", name, value, width=width, mult=mult)


def V(name, value):
    return _Field("value", name, value)


def DT():
    return _Field("dtype", "dtype", _hip.SWL_F16)


def ST():
    return _Field("value", "stream", None)


class Row:
    """name, args (field name -> baseline value, in prototype order), violations [(label, field, value, code)], note."""

    def __init__(self, name, fields, extra=(), note=None, call_baseline=True):
        assert len(fields) == len(_hip.SIGNATURES[name]), (name, len(fields), len(_hip.SIGNATURES[name]))
        self.name, self.note, self.call_baseline = name, note, call_baseline
        self.args, self.violations = {}, []
        slot = 1
        for f in fields:
            assert f.name not in self.args, (name, f.name)
            if f.kind == "ptr":
                f.value = _BASE + slot * _SLOT
                slot += 1
            self.args[f.name] = f.value
        for f in fields:
            if f.kind == "ptr":
                if not f.kw["nullable"]:
                    self._add(f"{f.name} NULL", f.name, None, BAD)
                if f.kw["align"] > 1:
                    self._add(f"{f.name} at +{f.kw['align'] // 2} bytes", f.name, f.value + f.kw["align"] // 2, BAD)
            elif f.kind == "count":
                self._add(f"{f.name} negative", f.name, -1, BAD)
            elif f.kind == "stride":
                w, m = f.kw["width"], f.kw["mult"]
                self._add(f"{f.name} negative", f.name, -m, BAD)
                self._add(f"{f.name} below the row width", f.name, w - m, BAD)
                if m > 1:
                    self._add(f"{f.name} off its multiple of {m}", f.name, f.value + m // 2, BAD)
            elif f.kind == "dtype":
                self._add("dtype code 7", f.name, 7, BAD)
        for label, field, value, code in extra:
            self._add(label, field, value, code)

    def _add(self, label, field, value, code):
        assert field in self.args, (self.name, field)
        self.violations.append((label, field, value, code))

    def call(self, lib, **override):
        args = dict(self.args)
        args.update(override)
        return getattr(lib, self.name)(*args.values())


# ---- shapes (those of tests/test_gpu_contract.py) ------------------------------------------------------------------------------
T, HID = 3, 136                                       # element-wise rows
BD, H, KVH, D, L, LAYER, BS, MBPS = 4, 8, 2, 64, 2, 1, 16, 8   # attention / KV stores: G = 4
SBS, NSB = 64, 2
QKV = (H + 2 * KVH) * D
PITCH = QKV + 8                                       # q, k, v as column slices of one padded qkv row
QW, KW = H * D, KVH * D
M, N, K = 5, 64, 1536                                  # skinny GEMMs: two tiles, twelve K-tiles (six per split)
KS = 2
ARGMAX_SCRATCH = 3 * 64 * 8                            # swl_argmax_scratch_bytes(3)


def _attn_tail(o_stride=True, q_stride=False):
    f = [V("softmax_scale", 0.125), C("num_decoding_seqs", BD), C("num_q_heads", H), C("num_kv_heads", KVH),
         V("head_dim", D), C("num_layers", L), V("block_size", BS), V("cur_layer", LAYER), C("max_blocks_per_seq", MBPS),
         V("seq_block_size", SBS), C("num_seq_blocks", NSB)]
    if q_stride:
        f.append(S("q_tok_stride", QW + 8, QW))
    if o_stride:
        f.append(S("o_tok_stride", QW + 8, QW))
    return f + [DT(), ST()]


def _attn_extra(bad_head_dim=UNSUP):
    return [("H % KVH != 0", "num_q_heads", 7, BAD), ("group size 3", "num_q_heads", 6, UNSUP),
            ("head_dim 48", "head_dim", 48, bad_head_dim), ("block_size 32", "block_size", 32, UNSUP),
            ("cur_layer -1", "cur_layer", -1, BAD), ("cur_layer == L", "cur_layer", L, BAD),
            ("max_blocks_per_seq 0", "max_blocks_per_seq", 0, BAD),
            ("seq_block_size 0", "seq_block_size", 0, BAD), ("seq_block_size % 16", "seq_block_size", 24, BAD),
            ("65536 sequences", "num_decoding_seqs", 65536, UNSUP)]


def _store_fields(prefill, at=False, fp8=False, rotary=False, decode_order=False):
    """The KV-store family: [q] k v [cos sin pos] pools tables counts strides."""
    pools = [P("k_cache"), P("v_cache")]
    tables = [P("block_table", 1), P("seq_ids", 1)] + ([P("start_locs", 1)] if prefill else []) + [P("seq_lens", 1)]
    if at:
        tables.append(P("ctx_lens", 1, nullable=fp8))
    counts = ([C("num_prefill_seqs", 2), C("max_prefill_len", 33)] if prefill else [C("num_decoding_seqs", BD)])
    f = []
    if rotary:
        f += [P("q"), P("k"), P("v"), P("cos_table"), P("sin_table"), P("pos_idx", 1, nullable=True)] + pools
    else:
        f += pools + [P("k"), P("v")] + ([P("inv_scales", 1)] if fp8 else [])
    f += tables + counts
    if decode_order:   # swl_rotary_store_kv_decode: H KVH D layer L bs mbps
        f += [C("num_q_heads", H), C("num_kv_heads", KVH), V("head_dim", D), V("cur_layer", LAYER), C("num_layers", L),
              C("block_size", BS), C("max_blocks_per_seq", MBPS)]
    else:
        f += [V("cur_layer", LAYER), C("num_layers", L)] + ([C("num_q_heads", H)] if rotary else []) + \
             [C("num_kv_heads", KVH), C("block_size", BS), V("head_dim", D), C("max_blocks_per_seq", MBPS)]
    if rotary:
        f.append(S("q_tok_stride", PITCH, QW))
    f += [S("k_tok_stride", PITCH, KW), S("v_tok_stride", PITCH, KW), DT(), ST()]
    return f


def _store_extra(bad_dim, dim_code, prefill):
    e = [("cur_layer -1", "cur_layer", -1, BAD), ("cur_layer == L", "cur_layer", L, BAD),
         ("block_size 0", "block_size", 0, BAD), ("max_blocks_per_seq 0", "max_blocks_per_seq", 0, BAD),
         (f"head_dim {bad_dim}", "head_dim", bad_dim, dim_code), ("head_dim 0", "head_dim", 0, BAD)]
    if prefill:
        e.append(("65536 sequences", "num_prefill_seqs", 65536, UNSUP))
    return e


def _gemm_out(m=M, n=N, k=K, x_align=16, with_ws=True, wide=False, ks=KS):
    f = [P("out", 8), P("x"), P("w")]
    if with_ws:
        f += [P("workspace"), V("workspace_bytes", ks * m * n * 4)]
    f += [C("M", m), C("N", n), C("K", k), S("x_row_stride", k + 8, k), S("out_row_stride", n + 4, n, 4)]
    if wide:
        f.append(V("waves_per_group", 4))
    if with_ws:
        f.append(V("k_splits", ks))
    return f + [DT(), ST()]


def _gemm_partial(m=M, n=N, k=K, wide=False, pre=(), ks=KS):
    f = [P("slabs"), V("slabs_bytes", ks * m * n * 4)] + list(pre) + [P("x"), P("w")]
    f += [C("M", m), C("N", n), C("K", k), S("x_row_stride", k + 8, k)]
    if wide:
        f.append(V("waves_per_group", 4))
    return f + [V("k_splits", ks), DT(), ST()]


def _shape_extra(max_m, k_tile, n_name="N"):
    return [(f"M = {max_m + 1}", "M", max_m + 1, UNSUP), (f"{n_name} % 32", n_name, 100, UNSUP),
            (f"K % {k_tile}", "K", K + 8, UNSUP), (f"{n_name} 0", n_name, 0, BAD), ("K 0", "K", 0, BAD)]


def _splits_extra(zero_ok):
    e = [("k_splits 3", "k_splits", 3, BAD), ("k_splits 32", "k_splits", 32, BAD), ("k_splits -1", "k_splits", -1, BAD)]
    return e if zero_ok else e + [("k_splits 0", "k_splits", 0, BAD)]


def _rows():
    rows = []

    def add(*a, **kw):
        rows.append(Row(*a, **kw))

    # ---- element-wise -----------------------------------------------------------------------------------------------------------
    hid_extra = [("hidden % 8", "hidden", HID + 4, BAD), ("hidden -8", "hidden", -8, BAD),
                 ("hidden past 16384", "hidden", 16392, UNSUP)]
    add("swl_rmsnorm", [P("x"), P("w"), V("eps", 1e-5), C("num_tokens", T), V("hidden", HID), DT(), ST()], hid_extra)
    add("swl_fused_add_rmsnorm", [P("x"), P("residual"), P("w"), V("eps", 1e-5), C("num_tokens", T), V("hidden", HID),
                                  DT(), ST()], hid_extra)
    add("swl_splitk_fused_add_rmsnorm",
        [P("x_out"), P("residual"), P("w"), V("eps", 1e-5), P("slabs"), V("k_splits", KS), C("num_tokens", T),
         V("hidden", HID), DT(), ST()], hid_extra + [("k_splits 0", "k_splits", 0, BAD), ("k_splits -1", "k_splits", -1, BAD)])
    add("swl_splitk_add_scale",
        [P("x_scaled"), P("residual"), P("w"), P("slabs"), V("k_splits", KS), P("ssq_out", 1), C("num_tokens", T),
         V("hidden", 1024), DT(), ST()],
        [("hidden % 1024", "hidden", 1032, UNSUP), ("hidden -8", "hidden", -8, BAD), ("k_splits 0", "k_splits", 0, BAD),
         ("65536 tokens", "num_tokens", 65536, UNSUP)])
    add("swl_silu_mul", [P("x"), C("num_tokens", T), V("ffn_inter_dim", 264), DT(), ST()],
        [("I % 8", "ffn_inter_dim", 260, BAD), ("I -8", "ffn_inter_dim", -8, BAD)])
    add("swl_rotary",
        [P("q"), P("k"), P("cos_table"), P("sin_table"), P("pos_idx", 1, nullable=True), C("num_tokens", 5),
         C("num_q_heads", H), C("num_kv_heads", KVH), V("head_dim", D), S("q_tok_stride", PITCH, QW),
         S("k_tok_stride", PITCH, KW), DT(), ST()],
        [("head_dim 48", "head_dim", 48, BAD), ("head_dim 0", "head_dim", 0, BAD)])

    # ---- KV stores --------------------------------------------------------------------------------------------------------------
    add("swl_store_kv_prefill", _store_fields(True), _store_extra(68, BAD, True))
    add("swl_store_kv_prefill_at", _store_fields(True, at=True), _store_extra(68, UNSUP, True))
    add("swl_store_kv_decode", _store_fields(False), _store_extra(68, BAD, False))
    add("swl_rotary_store_kv_prefill", _store_fields(True, rotary=True), _store_extra(48, UNSUP, True))
    add("swl_rotary_store_kv_prefill_at", _store_fields(True, at=True, rotary=True), _store_extra(48, UNSUP, True))
    add("swl_rotary_store_kv_decode", _store_fields(False, rotary=True, decode_order=True), _store_extra(48, BAD, False))
    f = _store_fields(False, rotary=True, decode_order=True)
    f = [P("q_out"), P("k_out"), P("v_out"), P("qkv_slabs"), V("k_splits", KS)] + f[3:]
    add("swl_splitk_rotary_store_kv_decode", f,
        _store_extra(48, BAD, False) + [("k_splits 0", "k_splits", 0, BAD), ("k_splits -1", "k_splits", -1, BAD)])
    add("swl_store_kv_prefill_at_fp8", _store_fields(True, at=True, fp8=True), _store_extra(72, BAD, True),
        note="the pools are bytes; head_dim % 16; ctx_lens may be NULL")
    add("swl_store_kv_decode_fp8", _store_fields(False, fp8=True), _store_extra(72, BAD, False))

    # ---- decode attention -------------------------------------------------------------------------------------------------------
    pools_tables = [P("k_cache"), P("v_cache"), P("block_table", 1), P("seq_ids", 1), P("seq_lens", 1)]
    nsb_extra = [("num_seq_blocks -1", "num_seq_blocks", -1, BAD)]
    add("swl_paged_attn_decode", [P("o"), P("q")] + pools_tables + [P("scratch")] + _attn_tail(q_stride=True),
        _attn_extra() + nsb_extra)
    add("swl_paged_attn_phase1",
        [P("o_direct", nullable=True), P("q")] + pools_tables + [P("mid_o", 4), P("mid_lse", 4)] + _attn_tail(q_stride=True),
        _attn_extra() + nsb_extra, note="o_direct may be NULL with num_seq_blocks > 1; when given it is checked")
    add("swl_paged_attn_phase2",
        [P("o"), P("mid_o", 4), P("mid_lse", 4), P("seq_lens", 1), C("num_decoding_seqs", BD), C("num_q_heads", H),
         V("head_dim", D), V("seq_block_size", SBS), C("num_seq_blocks", NSB), S("o_tok_stride", QW + 8, QW), DT(), ST()],
        [("head_dim 48", "head_dim", 48, UNSUP), ("seq_block_size 0", "seq_block_size", 0, BAD),
         ("65536 sequences", "num_decoding_seqs", 65536, UNSUP)])
    qkv_head = [P("qkv_slabs"), V("k_splits", KS)]
    qkv_mid = [P("cos_table"), P("sin_table"), P("pos_idx", 1, nullable=True), P("k_cache"), P("v_cache"),
               P("block_table", 1), P("seq_ids", 1), P("seq_lens", 1), P("scratch")]
    rs = [P("row_ssq", 1), V("ssq_parts", 2), V("hidden", 1024), V("eps", 1e-5)]
    ks_extra = [("k_splits 0", "k_splits", 0, BAD), ("k_splits -1", "k_splits", -1, BAD)]
    rs_extra = [("k_splits 0", "k_splits", 0, UNSUP), ("k_splits 3", "k_splits", 3, UNSUP), ("k_splits 8", "k_splits", 8, UNSUP),
                ("ssq_parts 9", "ssq_parts", 9, UNSUP), ("ssq_parts 0", "ssq_parts", 0, BAD), ("hidden 0", "hidden", 0, BAD)]
    add("swl_paged_attn_decode_qkv", [P("o")] + qkv_head + qkv_mid + _attn_tail(), _attn_extra() + nsb_extra + ks_extra)
    add("swl_paged_attn_decode_qkv_rs", [P("o")] + qkv_head + rs + qkv_mid + _attn_tail(),
        _attn_extra() + nsb_extra + rs_extra)
    add("swl_paged_attn_decode_qkv_rs_partials", [P("o", nullable=True)] + qkv_head + rs + qkv_mid + _attn_tail(),
        _attn_extra() + nsb_extra + rs_extra, note="o may be NULL with num_seq_blocks > 1; checked when given")
    fp8_pools = [P("k_cache"), P("v_cache"), P("kv_scales", 1), P("block_table", 1), P("seq_ids", 1), P("seq_lens", 1)]
    add("swl_paged_attn_decode_fp8", [P("o"), P("q")] + fp8_pools + [P("scratch")] + _attn_tail(q_stride=True),
        _attn_extra(BAD) + nsb_extra)
    add("swl_paged_attn_phase1_fp8",
        [P("o_direct", nullable=True), P("q")] + fp8_pools + [P("mid_o", 4), P("mid_lse", 4)] + _attn_tail(q_stride=True),
        _attn_extra(BAD) + nsb_extra)

    # ---- prefill attention ------------------------------------------------------------------------------------------------------
    add("swl_prefill_attn_varlen",
        [P("o"), P("q"), P("k"), P("v"), P("cu_seqlens", 1), C("num_prefill_seqs", 3), C("max_prefill_len", 70),
         C("num_q_heads", H), C("num_kv_heads", KVH), V("head_dim", D), V("softmax_scale", 0.125),
         S("q_tok_stride", PITCH, QW), S("k_tok_stride", PITCH, KW), S("v_tok_stride", PITCH, KW),
         S("o_tok_stride", QW + 8, QW), DT(), ST()],
        [("H % KVH != 0", "num_q_heads", 7, BAD), ("head_dim 48", "head_dim", 48, UNSUP)])

    def paged_prefill(fp8):
        return ([P("o"), P("q"), P("k_cache"), P("v_cache")] + ([P("kv_scales", 1)] if fp8 else []) +
                [P("block_table", 1), P("seq_ids", 1), P("cu_seqlens", 1), P("ctx_lens", 1), C("num_prefill_seqs", 3),
                 C("max_new_len", 70), C("max_total_len", 110), C("num_q_heads", H), C("num_kv_heads", KVH),
                 V("head_dim", D), C("num_layers", L), V("block_size", BS), V("cur_layer", LAYER),
                 C("max_blocks_per_seq", MBPS), V("softmax_scale", 0.125), S("q_tok_stride", QW + 8, QW),
                 S("o_tok_stride", QW + 8, QW), DT(), ST()])

    def paged_prefill_extra(dim_code):
        return [("H % KVH != 0", "num_q_heads", 7, BAD), ("head_dim 48", "head_dim", 48, dim_code),
                ("block_size 32", "block_size", 32, UNSUP), ("block_size 0", "block_size", 0, BAD),
                ("cur_layer -1", "cur_layer", -1, BAD), ("cur_layer == L", "cur_layer", L, BAD),
                ("max_total_len < max_new_len", "max_total_len", 69, BAD),
                ("max_total_len past the table row", "max_total_len", MBPS * 16 + 1, BAD),
                ("max_blocks_per_seq below ceil(total / 16)", "max_blocks_per_seq", 6, BAD)]
    add("swl_prefill_attn_paged", paged_prefill(False), paged_prefill_extra(UNSUP))
    add("swl_prefill_attn_paged_fp8", paged_prefill(True), paged_prefill_extra(BAD))

    # ---- sampling ---------------------------------------------------------------------------------------------------------------
    rows_, n = 3, 1000
    need = ARGMAX_SCRATCH         # (test_abi_contract.py holds it to swl_argmax_scratch_bytes; nothing here loads the library)
    add("swl_argmax",
        [P("out", 1), P("x"), P("scratch"), V("scratch_bytes", need), C("num_rows", rows_), V("n", n),
         S("row_stride", n + 8, n), DT(), ST()],
        [("scratch_bytes one short", "scratch_bytes", need - 1, BAD), ("n % 8", "n", n + 4, BAD), ("n 0", "n", 0, BAD),
         ("n -8", "n", -8, BAD)])
    add("swl_sample",
        [P("out", 1), P("x", 2), C("num_rows", rows_), V("n", n), S("row_stride", n + 1, n, 1), DT(),
         P("temperature", 1), P("top_k", 1), P("top_p", 1), P("seed", 1), P("pos", 1), ST()],
        [("n 0", "n", 0, BAD), ("n -1", "n", -1, BAD)])

    # ---- integer kernels --------------------------------------------------------------------------------------------------------
    add("swl_block_table_set",
        [P("num_seq_allocated_blocks", 1), P("block_table", 1), P("candidate_blocks", 1, nullable=True), P("seq_ids", 1),
         P("block_needed", 1), P("block_needed_excl_cumsum", 1), P("is_block_free", 1, nullable=True), C("batch_size", 3),
         V("max_blocks_per_seq", MBPS), ST()], [("max_blocks_per_seq 0", "max_blocks_per_seq", 0, BAD)])
    add("swl_block_table_unset",
        [P("num_seq_allocated_blocks", 1), P("block_table", 1), P("seq_ids", 1), P("is_block_free", 1), C("batch_size", 3),
         V("max_blocks_per_seq", MBPS), ST()], [("max_blocks_per_seq 0", "max_blocks_per_seq", 0, BAD)])
    add("swl_block_table_gather",
        [P("num_seq_allocated_blocks", 1), P("block_table", 1), P("seq_ids", 1), P("is_block_free", 1),
         P("out_excl_cumsum", 1), P("gathered_block_ids", 1, nullable=True), C("batch_size", 3),
         V("max_blocks_per_seq", MBPS), ST()], [("max_blocks_per_seq 0", "max_blocks_per_seq", 0, BAD)])
    add("swl_decode_positions", [P("pos_idx", 1), P("seq_lens", 1), C("num_decoding_seqs", BD), ST()])
    add("swl_swap_blocks",
        [P("src_ids", 1), P("dst_ids", 1), C("num_blocks_to_swap", 1), V("is_swap_in", 1), P("k_cache", 1), P("v_cache", 1),
         P("k_swap", 1), P("v_swap", 1), V("block_bytes", 256), ST()],
        [("block_bytes 0", "block_bytes", 0, BAD), ("block_bytes -256", "block_bytes", -256, BAD)],
        note="host code: src_ids / dst_ids are read on the host (the fake operands are zero-filled host memory: block 0 -> 0)")

    # ---- GEMMs, M <= 32 ---------------------------------------------------------------------------------------------------------
    ws_extra = [("workspace_bytes one short", "workspace_bytes", KS * M * N * 4 - 1, BAD)]
    for name in ("swl_gemm_skinny", "swl_gemm_skinny_packed"):
        add(name, _gemm_out(), _shape_extra(32, 128) + _splits_extra(True) + ws_extra,
            note="workspace may be NULL only when K is not split: here k_splits = 2")
    sl_extra = [("slabs_bytes one short", "slabs_bytes", KS * M * N * 4 - 1, BAD)]
    for name in ("swl_gemm_skinny_partial", "swl_gemm_skinny_packed_partial"):
        add(name, _gemm_partial(), _shape_extra(32, 128) + _splits_extra(False) + sl_extra)

    def silu_fields(m=M, i=N, k=K, pre=(), wide=False):
        f = [P("out", 8), P("x")] + list(pre) + [C("M", m), C("I", i), C("K", k), S("x_row_stride", k + 8, k),
                                                S("out_row_stride", i + 4, i, 4)]
        return f + ([V("waves_per_group", 4)] if wide else []) + [DT(), ST()]
    for name in ("swl_gemm_skinny_silu_gate", "swl_gemm_skinny_packed_silu_gate"):
        add(name, silu_fields(pre=[P("w")]), _shape_extra(32, 128, "I"))
    add("swl_gemm_skinny_packed_silu_gate_rs",
        silu_fields(pre=[P("w"), P("row_ssq", 1), V("ssq_parts", 2), V("eps", 1e-5)]),
        _shape_extra(32, 128, "I") + [("ssq_parts 9", "ssq_parts", 9, UNSUP), ("ssq_parts 0", "ssq_parts", 0, BAD)])
    add("swl_gemm_skinny_packed_silu_gate_nf", silu_fields(pre=[P("norm_w"), V("eps", 1e-5), P("w")]),
        _shape_extra(32, 128, "I"))
    kx = 1024   # the _nx entries run the ring kernel only: K / 128 >= 8
    add("swl_gemm_skinny_packed_silu_gate_nx",
        silu_fields(k=kx, pre=[P("norm_w"), V("eps", 1e-5), P("ssq_in"), V("ssq_parts", 64), P("w")]),
        [("M = 33", "M", 33, UNSUP), ("I % 32", "I", 100, UNSUP), ("K % 128", "K", kx - 8, UNSUP),
         ("K below 8 tiles", "K", 384, UNSUP), ("ssq_parts % 64", "ssq_parts", 65, UNSUP), ("ssq_parts 0", "ssq_parts", 0, UNSUP)])
    add("swl_gemm_skinny_packed_partial_nf",
        [P("slabs"), V("slabs_bytes", KS * M * N * 4), P("ssq_out", 1), P("x"), P("norm_w"), P("w"), C("M", M), C("N", N),
         C("K", K), S("x_row_stride", K + 8, K), V("k_splits", KS), DT(), ST()],
        _shape_extra(32, 128) + _splits_extra(False) + sl_extra)
    add("swl_gemm_skinny_packed_partial_nx",
        [P("slabs"), V("slabs_bytes", KS * M * N * 4), P("x"), P("norm_w"), V("eps", 1e-5), P("ssq_in"), V("ssq_parts", 64),
         P("w"), C("M", M), C("N", N), C("K", kx), S("x_row_stride", kx + 8, kx), V("k_splits", KS), DT(), ST()],
        [("M = 33", "M", 33, UNSUP), ("N % 32", "N", 100, UNSUP), ("K % 128", "K", kx - 8, UNSUP),
         ("ssq_parts % 64", "ssq_parts", 65, UNSUP), ("k_splits 0", "k_splits", 0, BAD), ("k_splits 3", "k_splits", 3, BAD),
         ("k_splits 32", "k_splits", 32, BAD),
         ("k_splits -1", "k_splits", -1, BAD), ("K % (128 * k_splits)", "k_splits", 16, UNSUP)] + sl_extra)
    add("swl_splitk_reduce",
        [P("out", 8), P("slabs"), V("k_splits", KS), C("M", M), V("N", N), S("out_row_stride", N + 4, N, 4), DT(), ST()],
        [("N % 4", "N", N + 2, BAD), ("N 0", "N", 0, BAD), ("k_splits 0", "k_splits", 0, BAD)])
    add("swl_gemm_pack_weight", [P("dst"), P("src"), V("N", N), V("K", K), DT(), ST()],
        [("N % 32", "N", 100, UNSUP), ("K % 16", "K", K + 8, UNSUP), ("N 0", "N", 0, BAD), ("K -16", "K", -16, BAD)])

    # ---- GEMMs, M <= 64 and M <= 256 ------------------------------------------------------------------------------------------
    mm = 33
    add("swl_gemm_packed_mid", _gemm_out(m=mm), _shape_extra(64, 128) + _splits_extra(True) +
        [("workspace_bytes one short", "workspace_bytes", KS * mm * N * 4 - 1, BAD)])
    add("swl_gemm_packed_mid_partial", _gemm_partial(m=mm), _shape_extra(64, 128) + _splits_extra(False) +
        [("slabs_bytes one short", "slabs_bytes", KS * mm * N * 4 - 1, BAD)])
    add("swl_gemm_packed_mid_silu_gate", silu_fields(m=mm, pre=[P("w")]), _shape_extra(64, 128, "I"))
    mw, kw = 65, 1024
    wide_shape = [("M = 257", "M", 257, UNSUP), ("N % 32", "N", 100, UNSUP), ("K % 64", "K", kw - 8, UNSUP),
                  ("waves_per_group 5", "waves_per_group", 5, BAD), ("waves_per_group -4", "waves_per_group", -4, BAD)]
    add("swl_gemm_packed_wide", _gemm_out(m=mw, k=kw, wide=True), wide_shape + _splits_extra(True) +
        [("workspace_bytes one short", "workspace_bytes", KS * mw * N * 4 - 1, BAD)])
    add("swl_gemm_packed_wide_partial", _gemm_partial(m=mw, k=kw, wide=True), wide_shape + _splits_extra(False) +
        [("slabs_bytes one short", "slabs_bytes", KS * mw * N * 4 - 1, BAD), ("K % (64 * k_splits)", "K", 64 * 3, UNSUP)])
    add("swl_gemm_packed_wide_silu_gate", silu_fields(m=mw, k=kw, pre=[P("w")], wide=True),
        [("M = 257", "M", 257, UNSUP), ("I % 32", "I", 100, UNSUP), ("K % 64", "K", kw - 8, UNSUP),
         ("waves_per_group 5", "waves_per_group", 5, BAD)])

    # ---- row-owned and tiny projections -----------------------------------------------------------------------------------------
    kr = 1024
    rows_extra = [("M = 33", "M", 33, UNSUP), ("N % 32", "N", 48, UNSUP), ("K % 1024", "K", kr - 128, UNSUP),
                  ("N 0", "N", 0, BAD), ("K 0", "K", 0, BAD)]
    add("swl_gemm_rows_add", [P("residual", 2), P("x"), P("w"), C("M", M), V("N", 64), V("K", kr),
                              S("x_row_stride", kr + 8, kr), DT(), ST()], rows_extra)
    add("swl_gemm_rows_add_ssq", [P("residual", 2), P("ssq_out", 4), P("x"), P("w"), C("M", M), V("N", 64), V("K", kr),
                                  S("x_row_stride", kr + 8, kr), DT(), ST()], rows_extra)
    tm, tn, tk = 4, 64, 256            # gemm_tiny: one workgroup of two tiles, two 128-column K-tiles
    tiny_bytes = KS * tm * tn * 4
    tiny_extra = [("M = 5", "M", 5, UNSUP), ("slabs_out_bytes one short", "slabs_out_bytes", tiny_bytes - 1, BAD),
                  ("k_splits_out 0", "k_splits_out", 0, BAD), ("k_splits_out -1", "k_splits_out", -1, BAD),
                  ("K chunk % 128", "k_splits_out", 4, UNSUP)]
    add("swl_gemm_tiny_partial_from_attn",
        [P("slabs_out"), V("slabs_out_bytes", tiny_bytes), V("k_splits_out", KS), P("attn_scratch"), P("seq_lens", 1),
         C("num_q_heads", 8), V("head_dim", 32), V("seq_block_size", SBS), V("num_seq_blocks", NSB), P("w"), C("M", tm),
         V("N", tn), DT(), ST()],
        tiny_extra + [("N % 32", "N", 48, UNSUP), ("head_dim % 8", "head_dim", 36, UNSUP),
                      ("seq_block_size 0", "seq_block_size", 0, BAD), ("num_seq_blocks 0", "num_seq_blocks", 0, BAD)])
    add("swl_gemm_tiny_partial_from_splitk",
        [P("slabs_out"), V("slabs_out_bytes", tiny_bytes), V("k_splits_out", KS), P("ssq_out", 1), P("slabs_in"),
         V("k_splits_in", KS), P("residual_in"), P("residual_out"), P("norm_w"), P("w"), C("M", tm), V("N", tn), V("K", tk),
         DT(), ST()],
        tiny_extra + [("N % 32", "N", 48, UNSUP), ("k_splits_in 0", "k_splits_in", 0, BAD),
                      ("K chunk past 4096", "K", 2 * 4096 + 256, UNSUP)])
    add("swl_gemm_tiny_silu_gate_from_splitk",
        [P("out", 8), P("slabs_in"), V("k_splits_in", KS), P("residual_in"), P("residual_out"), P("norm_w"), V("eps", 1e-5),
         P("w"), C("M", tm), V("I", tn), V("K", tk), S("out_row_stride", tn + 4, tn, 4), DT(), ST()],
        [("M = 5", "M", 5, UNSUP), ("I % 64", "I", 32, UNSUP), ("K past 4096", "K", 4096 + 128, UNSUP),
         ("K % 128", "K", tk + 8, UNSUP), ("k_splits_in 0", "k_splits_in", 0, BAD)])
    return rows


ROWS = {r.name: r for r in _rows()}

# same-pointer rules: a second field set to the value of the first
ALIASES = [("swl_gemm_pack_weight", "dst", "src"), ("swl_gemm_tiny_partial_from_splitk", "residual_out", "residual_in"),
           ("swl_gemm_tiny_partial_from_splitk", "slabs_out", "slabs_in"),
           ("swl_gemm_tiny_silu_gate_from_splitk", "residual_out", "residual_in")]
for _name, _field, _other in ALIASES:
    ROWS[_name]._add(f"{_field} == {_other}", _field, ROWS[_name].args[_other], BAD)

EXCLUDED = {
    "swl_decode_engine_reset": "opt-in persistent kernel, off by default and refused in FP8 mode; reset synchronises the "
                               "stream and writes its workspace from the host side of the call",
    "swl_decode_engine_step": "opt-in persistent kernel (one workgroup per CU, bounded waits): not something to call at the "
                              "edges of its contract",
}


def cases():
    """(entry, label, field, value, expected code) of every violation, for pytest.mark.parametrize."""
    return [(r.name, label, field, value, code) for r in ROWS.values() for label, field, value, code in r.violations]
