// kv_store.h — what the kernels that write K/V into the paged pools do alike (kvcache.hip, rotary.hip), device and host:
// the pool geometry, the slots a workgroup owns (a block span of a prefill chunk, the one slot of a decode token), the
// 16-byte store into either pool format, the rotary item bodies, and the argument checks of their entry points.
// Not for paged_attn.hip's prologue or decode_engine.hip: their rotary + store is part of a tuned schedule.
#pragma once

#include <initializer_list>

#include "fp8_kv.h"

namespace swl {

// ---- device side ----------------------------------------------------------------------------------------------------------

// Pool layout [num_blocks, L, KVH, block_size, D]: the [KVH, block_size, D] tile of one (block, layer) is contiguous
// (32 KiB for Llama-3-8B in 16 bits, 16 KiB in FP8), so a workgroup that owns one logical block of one sequence writes one
// contiguous run per pool with 16-byte stores. All pool offsets are int64 (a 288 GB pool has > 2^31 elements).
struct KvGeom {
    int layer, L, KVH, bs, D, mbps;   // current layer, layers, kv heads, tokens per block, head dim, block-table row width
    // element offset of the tile of (blk, layer) — elements are bytes in an FP8 pool
    __host__ __device__ int64_t tile(int64_t blk) const { return (blk * L + layer) * KVH * static_cast<int64_t>(bs) * D; }
    __host__ __device__ int64_t head_pitch() const { return static_cast<int64_t>(bs) * D; }
};

// Elements in one 16-byte store into a pool of `Pool` elements: 8 (16-bit pools) or 16 (FP8 pools).
template <typename Pool>
constexpr int kPutElems = 16 / static_cast<int>(sizeof(Pool));

// One 16-byte store into a pool. A 16-bit pool takes a bit-exact copy of 8 elements. A byte pool takes 16 elements — two
// 16-byte reads of the 16-bit projection — as fp32(x) * inv, clamped to +-448 and rounded to nearest even by
// v_cvt_pk_fp8_f32 (the contract and the host twin: fp8_kv.h); `inv` is the inverse scale of the (layer, kv head).
template <typename T, typename Pool>
__device__ __forceinline__ void put16(Pool *dst, const T *src, float inv) {
    if constexpr (sizeof(Pool) == 1)
        *reinterpret_cast<u32x4_t *>(dst) = quantise16<T>(load8(src), load8(src + 8), inv);
    else
        store8(dst, load8(src));
}

// The current layer's rows of inv_scales, fp32 [2, L, KVH] with the k rows first. 16-bit pools have no scales: the
// pointer (NULL there) is not touched and put16 ignores the 1.
template <typename Pool>
struct InvRows {
    const float *k_row = nullptr, *v_row = nullptr;
    __device__ __forceinline__ InvRows(const float *inv_scales, const KvGeom &g) {
        if constexpr (sizeof(Pool) == 1) {
            k_row = inv_scales + static_cast<int64_t>(g.layer) * g.KVH;
            v_row = k_row + static_cast<int64_t>(g.L) * g.KVH;
        }
    }
    __device__ __forceinline__ float k(int h) const { return sizeof(Pool) == 1 ? k_row[h] : 1.0f; }
    __device__ __forceinline__ float v(int h) const { return sizeof(Pool) == 1 ? v_row[h] : 1.0f; }
};

// The prefill block span. Sequence s already holds ctx = ctx_lens[s] tokens (NULL: every context is 0, whole prompts):
// token t of its chunk goes to logical position ctx + t. A chunk may start and end inside a block, so a chunk of n tokens
// touches up to ceil(n / bs) + 1 logical blocks (ceil(n / bs) at context 0): workgroup (x, s) owns logical block
// ctx / bs + x and writes the slots of it that lie in [ctx, ctx + n) — nothing else of the pool is touched.
struct PrefillSpan {
    int ctx, pos0, lo, hi;   // context; first position of the block; the positions [lo, hi) of it that the chunk owns
    int64_t start, tile;     // first token row of the sequence in k / v; pool offset of the block's tile
    __device__ __forceinline__ bool owns(int pos) const { return pos >= lo && pos < hi; }
    __device__ __forceinline__ int64_t tok(int pos) const { return start + (pos - ctx); }
};

// false: this workgroup has nothing to write (and never indexes outside the table row).
// CTX = false: ctx_lens is not looked at and the context is the constant 0 — the plain 16-bit store's instantiation, whose
// prologue then folds to `tok0 / ntok` (why not a runtime NULL: profiles/kv_store_shared_kernel_resources.md).
template <bool CTX = true>
__device__ __forceinline__ bool prefill_span(PrefillSpan &sp, const KvGeom &g, const int *__restrict__ block_table,
                                             const int *__restrict__ seq_ids, const int *__restrict__ start_locs,
                                             const int *__restrict__ seq_lens, const int *__restrict__ ctx_lens) {
    const int s = blockIdx.y;
    sp.ctx = CTX && ctx_lens ? ctx_lens[s] : 0;
    const int len = seq_lens[s];
    const int lb = sp.ctx / g.bs + blockIdx.x;   // logical block inside the sequence
    sp.pos0 = lb * g.bs;
    sp.lo = max(sp.pos0, sp.ctx), sp.hi = min(sp.pos0 + g.bs, sp.ctx + len);
    if (sp.lo >= sp.hi || sp.ctx < 0 || lb >= g.mbps) return false;
    sp.start = start_locs[s];
    const int seq_id = seq_ids[s];
    sp.tile = g.tile(block_table[static_cast<int64_t>(seq_id) * g.mbps + lb]);
    return true;
}

// The tile walk: items [kvh][slot][chunk] of `cpr` chunks per (slot, head) row, in destination order (item `it` is the
// it-th 16-byte store of the tile when a chunk is a whole store), 256 threads. f(it, h, t, c, pos) for the owned slots.
template <typename F>
__device__ __forceinline__ void walk_tile(const KvGeom &g, const PrefillSpan &sp, int cpr, F &&f) {
    const int items = g.KVH * g.bs * cpr;
    for (int it = threadIdx.x; it < items; it += 256) {
        const int c = it % cpr;
        const int t = (it / cpr) % g.bs;
        const int h = it / (cpr * g.bs);
        const int pos = sp.pos0 + t;
        if (sp.owns(pos)) f(it, h, t, c, pos);
    }
}

// The decode slot of token i of a decode batch: position seq_lens[i] - 1 of its sequence.
struct DecodeSlot {
    int pos;
    int64_t base;   // pool offset of (blk, layer, kvh = 0, slot, 0); kv head h is h * g.head_pitch() further
};

// false: an inert row of a padded decode batch (length 0: worker/model.py, hipGraph buckets) — nothing rotated or stored
__device__ __forceinline__ bool decode_slot(DecodeSlot &ds, const KvGeom &g, const int *__restrict__ block_table,
                                            const int *__restrict__ seq_ids, const int *__restrict__ seq_lens, int64_t i) {
    const int seq_id = seq_ids[i];
    ds.pos = seq_lens[i] - 1;
    if (ds.pos < 0) return false;
    const int64_t blk = block_table[static_cast<int64_t>(seq_id) * g.mbps + ds.pos / g.bs];
    const int slot = ds.pos % g.bs;
    ds.base = g.tile(blk) + static_cast<int64_t>(slot) * g.D;
    return true;
}

// Rotary items. One lane owns 8 consecutive elements of the first half of a head and the matching 8 of the second half
// (two 16-byte loads, two 16-byte stores); cos/sin come as one 16-byte load each from row `row` of the tables.
// Rounding points: rotate8 (swl_common.h).
template <typename T>
__device__ __forceinline__ void rotate_item(T *head, const T *cos_t, const T *sin_t, int64_t row, int half, int c,
                                            vec8_t<T> &x0, vec8_t<T> &x1) {
    const vec8_t<T> cv = load8(cos_t + row * half + c * 8);
    const vec8_t<T> sv = load8(sin_t + row * half + c * 8);
    x0 = load8(head + c * 8), x1 = load8(head + half + c * 8);
    rotate8<T>(x0, x1, cv, sv);
    store8(head + c * 8, x0);
    store8(head + half + c * 8, x1);
}

// chunk c of the q or k head at `head`, rotated in place
template <typename T>
__device__ __forceinline__ void rotate_in_place(T *head, const T *cos_t, const T *sin_t, int64_t row, int half, int c) {
    vec8_t<T> x0, x1;
    rotate_item<T>(head, cos_t, sin_t, row, half, c, x0, x1);
}

// a k item: rotated, written back (the prefill attention reads the fresh projections, not the pool) AND written into the
// head's row `dst` of the pool tile
template <typename T>
__device__ __forceinline__ void rotate_k_item(T *head, T *dst, const T *cos_t, const T *sin_t, int64_t row, int half,
                                              int c) {
    vec8_t<T> x0, x1;
    rotate_item<T>(head, cos_t, sin_t, row, half, c, x0, x1);
    store8(dst + c * 8, x0);
    store8(dst + half + c * 8, x1);
}

// ---- host side ------------------------------------------------------------------------------------------------------------

// What an entry point of the family was handed. No check relies on a default: an entry runs only the steps whose fields
// its prototype has (swl_rotary has no pools and no geometry beyond the heads and head_dim).
struct KvStoreArgs {
    void *q = nullptr, *k = nullptr, *v = nullptr;           // [tokens, heads, D] rows of T, strided by the token pitch
    const void *cos_table = nullptr, *sin_table = nullptr;
    const int32_t *pos_idx = nullptr;                        // nullable
    void *k_cache = nullptr, *v_cache = nullptr;
    const float *inv_scales = nullptr;                       // FP8 pools only
    const int32_t *block_table = nullptr, *seq_ids = nullptr, *start_locs = nullptr, *seq_lens = nullptr;
    const int32_t *ctx_lens = nullptr;                       // nullable where the entry says so
    int64_t num_seqs = 0;                                    // sequences (swl_rotary: tokens)
    int max_len = 1;                                         // prefill entries: the longest chunk (0: an empty batch)
    int H = 1;                                               // q heads; the plain stores have none to check
    KvGeom g{};
    int64_t q_tok_stride = 0, k_tok_stride = 0, v_tok_stride = 0;
    const float *slabs = nullptr;                            // split-K partials of the fused qkv projection, or NULL
    int k_splits = 0;
    bool empty() const { return num_seqs == 0 || max_len == 0; }
};

// Callers are promised every refusal code, double faults included (tests/_contract.py), so the checks are steps that
// return one code each and an entry lists them in the order it runs them. Most steps answer SWL_ERR_BAD_ARG; which of
// the two codes a bad head_dim gets, and where in the order, differs between the entries and is an argument of the step.
//   check_kv_counts           SWL_ERR_BAD_ARG; then an empty batch is SWL_OK with nothing else looked at (the entry returns)
//   check_present             SWL_ERR_BAD_ARG
//   check_heads               SWL_ERR_BAD_ARG
//   check_kv_geometry         SWL_ERR_BAD_ARG (the heads included)
//   check_head_dim_chunks     head_dim <= 0: SWL_ERR_BAD_ARG; not a multiple of the store item: `code`
//   check_head_dim_rotary     head_dim <= 0: SWL_ERR_BAD_ARG; not one the rotary kernels are built for: `code`
//   check_tok_stride          SWL_ERR_BAD_ARG
//   check_aligned16           SWL_ERR_BAD_ARG
//   check_slabs               SWL_ERR_BAD_ARG
//   check_prefill_grid        SWL_ERR_UNSUPPORTED — the last step of every prefill entry
#define SWL_KV_CHECK(step)                                     \
    do {                                                       \
        if (const int rc_ = (step); rc_ != SWL_OK) return rc_; \
    } while (0)

inline int check_kv_counts(const KvStoreArgs &a) { return a.num_seqs < 0 || a.max_len < 0 ? SWL_ERR_BAD_ARG : SWL_OK; }

inline int check_present(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!p) return SWL_ERR_BAD_ARG;
    return SWL_OK;
}

inline int check_heads(const KvStoreArgs &a) { return a.H <= 0 || a.g.KVH <= 0 ? SWL_ERR_BAD_ARG : SWL_OK; }

inline int check_kv_geometry(const KvStoreArgs &a) {
    const KvGeom &g = a.g;
    SWL_KV_CHECK(check_heads(a));
    return g.L <= 0 || g.layer < 0 || g.layer >= g.L || g.bs <= 0 || g.D <= 0 || g.mbps <= 0 ? SWL_ERR_BAD_ARG : SWL_OK;
}

// a store item is `elems` elements: 8 into 16-bit pools, 16 into FP8 pools
inline int check_head_dim_chunks(const KvStoreArgs &a, int elems, int code) {
    return a.g.D <= 0 ? SWL_ERR_BAD_ARG : (a.g.D & (elems - 1)) ? code : SWL_OK;
}

inline int check_head_dim_rotary(const KvStoreArgs &a, int code) {
    const int D = a.g.D;
    return D <= 0 ? SWL_ERR_BAD_ARG : D == 32 || D == 64 || D == 128 || D == 256 ? SWL_OK : code;
}

// rows of `heads` heads, read and written 16 bytes at a time
inline int check_tok_stride(const KvStoreArgs &a, int64_t stride, int heads) {
    return stride < static_cast<int64_t>(heads) * a.g.D || (stride & 7) ? SWL_ERR_BAD_ARG : SWL_OK;
}

inline int check_aligned16(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!aligned16(p)) return SWL_ERR_BAD_ARG;
    return SWL_OK;
}

inline int check_slabs(const KvStoreArgs &a) {
    return a.slabs && (a.k_splits <= 0 || !aligned16(a.slabs)) ? SWL_ERR_BAD_ARG : SWL_OK;
}

// grid.y = the sequence
inline int check_prefill_grid(const KvStoreArgs &a) { return a.num_seqs > 65535 ? SWL_ERR_UNSUPPORTED : SWL_OK; }

// The checks every store into the pools shares, all SWL_ERR_BAD_ARG: the pools, the k and v rows and the tables are there,
// the geometry is one, head_dim is a whole number of store items, the k and v rows fit their pitch, 16-byte alignment.
inline int check_store_operands(const KvStoreArgs &a, int item_elems) {
    SWL_KV_CHECK(check_present({a.k_cache, a.v_cache, a.k, a.v, a.block_table, a.seq_ids, a.seq_lens}));
    SWL_KV_CHECK(check_kv_geometry(a));
    SWL_KV_CHECK(check_head_dim_chunks(a, item_elems, SWL_ERR_BAD_ARG));
    SWL_KV_CHECK(check_tok_stride(a, a.k_tok_stride, a.g.KVH));
    SWL_KV_CHECK(check_tok_stride(a, a.v_tok_stride, a.g.KVH));
    return check_aligned16({a.k_cache, a.v_cache, a.k, a.v});
}

} // namespace swl
