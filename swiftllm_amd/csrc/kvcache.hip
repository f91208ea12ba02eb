// kvcache.hip — store freshly projected K/V rows into the paged KV pools (gfx950), 16-bit and FP8 (e4m3fn) pools alike.
//
// Replaces _fwd_kvcache_mgmt_prefill_kernel (swiftllm/worker/kernels/kvcache_mgmt.py:10-48) and
// _fwd_kvcache_mgmt_decoding_kernel (kvcache_mgmt.py:50-79). HBM-bound: 4*T*KVH*D*e bytes (K and V, read + write) into
// 16-bit pools, where the stores are bit-exact copies; 3*T*KVH*D*e into FP8 pools, where they quantise (fp8_kv.h).
// Reads are 256-byte rows (one head of one token) strided by the token pitch. The pool geometry, the slots a workgroup
// owns and the 16-byte store are kv_store.h's.
#include <type_traits>

#include "kv_store.h"

namespace swl {

// grid = (ceil(max_prefill_len / bs) [+ 1 where contexts may be nonzero], num_prefill_seqs): kv_store.h, prefill_span.
// Pool = T: 16-bit pools, inv_scales is NULL. Pool = uint8_t: FP8 pools; rotary has run before (a launch of its own).
// CTX = false: every context is 0 and ctx_lens is not looked at (kv_store.h, prefill_span).
// The geometry arrives as scalars and the two pointers only some instantiations read come last: the kernel arguments
// of the plain 16-bit store then lie where they always lay.
template <typename T, typename Pool, bool CTX>
__global__ __launch_bounds__(256) void store_prefill_kernel(
    Pool *__restrict__ k_cache, Pool *__restrict__ v_cache, const T *__restrict__ k, const T *__restrict__ v,
    const int *__restrict__ block_table, const int *__restrict__ seq_ids, const int *__restrict__ start_locs,
    const int *__restrict__ seq_lens, int cur_layer, int num_layers, int KVH, int block_size, int D, int max_blocks_per_seq,
    int64_t k_tok_stride, int64_t v_tok_stride, const int *__restrict__ ctx_lens, const float *__restrict__ inv_scales) {
    const KvGeom g{cur_layer, num_layers, KVH, block_size, D, max_blocks_per_seq};
    PrefillSpan sp;
    if (!prefill_span<CTX>(sp, g, block_table, seq_ids, start_locs, seq_lens, ctx_lens)) return;
    constexpr int E = kPutElems<Pool>;
    const InvRows<Pool> inv(inv_scales, g);
    walk_tile(g, sp, g.D / E, [&](int it, int h, int, int c, int pos) {
        const int64_t dst = sp.tile + static_cast<int64_t>(it) * E;
        const int64_t col = static_cast<int64_t>(h) * g.D + c * E;
        put16<T>(k_cache + dst, k + sp.tok(pos) * k_tok_stride + col, inv.k(h));
        put16<T>(v_cache + dst, v + sp.tok(pos) * v_tok_stride + col, inv.v(h));
    });
}

// Prefill fusion: rotary on q and k (rotary_emb.py:7-42) AND the prefill KV store
// (kvcache_mgmt.py:10-48) in one pass — two launches walk k twice (rotary_kernel: read + write, then the store: read
// again). Same grid as the store: the workgroup that owns one logical block of one sequence rotates its <= 16 tokens' q
// heads in place, rotates their k heads and writes them BOTH back to k and into the contiguous [KVH, bs, D] pool tile,
// and copies v into its tile. Same arithmetic and rounding points as rotary.hip (rotate8), bit-identical stores.
// This is the form for chunks behind a context (swl_rotary_store_kv_prefill_at); the order of the kernel arguments: as
// store_prefill_kernel's.
template <typename T>
__global__ __launch_bounds__(256) void rotary_store_prefill_at_kernel(
    T *__restrict__ q, T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ cos_t, const T *__restrict__ sin_t,
    const int *__restrict__ pos_idx, T *__restrict__ k_cache, T *__restrict__ v_cache, const int *__restrict__ block_table,
    const int *__restrict__ seq_ids, const int *__restrict__ start_locs, const int *__restrict__ seq_lens, int cur_layer,
    int num_layers, int H, int KVH, int block_size, int D, int max_blocks_per_seq, int64_t q_tok_stride, int64_t k_tok_stride,
    int64_t v_tok_stride, const int *__restrict__ ctx_lens) {
    const KvGeom g{cur_layer, num_layers, KVH, block_size, D, max_blocks_per_seq};
    PrefillSpan sp;
    if (!prefill_span(sp, g, block_table, seq_ids, start_locs, seq_lens, ctx_lens)) return;
    const int half = g.D >> 1;
    const int chunks = g.D >> 4;                    // 8-element chunks in half a head
    // ---- k: rotate, write back, write into the pool tile ----
    walk_tile(g, sp, chunks, [&](int, int h, int t, int c, int pos) {
        const int64_t tok = sp.tok(pos);
        const int64_t row = pos_idx ? pos_idx[tok] : pos;
        rotate_k_item<T>(k + tok * k_tok_stride + static_cast<int64_t>(h) * g.D,
                         k_cache + sp.tile + (static_cast<int64_t>(h) * g.bs + t) * g.D, cos_t, sin_t, row, half, c);
    });
    // ---- v: copy into the pool tile ----
    walk_tile(g, sp, g.D >> 3, [&](int it, int h, int, int c, int pos) {
        put16<T>(v_cache + sp.tile + static_cast<int64_t>(it) * 8,
                 v + sp.tok(pos) * v_tok_stride + static_cast<int64_t>(h) * g.D + c * 8, 1.0f);
    });
    // ---- q: rotate in place; items ordered [t][head][chunk] ----
    const int q_items = (sp.hi - sp.lo) * H * chunks;
    for (int it = threadIdx.x; it < q_items; it += 256) {
        const int c = it % chunks;
        const int h = (it / chunks) % H;
        const int pos = sp.lo + it / (chunks * H);
        const int64_t tok = sp.tok(pos);
        const int64_t row = pos_idx ? pos_idx[tok] : pos;
        rotate_in_place<T>(q + tok * q_tok_stride + static_cast<int64_t>(h) * g.D, cos_t, sin_t, row, half, c);
    }
}

// Whole prompts (swl_rotary_store_kv_prefill): the same pass with every context 0, kept as a kernel of its own with its
// own `tok0 / ntok` prologue and item loops. Folded into the kernel above (a NULL ctx_lens, or a template flag for it) the
// bfloat16 instantiation took 62 VGPRs for 58 and ran 2 % slower on a 4096-token prompt; the item bodies are the shared ones.
template <typename T>
__global__ __launch_bounds__(256) void rotary_store_prefill_kernel(
    T *__restrict__ q, T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ cos_t, const T *__restrict__ sin_t,
    const int *__restrict__ pos_idx, T *__restrict__ k_cache, T *__restrict__ v_cache, const int *__restrict__ block_table,
    const int *__restrict__ seq_ids, const int *__restrict__ start_locs, const int *__restrict__ seq_lens, int cur_layer,
    int num_layers, int H, int KVH, int block_size, int D, int max_blocks_per_seq, int64_t q_tok_stride, int64_t k_tok_stride,
    int64_t v_tok_stride) {
    const int s = blockIdx.y;
    const int lb = blockIdx.x;
    const int len = seq_lens[s];
    const int tok0 = lb * block_size;
    if (tok0 >= len || lb >= max_blocks_per_seq) return;   // (nothing to write; never index outside the table row)
    const int ntok = min(block_size, len - tok0);
    const int64_t start = start_locs[s];
    const int seq_id = seq_ids[s];
    const KvGeom g{cur_layer, num_layers, KVH, block_size, D, max_blocks_per_seq};
    const int64_t tile = g.tile(block_table[static_cast<int64_t>(seq_id) * max_blocks_per_seq + lb]);
    const int half = D >> 1;
    const int chunks = D >> 4;                      // 8-element chunks in half a head
    // ---- k: rotate, write back, write into the pool tile; items ordered [kvh][t][chunk] ----
    const int k_items = KVH * block_size * chunks;
    for (int it = threadIdx.x; it < k_items; it += 256) {
        const int c = it % chunks;
        const int t = (it / chunks) % block_size;
        const int h = it / (chunks * block_size);
        if (t >= ntok) continue;
        const int64_t tok = start + tok0 + t;
        const int64_t row = pos_idx ? pos_idx[tok] : tok0 + t;
        rotate_k_item<T>(k + tok * k_tok_stride + static_cast<int64_t>(h) * D,
                         k_cache + tile + (static_cast<int64_t>(h) * block_size + t) * D, cos_t, sin_t, row, half, c);
    }
    // ---- v: copy into the pool tile ----
    const int cpr = D >> 3;
    const int v_items = KVH * block_size * cpr;
    for (int it = threadIdx.x; it < v_items; it += 256) {
        const int c = it % cpr;
        const int t = (it / cpr) % block_size;
        const int h = it / (cpr * block_size);
        if (t < ntok)
            store8(v_cache + tile + static_cast<int64_t>(it) * 8,
                   load8(v + (start + tok0 + t) * v_tok_stride + static_cast<int64_t>(h) * D + c * 8));
    }
    // ---- q: rotate in place; items ordered [t][head][chunk] ----
    const int q_items = ntok * H * chunks;
    for (int it = threadIdx.x; it < q_items; it += 256) {
        const int c = it % chunks;
        const int h = (it / chunks) % H;
        const int t = it / (chunks * H);
        const int64_t tok = start + tok0 + t;
        const int64_t row = pos_idx ? pos_idx[tok] : tok0 + t;
        rotate_in_place<T>(q + tok * q_tok_stride + static_cast<int64_t>(h) * D, cos_t, sin_t, row, half, c);
    }
}

// grid = (num_decoding_seqs)
template <typename T, typename Pool>
__global__ __launch_bounds__(128) void store_decode_kernel(
    Pool *__restrict__ k_cache, Pool *__restrict__ v_cache, const T *__restrict__ k, const T *__restrict__ v,
    const float *__restrict__ inv_scales, const int *__restrict__ block_table, const int *__restrict__ seq_ids,
    const int *__restrict__ seq_lens, KvGeom g, int64_t k_tok_stride, int64_t v_tok_stride) {
    const int64_t i = blockIdx.x;
    DecodeSlot ds;
    if (!decode_slot(ds, g, block_table, seq_ids, seq_lens, i)) return;
    constexpr int E = kPutElems<Pool>;
    const InvRows<Pool> inv(inv_scales, g);
    const int cpr = g.D / E;
    for (int it = threadIdx.x; it < g.KVH * cpr; it += 128) {
        const int c = it % cpr;
        const int h = it / cpr;
        const int64_t dst = ds.base + h * g.head_pitch() + c * E;
        const int64_t col = static_cast<int64_t>(h) * g.D + c * E;
        put16<T>(k_cache + dst, k + i * k_tok_stride + col, inv.k(h));
        put16<T>(v_cache + dst, v + i * v_tok_stride + col, inv.v(h));
    }
}

// ---- launches: the grid, the block size and the casts of each kernel ------------------------------------------------------

// `spill`: contexts may be nonzero, so a chunk may end one block further than its length alone says
static dim3 prefill_grid(const KvStoreArgs &a, bool spill) {
    return dim3((a.max_len + a.g.bs - 1) / a.g.bs + (spill ? 1 : 0), static_cast<unsigned>(a.num_seqs));
}

// CTX = false: the plain entry — no contexts, no spill column
template <bool Fp8Pools, bool CTX>
static int launch_store_prefill(const KvStoreArgs &a, int dtype, swl_stream_t stream) {
    SWL_DISPATCH_DTYPE(dtype, T, {
        using P = std::conditional_t<Fp8Pools, uint8_t, T>;
        hipLaunchKernelGGL((store_prefill_kernel<T, P, CTX>), prefill_grid(a, CTX), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<P *>(a.k_cache), static_cast<P *>(a.v_cache),
                           static_cast<const T *>(a.k), static_cast<const T *>(a.v), a.block_table, a.seq_ids, a.start_locs,
                           a.seq_lens, a.g.layer, a.g.L, a.g.KVH, a.g.bs, a.g.D, a.g.mbps, a.k_tok_stride, a.v_tok_stride,
                           a.ctx_lens, a.inv_scales);
    });
    return check_launch();
}

// the two fused prefill kernels share their argument list up to ctx_lens, which only the `_at` kernel has
#define SWL_ROTARY_STORE_PREFILL_ARGS(T, a)                                                                                  \
    static_cast<T *>(a.q), static_cast<T *>(a.k), static_cast<const T *>(a.v), static_cast<const T *>(a.cos_table),          \
        static_cast<const T *>(a.sin_table), a.pos_idx, static_cast<T *>(a.k_cache), static_cast<T *>(a.v_cache),            \
        a.block_table, a.seq_ids, a.start_locs, a.seq_lens, a.g.layer, a.g.L, a.H, a.g.KVH, a.g.bs, a.g.D, a.g.mbps,         \
        a.q_tok_stride, a.k_tok_stride, a.v_tok_stride

template <bool CTX>
static int launch_rotary_store_prefill(const KvStoreArgs &a, int dtype, swl_stream_t stream) {
    SWL_DISPATCH_DTYPE(dtype, T, {
        if constexpr (CTX)
            hipLaunchKernelGGL((rotary_store_prefill_at_kernel<T>), prefill_grid(a, true), dim3(256), 0,
                               static_cast<hipStream_t>(stream), SWL_ROTARY_STORE_PREFILL_ARGS(T, a), a.ctx_lens);
        else
            hipLaunchKernelGGL((rotary_store_prefill_kernel<T>), prefill_grid(a, false), dim3(256), 0,
                               static_cast<hipStream_t>(stream), SWL_ROTARY_STORE_PREFILL_ARGS(T, a));
    });
    return check_launch();
}

template <bool Fp8Pools>
static int launch_store_decode(const KvStoreArgs &a, int dtype, swl_stream_t stream) {
    SWL_DISPATCH_DTYPE(dtype, T, {
        using P = std::conditional_t<Fp8Pools, uint8_t, T>;
        hipLaunchKernelGGL((store_decode_kernel<T, P>), dim3(static_cast<unsigned>(a.num_seqs)), dim3(128), 0,
                           static_cast<hipStream_t>(stream), static_cast<P *>(a.k_cache), static_cast<P *>(a.v_cache),
                           static_cast<const T *>(a.k), static_cast<const T *>(a.v), a.inv_scales, a.block_table, a.seq_ids,
                           a.seq_lens, a.g, a.k_tok_stride, a.v_tok_stride);
    });
    return check_launch();
}

// the checks of the rotary + store entries that follow the store's own: the rotary operands are there ...
static int check_rotary_present(const KvStoreArgs &a) { return check_present({a.q, a.cos_table, a.sin_table}); }
// ... and the q rows fit their pitch, 16-byte alignment
static int check_rotary_operands(const KvStoreArgs &a) {
    SWL_KV_CHECK(check_tok_stride(a, a.q_tok_stride, a.H));
    return check_aligned16({a.q, a.cos_table, a.sin_table});
}

} // namespace swl

using swl::KvStoreArgs;

static KvStoreArgs store_args(void *k_cache, void *v_cache, const void *k, const void *v, const float *inv_scales,
                              const int32_t *block_table, const int32_t *seq_ids, const int32_t *start_locs,
                              const int32_t *seq_lens, const int32_t *ctx_lens, int32_t num_seqs, int32_t max_len,
                              int32_t cur_layer, int32_t num_layers, int32_t num_kv_heads, int32_t block_size,
                              int32_t head_dim, int32_t max_blocks_per_seq, int64_t k_tok_stride, int64_t v_tok_stride) {
    KvStoreArgs a;
    a.k_cache = k_cache, a.v_cache = v_cache, a.k = const_cast<void *>(k), a.v = const_cast<void *>(v);
    a.inv_scales = inv_scales;
    a.block_table = block_table, a.seq_ids = seq_ids, a.start_locs = start_locs, a.seq_lens = seq_lens, a.ctx_lens = ctx_lens;
    a.num_seqs = num_seqs, a.max_len = max_len;
    a.g = {cur_layer, num_layers, num_kv_heads, block_size, head_dim, max_blocks_per_seq};
    a.k_tok_stride = k_tok_stride, a.v_tok_stride = v_tok_stride;
    return a;
}

static KvStoreArgs rotary_store_args(void *q, const void *cos_table, const void *sin_table, const int32_t *pos_idx,
                                     int32_t num_q_heads, int64_t q_tok_stride, KvStoreArgs a) {
    a.q = q, a.cos_table = cos_table, a.sin_table = sin_table, a.pos_idx = pos_idx;
    a.H = num_q_heads, a.q_tok_stride = q_tok_stride;
    return a;
}

extern "C" int swl_store_kv_prefill(void *k_cache, void *v_cache, const void *k, const void *v, const int32_t *block_table,
    const int32_t *seq_ids, const int32_t *start_locs, const int32_t *seq_lens, int32_t num_prefill_seqs,
    int32_t max_prefill_len, int32_t cur_layer, int32_t num_layers, int32_t num_kv_heads, int32_t block_size,
    int32_t head_dim, int32_t max_blocks_per_seq, int64_t k_tok_stride, int64_t v_tok_stride, int32_t dtype,
    swl_stream_t stream) {
    const KvStoreArgs a = store_args(k_cache, v_cache, k, v, nullptr, block_table, seq_ids, start_locs, seq_lens, nullptr,
                                     num_prefill_seqs, max_prefill_len, cur_layer, num_layers, num_kv_heads, block_size,
                                     head_dim, max_blocks_per_seq, k_tok_stride, v_tok_stride);
    SWL_KV_CHECK(swl::check_kv_counts(a));
    if (a.empty()) return SWL_OK;
    SWL_KV_CHECK(swl::check_store_operands(a, 8));
    SWL_KV_CHECK(swl::check_present({start_locs}));
    SWL_KV_CHECK(swl::check_prefill_grid(a));
    return swl::launch_store_prefill<false, false>(a, dtype, stream);
}

extern "C" int swl_rotary_store_kv_prefill(void *q, void *k, const void *v, const void *cos_table, const void *sin_table,
                                           const int32_t *pos_idx, void *k_cache, void *v_cache, const int32_t *block_table,
                                           const int32_t *seq_ids, const int32_t *start_locs, const int32_t *seq_lens,
                                           int32_t num_prefill_seqs, int32_t max_prefill_len, int32_t cur_layer,
                                           int32_t num_layers, int32_t num_q_heads, int32_t num_kv_heads, int32_t block_size,
                                           int32_t head_dim, int32_t max_blocks_per_seq, int64_t q_tok_stride,
                                           int64_t k_tok_stride, int64_t v_tok_stride, int32_t dtype, swl_stream_t stream) {
    const KvStoreArgs a = rotary_store_args(
        q, cos_table, sin_table, pos_idx, num_q_heads, q_tok_stride,
        store_args(k_cache, v_cache, k, v, nullptr, block_table, seq_ids, start_locs, seq_lens, nullptr, num_prefill_seqs,
                   max_prefill_len, cur_layer, num_layers, num_kv_heads, block_size, head_dim, max_blocks_per_seq,
                   k_tok_stride, v_tok_stride));
    SWL_KV_CHECK(swl::check_kv_counts(a));
    if (a.empty()) return SWL_OK;
    SWL_KV_CHECK(swl::check_store_operands(a, 8));
    SWL_KV_CHECK(swl::check_present({start_locs}));
    SWL_KV_CHECK(swl::check_rotary_present(a));
    SWL_KV_CHECK(swl::check_head_dim_rotary(a, SWL_ERR_UNSUPPORTED));
    SWL_KV_CHECK(swl::check_rotary_operands(a));
    SWL_KV_CHECK(swl::check_prefill_grid(a));
    return swl::launch_rotary_store_prefill<false>(a, dtype, stream);
}

// The _at entries: as their twins above plus ctx_lens (int32 [Bp]); a head_dim the kernels are not built for is
// SWL_ERR_UNSUPPORTED here, ahead of everything else (the twins report it as a bad argument, or later).
extern "C" int swl_store_kv_prefill_at(void *k_cache, void *v_cache, const void *k, const void *v,
                                       const int32_t *block_table, const int32_t *seq_ids, const int32_t *start_locs,
                                       const int32_t *seq_lens, const int32_t *ctx_lens, int32_t num_prefill_seqs,
                                       int32_t max_prefill_len, int32_t cur_layer, int32_t num_layers,
                                       int32_t num_kv_heads, int32_t block_size, int32_t head_dim,
                                       int32_t max_blocks_per_seq, int64_t k_tok_stride, int64_t v_tok_stride,
                                       int32_t dtype, swl_stream_t stream) {
    const KvStoreArgs a = store_args(k_cache, v_cache, k, v, nullptr, block_table, seq_ids, start_locs, seq_lens, ctx_lens,
                                     num_prefill_seqs, max_prefill_len, cur_layer, num_layers, num_kv_heads, block_size,
                                     head_dim, max_blocks_per_seq, k_tok_stride, v_tok_stride);
    SWL_KV_CHECK(swl::check_kv_counts(a));
    if (a.empty()) return SWL_OK;
    SWL_KV_CHECK(swl::check_head_dim_chunks(a, 8, SWL_ERR_UNSUPPORTED));
    SWL_KV_CHECK(swl::check_store_operands(a, 8));
    SWL_KV_CHECK(swl::check_present({start_locs, ctx_lens}));
    SWL_KV_CHECK(swl::check_prefill_grid(a));
    return swl::launch_store_prefill<false, true>(a, dtype, stream);
}

extern "C" int swl_rotary_store_kv_prefill_at(void *q, void *k, const void *v, const void *cos_table, const void *sin_table,
                                              const int32_t *pos_idx, void *k_cache, void *v_cache,
                                              const int32_t *block_table, const int32_t *seq_ids,
                                              const int32_t *start_locs, const int32_t *seq_lens, const int32_t *ctx_lens,
                                              int32_t num_prefill_seqs, int32_t max_prefill_len, int32_t cur_layer,
                                              int32_t num_layers, int32_t num_q_heads, int32_t num_kv_heads,
                                              int32_t block_size, int32_t head_dim, int32_t max_blocks_per_seq,
                                              int64_t q_tok_stride, int64_t k_tok_stride, int64_t v_tok_stride,
                                              int32_t dtype, swl_stream_t stream) {
    const KvStoreArgs a = rotary_store_args(
        q, cos_table, sin_table, pos_idx, num_q_heads, q_tok_stride,
        store_args(k_cache, v_cache, k, v, nullptr, block_table, seq_ids, start_locs, seq_lens, ctx_lens, num_prefill_seqs,
                   max_prefill_len, cur_layer, num_layers, num_kv_heads, block_size, head_dim, max_blocks_per_seq,
                   k_tok_stride, v_tok_stride));
    SWL_KV_CHECK(swl::check_kv_counts(a));
    if (a.empty()) return SWL_OK;
    SWL_KV_CHECK(swl::check_head_dim_rotary(a, SWL_ERR_UNSUPPORTED));
    SWL_KV_CHECK(swl::check_store_operands(a, 8));
    SWL_KV_CHECK(swl::check_present({start_locs, ctx_lens}));
    SWL_KV_CHECK(swl::check_rotary_present(a));
    SWL_KV_CHECK(swl::check_rotary_operands(a));
    SWL_KV_CHECK(swl::check_prefill_grid(a));
    return swl::launch_rotary_store_prefill<true>(a, dtype, stream);
}

extern "C" int swl_store_kv_decode(void *k_cache, void *v_cache, const void *k, const void *v, const int32_t *block_table,
    const int32_t *seq_ids, const int32_t *seq_lens, int32_t num_decoding_seqs, int32_t cur_layer, int32_t num_layers,
    int32_t num_kv_heads, int32_t block_size, int32_t head_dim, int32_t max_blocks_per_seq, int64_t k_tok_stride,
    int64_t v_tok_stride, int32_t dtype, swl_stream_t stream) {
    const KvStoreArgs a = store_args(k_cache, v_cache, k, v, nullptr, block_table, seq_ids, nullptr, seq_lens, nullptr,
                                     num_decoding_seqs, 1, cur_layer, num_layers, num_kv_heads, block_size, head_dim,
                                     max_blocks_per_seq, k_tok_stride, v_tok_stride);
    SWL_KV_CHECK(swl::check_kv_counts(a));
    if (a.empty()) return SWL_OK;
    SWL_KV_CHECK(swl::check_store_operands(a, 8));
    return swl::launch_store_decode<false>(a, dtype, stream);
}

// ---- FP8 (e4m3fn) pools: the pools are bytes, an item is 16 elements; ctx_lens == NULL: every context is 0 ----------------
extern "C" int swl_store_kv_prefill_at_fp8(void *k_cache, void *v_cache, const void *k, const void *v,
                                           const float *inv_scales, const int32_t *block_table, const int32_t *seq_ids,
                                           const int32_t *start_locs, const int32_t *seq_lens, const int32_t *ctx_lens,
                                           int32_t num_prefill_seqs, int32_t max_prefill_len, int32_t cur_layer,
                                           int32_t num_layers, int32_t num_kv_heads, int32_t block_size, int32_t head_dim,
                                           int32_t max_blocks_per_seq, int64_t k_tok_stride, int64_t v_tok_stride,
                                           int32_t dtype, swl_stream_t stream) {
    const KvStoreArgs a = store_args(k_cache, v_cache, k, v, inv_scales, block_table, seq_ids, start_locs, seq_lens, ctx_lens,
                                     num_prefill_seqs, max_prefill_len, cur_layer, num_layers, num_kv_heads, block_size,
                                     head_dim, max_blocks_per_seq, k_tok_stride, v_tok_stride);
    SWL_KV_CHECK(swl::check_kv_counts(a));
    if (a.empty()) return SWL_OK;
    SWL_KV_CHECK(swl::check_store_operands(a, 16));
    SWL_KV_CHECK(swl::check_present({inv_scales, start_locs}));
    SWL_KV_CHECK(swl::check_prefill_grid(a));
    return swl::launch_store_prefill<true, true>(a, dtype, stream);
}

extern "C" int swl_store_kv_decode_fp8(void *k_cache, void *v_cache, const void *k, const void *v, const float *inv_scales,
                                       const int32_t *block_table, const int32_t *seq_ids, const int32_t *seq_lens,
                                       int32_t num_decoding_seqs, int32_t cur_layer, int32_t num_layers,
                                       int32_t num_kv_heads, int32_t block_size, int32_t head_dim,
                                       int32_t max_blocks_per_seq, int64_t k_tok_stride, int64_t v_tok_stride,
                                       int32_t dtype, swl_stream_t stream) {
    const KvStoreArgs a = store_args(k_cache, v_cache, k, v, inv_scales, block_table, seq_ids, nullptr, seq_lens, nullptr,
                                     num_decoding_seqs, 1, cur_layer, num_layers, num_kv_heads, block_size, head_dim,
                                     max_blocks_per_seq, k_tok_stride, v_tok_stride);
    SWL_KV_CHECK(swl::check_kv_counts(a));
    if (a.empty()) return SWL_OK;
    SWL_KV_CHECK(swl::check_store_operands(a, 16));
    SWL_KV_CHECK(swl::check_present({inv_scales}));
    return swl::launch_store_decode<true>(a, dtype, stream);
}
