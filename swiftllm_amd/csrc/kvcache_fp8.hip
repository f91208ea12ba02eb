// kvcache_fp8.hip — quantising stores into the FP8 (e4m3fn) KV pools (gfx950). Contract: fp8_kv.h.
//
// The twins of store_kv_prefill_at_kernel / store_kv_decode_kernel (kvcache.hip) for pools of 1-byte elements: same
// grids, same ownership of slots, but an item is 16 ELEMENTS — two 16-byte reads of the 16-bit projection, one 16-byte
// store into the 2 KiB (at D = 128) tile. Every element is fp32(x) * inv_scale[layer, kv-head], clamped to +-448 and
// rounded to nearest even by v_cvt_pk_fp8_f32; the bytes equal the host expression in fp8_kv.h. Rotary has run before
// (a launch of its own in FP8 mode).
#include "fp8_kv.h"

namespace swl {

// grid = (ceil(max_prefill_len / bs) + 1, num_prefill_seqs); ctx_lens == NULL: every context is 0 (whole prompts)
template <typename T>
__global__ __launch_bounds__(256) void store_kv_prefill_at_fp8_kernel(
    uint8_t *__restrict__ k_cache, uint8_t *__restrict__ v_cache, const T *__restrict__ k, const T *__restrict__ v,
    const float *__restrict__ inv_scales, const int *__restrict__ block_table, const int *__restrict__ seq_ids,
    const int *__restrict__ start_locs, const int *__restrict__ seq_lens, const int *__restrict__ ctx_lens, int cur_layer,
    int num_layers, int KVH, int block_size, int D, int max_blocks_per_seq, int64_t k_tok_stride, int64_t v_tok_stride) {
    const int s = blockIdx.y;
    const int ctx = ctx_lens ? ctx_lens[s] : 0;
    const int len = seq_lens[s];
    const int lb = ctx / block_size + blockIdx.x; // logical block inside the sequence
    const int pos0 = lb * block_size;
    const int lo = max(pos0, ctx), hi = min(pos0 + block_size, ctx + len);   // positions of this block the chunk owns
    if (lo >= hi || ctx < 0 || lb >= max_blocks_per_seq) return;   // (nothing to write; never index outside the table row)
    const int64_t start = start_locs[s];
    const int seq_id = seq_ids[s];
    const int64_t blk = block_table[static_cast<int64_t>(seq_id) * max_blocks_per_seq + lb];
    const int64_t tile = (blk * num_layers + cur_layer) * KVH * static_cast<int64_t>(block_size) * D;   // bytes
    const float *k_inv = inv_scales + static_cast<int64_t>(cur_layer) * KVH;
    const float *v_inv = k_inv + static_cast<int64_t>(num_layers) * KVH;

    const int cpr = D >> 4;                    // 16-element chunks per (token, head) row
    const int items = KVH * block_size * cpr;  // destination order: [kvh][slot][chunk] == contiguous
    for (int it = threadIdx.x; it < items; it += 256) {
        const int c = it % cpr;
        const int t = (it / cpr) % block_size;
        const int h = it / (cpr * block_size);
        const int pos = pos0 + t;
        if (pos >= lo && pos < hi) {
            const int64_t tok = start + (pos - ctx);
            const int64_t dst = tile + static_cast<int64_t>(it) * 16;
            const T *ks = k + tok * k_tok_stride + static_cast<int64_t>(h) * D + c * 16;
            const T *vs = v + tok * v_tok_stride + static_cast<int64_t>(h) * D + c * 16;
            *reinterpret_cast<u32x4_t *>(k_cache + dst) = quantise16<T>(load8(ks), load8(ks + 8), k_inv[h]);
            *reinterpret_cast<u32x4_t *>(v_cache + dst) = quantise16<T>(load8(vs), load8(vs + 8), v_inv[h]);
        }
    }
}

// grid = (num_decoding_seqs)
template <typename T>
__global__ __launch_bounds__(128) void store_kv_decode_fp8_kernel(
    uint8_t *__restrict__ k_cache, uint8_t *__restrict__ v_cache, const T *__restrict__ k, const T *__restrict__ v,
    const float *__restrict__ inv_scales, const int *__restrict__ block_table, const int *__restrict__ seq_ids,
    const int *__restrict__ seq_lens, int cur_layer, int num_layers, int KVH, int block_size, int D, int max_blocks_per_seq,
    int64_t k_tok_stride, int64_t v_tok_stride) {
    const int64_t i = blockIdx.x;
    const int seq_id = seq_ids[i];
    const int pos = seq_lens[i] - 1;
    if (pos < 0) return; // an inert row of a padded decode batch (length 0)
    const int64_t blk = block_table[static_cast<int64_t>(seq_id) * max_blocks_per_seq + pos / block_size];
    const int slot = pos % block_size;
    const int64_t base = (blk * num_layers + cur_layer) * KVH * static_cast<int64_t>(block_size) * D +
                         static_cast<int64_t>(slot) * D;   // bytes
    const float *k_inv = inv_scales + static_cast<int64_t>(cur_layer) * KVH;
    const float *v_inv = k_inv + static_cast<int64_t>(num_layers) * KVH;
    const int cpr = D >> 4;
    for (int it = threadIdx.x; it < KVH * cpr; it += 128) {
        const int c = it % cpr;
        const int h = it / cpr;
        const int64_t dst = base + static_cast<int64_t>(h) * block_size * D + c * 16;
        const T *ks = k + i * k_tok_stride + static_cast<int64_t>(h) * D + c * 16;
        const T *vs = v + i * v_tok_stride + static_cast<int64_t>(h) * D + c * 16;
        *reinterpret_cast<u32x4_t *>(k_cache + dst) = quantise16<T>(load8(ks), load8(ks + 8), k_inv[h]);
        *reinterpret_cast<u32x4_t *>(v_cache + dst) = quantise16<T>(load8(vs), load8(vs + 8), v_inv[h]);
    }
}

} // namespace swl

static int store_fp8_args(const void *kc, const void *vc, const void *k, const void *v, const void *inv, const void *bt,
                          const void *ids, const void *lens, int cur_layer, int L, int KVH, int bs, int D, int mbps,
                          int64_t ks, int64_t vs) {
    if (!kc || !vc || !k || !v || !inv || !bt || !ids || !lens) return SWL_ERR_BAD_ARG;
    if (L <= 0 || cur_layer < 0 || cur_layer >= L || KVH <= 0 || bs <= 0 || D <= 0 || mbps <= 0) return SWL_ERR_BAD_ARG;
    if (D & 15) return SWL_ERR_BAD_ARG;        // an item is 16 elements = one 16-byte store
    if (ks < static_cast<int64_t>(KVH) * D || vs < static_cast<int64_t>(KVH) * D || (ks & 7) || (vs & 7))
        return SWL_ERR_BAD_ARG;
    if (!(swl::aligned16(kc) && swl::aligned16(vc) && swl::aligned16(k) && swl::aligned16(v))) return SWL_ERR_BAD_ARG;
    return SWL_OK;
}

extern "C" int swl_store_kv_prefill_at_fp8(void *k_cache, void *v_cache, const void *k, const void *v,
                                           const float *inv_scales, const int32_t *block_table, const int32_t *seq_ids,
                                           const int32_t *start_locs, const int32_t *seq_lens, const int32_t *ctx_lens,
                                           int32_t num_prefill_seqs, int32_t max_prefill_len, int32_t cur_layer,
                                           int32_t num_layers, int32_t num_kv_heads, int32_t block_size, int32_t head_dim,
                                           int32_t max_blocks_per_seq, int64_t k_tok_stride, int64_t v_tok_stride,
                                           int32_t dtype, swl_stream_t stream) {
    if (num_prefill_seqs < 0 || max_prefill_len < 0) return SWL_ERR_BAD_ARG;
    if (num_prefill_seqs == 0 || max_prefill_len == 0) return SWL_OK;
    const int rc = store_fp8_args(k_cache, v_cache, k, v, inv_scales, block_table, seq_ids, seq_lens, cur_layer, num_layers,
                                  num_kv_heads, block_size, head_dim, max_blocks_per_seq, k_tok_stride, v_tok_stride);
    if (rc != SWL_OK) return rc;
    if (!start_locs) return SWL_ERR_BAD_ARG;
    if (num_prefill_seqs > 65535) return SWL_ERR_UNSUPPORTED;
    const dim3 grid((max_prefill_len + block_size - 1) / block_size + 1, num_prefill_seqs);
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::store_kv_prefill_at_fp8_kernel<T>), grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<uint8_t *>(k_cache), static_cast<uint8_t *>(v_cache), static_cast<const T *>(k),
                           static_cast<const T *>(v), inv_scales, block_table, seq_ids, start_locs, seq_lens, ctx_lens,
                           cur_layer, num_layers, num_kv_heads, block_size, head_dim, max_blocks_per_seq, k_tok_stride,
                           v_tok_stride);
    });
    return swl::check_launch();
}

extern "C" int swl_store_kv_decode_fp8(void *k_cache, void *v_cache, const void *k, const void *v, const float *inv_scales,
                                       const int32_t *block_table, const int32_t *seq_ids, const int32_t *seq_lens,
                                       int32_t num_decoding_seqs, int32_t cur_layer, int32_t num_layers,
                                       int32_t num_kv_heads, int32_t block_size, int32_t head_dim,
                                       int32_t max_blocks_per_seq, int64_t k_tok_stride, int64_t v_tok_stride,
                                       int32_t dtype, swl_stream_t stream) {
    if (num_decoding_seqs < 0) return SWL_ERR_BAD_ARG;
    if (num_decoding_seqs == 0) return SWL_OK;
    const int rc = store_fp8_args(k_cache, v_cache, k, v, inv_scales, block_table, seq_ids, seq_lens, cur_layer, num_layers,
                                  num_kv_heads, block_size, head_dim, max_blocks_per_seq, k_tok_stride, v_tok_stride);
    if (rc != SWL_OK) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::store_kv_decode_fp8_kernel<T>), dim3(num_decoding_seqs), dim3(128), 0,
                           static_cast<hipStream_t>(stream), static_cast<uint8_t *>(k_cache),
                           static_cast<uint8_t *>(v_cache), static_cast<const T *>(k), static_cast<const T *>(v), inv_scales,
                           block_table, seq_ids, seq_lens, cur_layer, num_layers, num_kv_heads, block_size, head_dim,
                           max_blocks_per_seq, k_tok_stride, v_tok_stride);
    });
    return swl::check_launch();
}
