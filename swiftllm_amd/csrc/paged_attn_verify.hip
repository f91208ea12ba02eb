// paged_attn_verify.hip — paged attention for a speculative-decoding VERIFY step on gfx950 (an addition, no reference
// counterpart): every sequence brings n <= 16/G new tokens (its last accepted token and its drafts) behind c resident
// ones; row i attends keys j <= c + i. The semantics are swl_prefill_attn_paged's (prefill_attn_paged.hip), the
// arithmetic is the decode kernel's (paged_attn.hip, plain-q matrix-core path):
//   * grid (split, kv-head, sequence), 4 or 8 waves, register K/V ring of depth 2 and the merge of the waves
//     (decode_attn.h, the decode kernel's own), attend_block_mfma (attn_mfma.h);
//   * the decode kernel carries the G q-heads of a kv-head as the N columns of its 16 x 16 MFMA tiles and leaves
//     columns >= G zero. Here (token t, head g) sits at column t*G + g: up to 16/G tokens are verified for the KV
//     bytes and the MFMA issues of one. G = 1 uses the same path (16 columns = 16 tokens);
//   * the key limit is per lane (c + t + 1 for the lane's column); the masked body runs only in blocks with
//     tok0 + 16 > c + 1 — at most two per sequence — every earlier block runs the unmasked body;
//   * columns with t >= n carry zero q and are never written; a (row, split) without a visible key writes nothing
//     (phase 2 reads ceil(row_len / seq_block_size) partials of a row: exactly the splits that have one);
//   * K/V rows at positions >= c + n are staged as zeros (a masked p = 0 times a NaN V is NaN), rows in (c + i, c + n)
//     are the finite rows the preceding store wrote and their scores get kNegBig;
//   * phase 2 is paged_attn_phase2_kernel with every ROW as a "sequence" of length row_lens[r] = position + 1.
// The new tokens' rotary + store stay a launch of their own before this one (swl_rotary_store_kv_prefill_at).
#include "decode_attn.h"

namespace swl {

constexpr int kVerifyCols = 16; // N columns of the MFMA tile = (token, head) pairs per kv-head
constexpr int kVerifyDepth = 2; // K/V register ring, as the decode kernel's matrix-core path (kPaMfmaDepth)

// block_table / seq_ids / cu_seqlens / ctx_lens are __restrict__ kernel arguments so block ids stay scalar loads
// (see paged_attn_phase1_kernel).
template <typename T, int D, int G, int NW>
__global__ __launch_bounds__(NW * 64) void paged_attn_verify_kernel(DecodeAttnParams p,
                                                                    const int *__restrict__ block_table,
                                                                    const int *__restrict__ seq_ids_r,
                                                                    const int *__restrict__ cu_r,
                                                                    const int *__restrict__ ctx_r) {
    using Tile = DecodeTile<T, D, G>;
    using MT = MfmaTile<T, D>;
    constexpr int LPT = Tile::LPT, TPI = Tile::TPI, NI = Tile::NI;
    constexpr int C = kVerifyCols, TMAX = C / G, ND = kVerifyDepth;
    __shared__ float sm_ml[NW][C][2];
    __shared__ float sm_acc[NW][C][D];
    __shared__ __attribute__((aligned(16))) T sm_stage[NW][MT::ELEMS];

    const int split = blockIdx.x;
    const int kvh = blockIdx.y;
    const int seq = blockIdx.z;
    const int ctx = ctx_r[seq];
    const int row0 = cu_r[seq];
    const int n = min(cu_r[seq + 1] - row0, TMAX);
    if (n <= 0) return; // uniform for the workgroup, before any barrier
    const int total = ctx + n;
    const int tok_begin = split * p.seq_block_size;
    if (tok_begin >= total) return;
    const int tok_end = min(total, tok_begin + p.seq_block_size);
    const int blk_end = min((tok_end + kBlk - 1) / kBlk, p.max_blocks_per_seq); // never index past the table row
    const int seq_id = seq_ids_r[seq];
    const int *__restrict__ bt = block_table + static_cast<int64_t>(seq_id) * p.max_blocks_per_seq;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = lane % LPT;
    const int row = lane / LPT;
    const float c = p.scale_log2e;

    const T *kc = static_cast<const T *>(p.k_cache);
    const T *vc = static_cast<const T *>(p.v_cache);
    const int64_t tile_elems = static_cast<int64_t>(kBlk) * D;
    const int64_t layer_head = static_cast<int64_t>(p.layer) * p.KVH + kvh;
    const int64_t blk_pitch = static_cast<int64_t>(p.L) * p.KVH;

    // Q^T B fragments: lane (mq, mh) -> Q[token mh / G][head mh % G][32 j + 8 mq ..], zero for columns of tokens >= n
    const int mq = lane >> 4, mh = lane & 15;
    const int col_t = mh / G, col_g = mh % G;
    vec8_t<T> qb[MT::QS];
    {
        const T *qp = static_cast<const T *>(p.q) + static_cast<int64_t>(row0 + min(col_t, n - 1)) * p.q_tok_stride +
                      (static_cast<int64_t>(kvh) * G + col_g) * D + 8 * mq;
#pragma unroll
        for (int j = 0; j < MT::QS; ++j) {
            qb[j] = load8(qp + 32 * j);
            if (col_t >= n) qb[j] = vec8_t<T>{};
        }
    }
    // keys this lane's column may see: j < lim (an idle column gets the last real row's limit; it is never written)
    const int lim = ctx + min(col_t, n - 1) + 1;

    float m = kNegBig, l = 0.f;
    float4_t acc4[MT::OS]; // O^T[d = 16 mm + 4 mq + r][column mh]
#pragma unroll
    for (int mm = 0; mm < MT::OS; ++mm) acc4[mm] = float4_t{0.f, 0.f, 0.f, 0.f};

    vec8_t<T> Kr[ND][NI], Vr[ND][NI];
    auto load_phys = [&](int64_t phys, vec8_t<T>(&Kd)[NI], vec8_t<T>(&Vd)[NI]) {
        const int64_t base = (phys * blk_pitch + layer_head) * tile_elems + lane * 8;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            Kd[i] = load8_nt(kc + base + i * 512);
            Vd[i] = load8_nt(vc + base + i * 512);
        }
    };
    auto attend = [&](int b, vec8_t<T>(&Kd)[NI], vec8_t<T>(&Vd)[NI]) {
        const int tok0 = b * kBlk;
        const bool masked = tok0 + kBlk > ctx + 1; // wave-uniform: some column does not see the whole block
        if (masked) {
            // slots past the sequence's new tokens hold whatever an earlier owner left (NaN included): staged as zeros
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (tok0 + i * TPI + row >= total) {
                    Kd[i] = vec8_t<T>{};
                    Vd[i] = vec8_t<T>{};
                }
        }
        attend_block_mfma<T, D, G>(qb, Kd, Vd, m, l, acc4, &sm_stage[wave][0], c, tok0, row, chunk, lane, lim, masked);
    };

    const int b = tok_begin / kBlk + wave;
    kv_ring_prefetch<0, ND, NW>(b, blk_end, bt, Kr, Vr, load_phys);
    kv_ring_stream<ND, NW>(b, blk_end, bt, Kr, Vr, load_phys, attend, attend);
    mfma_wave_finish(m, l, acc4, sm_ml, sm_acc, wave, lane);
    __syncthreads();

    // merge the waves and write the real columns that saw a key in this split
    for (int oidx = threadIdx.x; oidx < C * D; oidx += NW * 64) {
        const int col = oidx / D;
        const int t = col / G;
        if (t >= n || ctx + t + 1 <= tok_begin) continue; // idle column / no visible key: contributes nothing
        merge_waves_elem<T, D, NW, C, false>(p, sm_ml, sm_acc, c, 1.0f, col, oidx % D, row0 + t, kvh * G + col % G,
                                             split);
    }
}

template <typename T>
static int launch_verify(const DecodeAttnParams &p, const int *bt, const int *seq_ids, const int *cu, const int *ctx,
                         int num_seqs, int D, hipStream_t stream) {
    return dispatch_decode_attn(D, p.H / p.KVH, p.seq_block_size, [&](auto d, auto g, auto nw) {
        constexpr int NW = decltype(nw)::value;
        hipLaunchKernelGGL((paged_attn_verify_kernel<T, decltype(d)::value, decltype(g)::value, NW>),
                           dim3(p.num_seq_blocks, p.KVH, num_seqs), dim3(NW * 64), 0, stream, p, bt, seq_ids, cu, ctx);
        return check_launch();
    });
}

} // namespace swl

extern "C" int swl_paged_attn_verify_max_tokens(int32_t num_q_heads, int32_t num_kv_heads) {
    if (num_q_heads <= 0 || num_kv_heads <= 0 || num_q_heads % num_kv_heads != 0) return 0;
    const int G = num_q_heads / num_kv_heads;
    return (G == 1 || G == 2 || G == 4 || G == 8) ? swl::kVerifyCols / G : 0;
}

extern "C" int swl_paged_attn_verify(void *o, const void *q, const void *k_cache, const void *v_cache,
                                     const int32_t *block_table, const int32_t *seq_ids, const int32_t *cu_seqlens,
                                     const int32_t *ctx_lens, const int32_t *row_lens, void *scratch,
                                     float softmax_scale, int32_t num_seqs, int32_t num_rows, int32_t max_new_len,
                                     int32_t max_total_len, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                                     int32_t num_layers, int32_t block_size, int32_t cur_layer,
                                     int32_t max_blocks_per_seq, int32_t seq_block_size, int32_t num_seq_blocks,
                                     int64_t q_tok_stride, int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    if (num_seqs < 0 || num_rows < 0) return SWL_ERR_BAD_ARG;
    if (num_seqs == 0 || num_rows == 0) return SWL_OK;
    if (!o || !q || !k_cache || !v_cache || !block_table || !seq_ids || !cu_seqlens || !ctx_lens || !row_lens)
        return SWL_ERR_BAD_ARG;
    if (head_dim <= 0 || max_new_len <= 0 || max_total_len < max_new_len || num_seq_blocks <= 0) return SWL_ERR_BAD_ARG;
    const swl::DecodeAttnArgs a{o, q, k_cache, v_cache, q_tok_stride, o_tok_stride, num_q_heads, num_kv_heads, head_dim,
                                num_layers, block_size, cur_layer, max_blocks_per_seq, seq_block_size, num_seq_blocks};
    if (const int rc = swl::check_decode_geometry(a)) return rc;
    // what this entry has no kernel for is refused before the layout is looked at
    if (!(head_dim == 32 || head_dim == 64 || head_dim == 128)) return SWL_ERR_UNSUPPORTED;
    const int tmax = swl_paged_attn_verify_max_tokens(num_q_heads, num_kv_heads);
    if (tmax == 0 || max_new_len > tmax) return SWL_ERR_UNSUPPORTED;
    if (!swl::decode_grid_fits(num_seqs, num_kv_heads) || num_rows > 65535) return SWL_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(num_rows) > static_cast<int64_t>(num_seqs) * max_new_len) return SWL_ERR_BAD_ARG;
    if (const int rc = swl::check_decode_layout(a)) return rc;
    // every key of the longest sequence belongs to a split, and to a block of its table row
    if (static_cast<int64_t>(seq_block_size) * num_seq_blocks < max_total_len) return SWL_ERR_BAD_ARG;
    if ((static_cast<int64_t>(max_total_len) + block_size - 1) / block_size > max_blocks_per_seq) return SWL_ERR_BAD_ARG;
    float *mid_o, *mid_lse;
    if (!swl::split_scratch(scratch, num_rows, num_q_heads, head_dim, num_seq_blocks, mid_o, mid_lse))
        return SWL_ERR_BAD_ARG;
    swl::DecodeAttnParams p{};
    swl::fill_decode_params(p, a, mid_o, mid_lse, softmax_scale);
    int rc;
    SWL_DISPATCH_DTYPE(dtype, T, {
        rc = swl::launch_verify<T>(p, block_table, seq_ids, cu_seqlens, ctx_lens, num_seqs, head_dim,
                                   static_cast<hipStream_t>(stream));
    });
    if (rc != SWL_OK || num_seq_blocks == 1) return rc;
    // every row is a "sequence" of row_lens[r] keys: it reads the ceil(row_lens[r] / seq_block_size) partials it has
    return swl_paged_attn_phase2(o, mid_o, mid_lse, row_lens, num_rows, num_q_heads, head_dim, seq_block_size,
                                 num_seq_blocks, o_tok_stride, dtype, stream);
}
