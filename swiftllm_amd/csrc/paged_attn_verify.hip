// paged_attn_verify.hip — paged attention for a speculative-decoding VERIFY step on gfx950 (an addition, no reference
// counterpart): every sequence brings n <= 16/G new tokens (its last accepted token and its drafts) behind c resident
// ones; row i attends keys j <= c + i. The semantics are swl_prefill_attn_paged's (prefill_attn_paged.hip), the
// arithmetic is the decode kernel's (paged_attn.hip, plain-q matrix-core path):
//   * grid (split, kv-head, sequence), 4 or 8 waves, register K/V ring of depth 2, attend_block_mfma (attn_mfma.h);
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
#include "attn_mfma.h"

namespace swl {

template <int V>
struct VerifyIntTag {
    static constexpr int value = V;
};

struct PagedAttnVerifyParams {
    void *o;
    const void *q;
    const void *k_cache;
    const void *v_cache;
    float *mid_o;
    float *mid_lse;
    float scale_log2e;
    int H, KVH, L, layer, max_blocks_per_seq, seq_block_size, num_seq_blocks;
    int64_t q_tok_stride, o_tok_stride;
};

constexpr int kVerifyCols = 16; // N columns of the MFMA tile = (token, head) pairs per kv-head
constexpr int kVerifyDepth = 2; // K/V register ring, as the decode kernel's matrix-core path (kPaMfmaDepth)

// block_table / seq_ids / cu_seqlens / ctx_lens are __restrict__ kernel arguments so block ids stay scalar loads
// (see paged_attn_phase1_kernel).
template <typename T, int D, int G, int NW>
__global__ __launch_bounds__(NW * 64) void paged_attn_verify_kernel(PagedAttnVerifyParams p,
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
    auto load_block = [&](int b, vec8_t<T>(&Kd)[NI], vec8_t<T>(&Vd)[NI]) {
        load_phys(bt[b], Kd, Vd); // scalar load: b is wave-uniform
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
    auto prefetch_kv = [&](int b0, auto lo_tag, auto hi_tag) {
#pragma unroll
        for (int d = decltype(lo_tag)::value; d < decltype(hi_tag)::value; ++d)
            if (b0 + d * NW < blk_end) load_block(b0 + d * NW, Kr[d], Vr[d]);
    };

    int b = tok_begin / kBlk + wave;
    prefetch_kv(b, VerifyIntTag<0>{}, VerifyIntTag<ND>{});
    // steady state and drain: the decode kernel's (paged_attn_phase1_kernel), fences included
    if (b + (2 * ND - 1) * NW < blk_end) {
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0), expcnt/lgkmcnt untouched
        do {
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const int64_t phys_next = bt[b + (d + ND) * NW];
                __builtin_amdgcn_sched_barrier(0);
                attend(b + d * NW, Kr[d], Vr[d]);
                __builtin_amdgcn_sched_barrier(0);
                load_phys(phys_next, Kr[d], Vr[d]);
                __builtin_amdgcn_sched_barrier(0);
            }
            b += ND * NW;
        } while (b + (2 * ND - 1) * NW < blk_end);
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        if (b + d * NW < blk_end) {
            attend(b + d * NW, Kr[d], Vr[d]);
            __builtin_amdgcn_sched_barrier(0);
            if (b + (d + ND) * NW < blk_end) load_block(b + (d + ND) * NW, Kr[d], Vr[d]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int d = 0; d < ND - 1; ++d)
        if (b + (d + ND) * NW < blk_end) attend(b + (d + ND) * NW, Kr[d], Vr[d]);

    // O^T of the last block is stored by DS instructions below (swl_common.h)
#pragma unroll
    for (int mm = 0; mm < MT::OS; ++mm) mfma_results_tie(acc4[mm]);
    mfma_results_ready<4>(acc4[MT::OS - 1]);
    // the four lanes (mq = 0..3) of a column share m and each hold the row sum of their own tokens
    const float lt = rows_allreduce_sum(l);
    if (mq == 0) {
        sm_ml[wave][mh][0] = m;
        sm_ml[wave][mh][1] = lt;
    }
#pragma unroll
    for (int mm = 0; mm < MT::OS; ++mm)
#pragma unroll
        for (int r = 0; r < 4; ++r) sm_acc[wave][mh][16 * mm + 4 * mq + r] = acc4[mm][r];
    __syncthreads();

    // merge the waves (merge_waves_write's arithmetic) and write the real columns that saw a key in this split
    const int nsb = p.num_seq_blocks;
    for (int oidx = threadIdx.x; oidx < C * D; oidx += NW * 64) {
        const int col = oidx / D;
        const int d = oidx % D;
        const int t = col / G;
        if (t >= n || ctx + t + 1 <= tok_begin) continue; // idle column / no visible key: contributes nothing
        float M = sm_ml[0][col][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) M = fmaxf(M, sm_ml[w][col][0]);
        float Lsum = 0.f, A = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float wgt = fast_exp2((sm_ml[w][col][0] - M) * c);
            Lsum = fmaf(sm_ml[w][col][1], wgt, Lsum);
            A = fmaf(sm_acc[w][col][d], wgt, A);
        }
        const float out = A / Lsum;
        const int head = kvh * G + col % G;
        const int64_t orow = row0 + t;
        if (nsb == 1) {
            static_cast<T *>(p.o)[orow * p.o_tok_stride + static_cast<int64_t>(head) * D + d] = to_t<T>(out);
        } else {
            const int64_t part = (orow * p.H + head) * nsb + split;
            p.mid_o[part * D + d] = out;
            if (d == 0) p.mid_lse[part] = fast_log2(Lsum) + M * c;
        }
    }
}

template <typename T, int D, int G>
static int launch_verify(const PagedAttnVerifyParams &p, const int *bt, const int *seq_ids, const int *cu,
                         const int *ctx, int num_seqs, hipStream_t stream) {
    const dim3 grid(p.num_seq_blocks, p.KVH, num_seqs);
    // >= 32 KV blocks per split: 8-wave workgroups, else 4 (launch_phase1's rule)
    if (p.seq_block_size >= 32 * kBlk)
        hipLaunchKernelGGL((paged_attn_verify_kernel<T, D, G, 8>), grid, dim3(512), 0, stream, p, bt, seq_ids, cu, ctx);
    else
        hipLaunchKernelGGL((paged_attn_verify_kernel<T, D, G, 4>), grid, dim3(256), 0, stream, p, bt, seq_ids, cu, ctx);
    return check_launch();
}

template <typename T, int D>
static int dispatch_verify_g(const PagedAttnVerifyParams &p, const int *bt, const int *seq_ids, const int *cu,
                             const int *ctx, int num_seqs, int G, hipStream_t stream) {
    switch (G) {
    case 1: return launch_verify<T, D, 1>(p, bt, seq_ids, cu, ctx, num_seqs, stream);
    case 2: return launch_verify<T, D, 2>(p, bt, seq_ids, cu, ctx, num_seqs, stream);
    case 4: return launch_verify<T, D, 4>(p, bt, seq_ids, cu, ctx, num_seqs, stream);
    case 8: return launch_verify<T, D, 8>(p, bt, seq_ids, cu, ctx, num_seqs, stream);
    default: return SWL_ERR_UNSUPPORTED;
    }
}

template <typename T>
static int dispatch_verify(const PagedAttnVerifyParams &p, const int *bt, const int *seq_ids, const int *cu,
                           const int *ctx, int num_seqs, int D, int G, hipStream_t stream) {
    switch (D) {
    case 32: return dispatch_verify_g<T, 32>(p, bt, seq_ids, cu, ctx, num_seqs, G, stream);
    case 64: return dispatch_verify_g<T, 64>(p, bt, seq_ids, cu, ctx, num_seqs, G, stream);
    case 128: return dispatch_verify_g<T, 128>(p, bt, seq_ids, cu, ctx, num_seqs, G, stream);
    default: return SWL_ERR_UNSUPPORTED;
    }
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
    if (num_q_heads <= 0 || num_kv_heads <= 0 || num_q_heads % num_kv_heads != 0 || head_dim <= 0 || num_layers <= 0 ||
        cur_layer < 0 || cur_layer >= num_layers || max_blocks_per_seq <= 0 || max_new_len <= 0 ||
        max_total_len < max_new_len || num_seq_blocks <= 0)
        return SWL_ERR_BAD_ARG;
    if (block_size != swl::kBlk) return SWL_ERR_UNSUPPORTED;
    if (!(head_dim == 32 || head_dim == 64 || head_dim == 128)) return SWL_ERR_UNSUPPORTED;
    const int tmax = swl_paged_attn_verify_max_tokens(num_q_heads, num_kv_heads);
    if (tmax == 0 || max_new_len > tmax) return SWL_ERR_UNSUPPORTED;
    if (num_seqs > 65535 || num_rows > 65535 || num_kv_heads > 65535) return SWL_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(num_rows) > static_cast<int64_t>(num_seqs) * max_new_len) return SWL_ERR_BAD_ARG;
    if (seq_block_size <= 0 || seq_block_size % block_size != 0) return SWL_ERR_BAD_ARG;
    // every key of the longest sequence belongs to a split, and to a block of its table row
    if (static_cast<int64_t>(seq_block_size) * num_seq_blocks < max_total_len) return SWL_ERR_BAD_ARG;
    if ((static_cast<int64_t>(max_total_len) + block_size - 1) / block_size > max_blocks_per_seq) return SWL_ERR_BAD_ARG;
    const int64_t hd = static_cast<int64_t>(num_q_heads) * head_dim;
    if (!swl::aligned16(o) || !swl::aligned16(q) || !swl::aligned16(k_cache) || !swl::aligned16(v_cache) ||
        (q_tok_stride & 7) || q_tok_stride < hd || (o_tok_stride & 7) || o_tok_stride < hd)
        return SWL_ERR_BAD_ARG;
    float *mid_o = nullptr, *mid_lse = nullptr;
    if (num_seq_blocks > 1) {
        if (!scratch || !swl::aligned16(scratch)) return SWL_ERR_BAD_ARG;
        mid_o = static_cast<float *>(scratch);
        mid_lse = mid_o + static_cast<size_t>(num_rows) * num_q_heads * num_seq_blocks * head_dim;
    }
    swl::PagedAttnVerifyParams p{};
    p.o = o;
    p.q = q;
    p.k_cache = k_cache;
    p.v_cache = v_cache;
    p.mid_o = mid_o;
    p.mid_lse = mid_lse;
    p.scale_log2e = softmax_scale * 1.44269504088896340736f;
    p.H = num_q_heads;
    p.KVH = num_kv_heads;
    p.L = num_layers;
    p.layer = cur_layer;
    p.max_blocks_per_seq = max_blocks_per_seq;
    p.seq_block_size = seq_block_size;
    p.num_seq_blocks = num_seq_blocks;
    p.q_tok_stride = q_tok_stride;
    p.o_tok_stride = o_tok_stride;
    const int G = num_q_heads / num_kv_heads;
    int rc;
    SWL_DISPATCH_DTYPE(dtype, T, {
        rc = swl::dispatch_verify<T>(p, block_table, seq_ids, cu_seqlens, ctx_lens, num_seqs, head_dim, G,
                                     static_cast<hipStream_t>(stream));
    });
    if (rc != SWL_OK || num_seq_blocks == 1) return rc;
    // every row is a "sequence" of row_lens[r] keys: it reads the ceil(row_lens[r] / seq_block_size) partials it has
    return swl_paged_attn_phase2(o, mid_o, mid_lse, row_lens, num_rows, num_q_heads, head_dim, seq_block_size,
                                 num_seq_blocks, o_tok_stride, dtype, stream);
}
