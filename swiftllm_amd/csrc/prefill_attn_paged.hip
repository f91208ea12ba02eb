// prefill_attn_paged.hip — causal flash attention of prompt CHUNKS over the paged KV pool (GQA) on the CDNA4 matrix
// cores (gfx950): chunked prefill, continuation of a sequence whose first tokens are already resident.
//
// The reference has no such operator (its prefill attends to the fresh projections only: transformer_layer.py:83-96);
// this is an addition. Sequence s has c = ctx_lens[s] tokens in the pool and n = cu[s+1] - cu[s] new ones whose rotated K
// and V were written to logical positions [c, c + n) by swl_rotary_store_kv_prefill_at / swl_store_kv_prefill_at on
// the same stream just before. Row i of the chunk (absolute position c + i) sees keys j <= c + i. ALL keys and values,
// the chunk's own included, are read from the pool through the block table: one address stream, and the store is
// bit-exact, so the bits are those of the fresh projections. c is any value >= 0 (c = 0: a plain causal prefill);
// n = 0 sequences launch workgroups that leave on their first branch.
//
// The grid decode, the Q^T load, the arithmetic of a 64-key tile and the epilogue are prefill_tile.h's, the body the
// fresh-K/V kernels of prefill_attn.hip run: same arithmetic, same fragment order, same error bounds, and at c = 0 the same
// bits by construction. Workgroup = 4 waves = 128 chunk rows of one (sequence, q-head); row-major K/V tiles at the pitches
// of prefill_attn_kernel. What this kernel adds:
//   * the mask compares ABSOLUTE positions (row c + i against key j);
//   * keys are walked in 64-key tiles ALIGNED TO ABSOLUTE POSITION 0, so a tile is exactly four 16-token pool blocks.
//     For one (block, layer, kv-head) the 16 x D slab is contiguous (4 KiB at D = 128): a staging pass reads one block
//     id (at D = 128 the id is workgroup-uniform: a scalar load) and 16 bytes per lane from that slab. Block ids are
//     fetched one tile ahead of the K/V loads that need them, the K/V loads one tile ahead of the MFMAs (issue-early /
//     write-late, as the register-staged kernel of prefill_attn.hip).
//   * work per q-block is ceil((c + q0 + rows) / 64) tiles — it grows with the CONTEXT, not with q0 alone. Inside a
//     sequence it is still monotone in q0, so the descending q-block order issues the longest first; across sequences
//     the contexts live on the device and the host does not sort by them.
//
// The masked-garbage hazard. The slots of a sequence's last block past c + n, and every pool block outside its table,
// hold whatever an earlier owner left — NaN and Inf included — and a masked key must contribute NOTHING: its p is
// exactly 0, but 0 * NaN in the PV product is NaN. Keys >= c + n are therefore never read: their K and V rows are
// staged as zeros (block-table indices past the sequence's last block are clamped and unused). Keys inside [0, c + n)
// above a row's diagonal are real, finite rows the store has just written; their scores are replaced by the finite
// stand-in for -inf before the softmax, so p = 0 times a finite v. In an FP8 pool the codes 0x7f / 0xff are NaN and a slot
// past the length may hold them: the rule is the same, the zero rows are staged as code 0x00 = +0.
//
// The two pool formats. prefill_attn_paged_kernel<T, D, FP8> is ONE kernel: grid, tiles, fragment order, masking, lazy
// maximum and epilogue do not know how the pool is stored. FP8 = false reads pools of T. FP8 = true reads 1-byte e4m3fn
// pools (storage contract: fp8_kv.h) and computes on the STORED values, since the conversion to T is exact. What the
// format decides is the staging and two factors:
//   * a lane's 16 bytes per pass are 8 elements or 16 codes, so a pass covers 256 / (D / 8) tile rows (16 / 32 / 64 at
//     D = 128 / 64 / 32) or 256 / (D / 16), at most the tile (32 / 64 / 64; at D = 32 threads 128..255 stage nothing).
//     Only the 16-row pass of 16-bit pools at D = 128 has a workgroup-uniform block id; an FP8 pass may span two blocks;
//   * FP8: the conversion (v_cvt_scalef32_pk_*_fp8, scale 1) sits between the staging registers and the two 16-byte LDS
//     writes per lane;
//   * FP8: k_scale[layer, kv-head] is folded into the exp2 factor c = scale * log2(e) * k_scale, v_scale into the final
//     normalisation before the one rounding. 16-bit pools carry no such multiplies.
// With FP8 pools the chunk's own keys are read back QUANTISED: a chunked prompt is not bit-equal to a whole-prompt prefill
// (which attends to its fresh 16-bit projections).
#include <type_traits>

#include "prefill_tile.h"
#include "fp8_kv.h"

namespace swl {

struct PagedPrefillParams {
    void *o;
    const void *q;
    const void *k_cache;
    const void *v_cache;
    const int *block_table;
    const int *seq_ids;
    const int *cu_seqlens;
    const int *ctx_lens;
    int num_seqs, H, KVH, num_q_blocks;
    int num_layers, cur_layer, max_blocks_per_seq;
    float scale_log2e;
    int64_t q_tok_stride, o_tok_stride;
    const float *kv_scales;     // FP8 pools: [2][L][KVH]; not read for 16-bit pools
};

template <typename T, int D, bool FP8>
__global__ __launch_bounds__(256, 2) void prefill_attn_paged_kernel(PagedPrefillParams p) {
    constexpr int KRS = D + 8;   // K row pitch (elements): 16 consecutive rows hit 16 distinct 16-B slots
    constexpr int VRS = D + 32;  // V row pitch: 4 rows x two 16-col halves tile the 64 banks exactly
    constexpr int KSTEPS = D / 16;
    constexpr int DT = D / 32;
    using Pool = std::conditional_t<FP8, uint8_t, T>;        // pool element
    using Raw = std::conditional_t<FP8, u32x4_t, vec8_t<T>>; // a lane's 16 bytes of a pool row
    constexpr int EPC = 16 / sizeof(Pool);   // pool elements per 16-byte chunk
    constexpr int SCPR = D / EPC;            // 16-byte chunks per pool row (staging)
    constexpr int RPP = 256 / SCPR < kBK ? 256 / SCPR : kBK;   // rows staged per pass (see the header)
    constexpr int NPASS = kBK / RPP;       // passes per tile
    __shared__ __attribute__((aligned(16))) T smem[kBK * KRS + kBK * VRS];   // K tile, V tile; the O tiles of the epilogue
    T *const Ks = smem;
    T *const Vs = smem + kBK * KRS;

    const PrefillGrid u = PrefillGrid::decode(blockIdx.x, p.num_seqs, p.H, p.KVH, p.num_q_blocks, 1);   // most tiles first
    if (!u.valid) return;
    const int seq = u.seq, kvh = u.kvh;
    const int head = kvh * (p.H / p.KVH) + u.hgroup;
    const int start = p.cu_seqlens[seq];
    const int len = p.cu_seqlens[seq + 1] - start;      // new tokens (chunk rows)
    const int q0 = u.qb * kBQ;
    if (q0 >= len) return;
    const int ctx = p.ctx_lens[seq];
    const int total = ctx + len;                        // keys resident once the chunk is stored
    const int last_blk = (total - 1) / kBlk;            // last logical block of the sequence (len >= 1 here)
    const int *bt = p.block_table + static_cast<int64_t>(p.seq_ids[seq]) * p.max_blocks_per_seq;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31;
    const int hf = lane >> 5;
    const int q0w = q0 + wave * 32; // first chunk row of this wave
    const int qrow = q0w + l32;     // this lane's chunk row
    const int qpos = ctx + qrow;    // ... and its absolute position: it sees keys <= qpos
    const int qpos0w = ctx + q0w;
    float c = p.scale_log2e, v_scale = 1.0f;
    if constexpr (FP8) {
        c *= p.kv_scales[static_cast<int64_t>(p.cur_layer) * p.KVH + kvh];
        v_scale = p.kv_scales[(static_cast<int64_t>(p.num_layers) + p.cur_layer) * p.KVH + kvh];
    }

    const T *qg = static_cast<const T *>(p.q);
    const Pool *kc = static_cast<const Pool *>(p.k_cache);
    const Pool *vc = static_cast<const Pool *>(p.v_cache);

    vec8_t<T> qf[KSTEPS];
    prefill_load_q<T, D>(qf, qg, start, head, p.q_tok_stride, qrow, len, hf);

    float16_t ot[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) ot[dt] = float16_t{};
    float m_run = kNegBig;
    float l_run = 0.f;

    // ---- staging: thread -> (tile row srow + pass*RPP, chunk sc); tile row r = block r / 16 of the tile, slot r % 16 ----
    const int srow = tid / SCPR;
    const int sc = tid % SCPR;
    // FP8, D = 32: a pass is the whole tile and threads 128.. have no row. (At D >= 64 every FP8 thread stages as well; the
    // test stays a run-time one there, as it has been since the FP8 kernel was written: its register allocation is kept.)
    const bool stager = !FP8 || srow < RPP;
    Raw kst[NPASS], vst[NPASS];
    int bid[NPASS];                                      // pool block of each pass, for the tile fetch_tile takes next
    // offset of (block 0, this layer, this kv-head, slot 0) and the pitch of one pool block, in pool elements
    const int64_t blk_pitch = static_cast<int64_t>(p.num_layers) * p.KVH * kBlk * D;
    const int64_t slab0 = (static_cast<int64_t>(p.cur_layer) * p.KVH + kvh) * kBlk * D;
    auto load_ids = [&](int tile) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            // (RPP = 16: the block of a pass is the same for the whole workgroup — a scalar load)
            const int b = 4 * tile + (RPP == 16 ? ps : ((stager ? srow : 0) + ps * RPP) >> 4);
            bid[ps] = bt[min(b, last_blk)];              // indices past the sequence's blocks: clamped, their rows unused
        }
    };
    auto fetch_tile = [&](int tile) {
        const int key0 = tile * kBK;
        const bool whole = key0 + kBK <= total;        // (workgroup-uniform) every key of the tile is resident
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int r = srow + ps * RPP;
            const int64_t off = static_cast<int64_t>(bid[ps]) * blk_pitch + slab0 + (r & 15) * D + sc * EPC;
            Raw kt = Raw{}, vt = Raw{};
            if (stager && (whole || key0 + r < total)) { // keys >= c + n are never read: zeros (see the header)
                kt = *reinterpret_cast<const Raw *>(kc + off);
                vt = *reinterpret_cast<const Raw *>(vc + off);
            }
            kst[ps] = kt;
            vst[ps] = vt;
        }
    };
    auto to_lds = [&](T *dst, const Raw &raw) {
        if constexpr (FP8) {
            vec8_t<T> lo, hi;
            fp8x16_to_t<T>(raw, lo, hi);
            *reinterpret_cast<vec8_t<T> *>(dst) = lo;
            *reinterpret_cast<vec8_t<T> *>(dst + 8) = hi;
        } else {
            *reinterpret_cast<vec8_t<T> *>(dst) = raw;
        }
    };
    auto commit_tile = [&]() {
        if (!stager) return;
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int r = srow + ps * RPP;
            to_lds(&Ks[r * KRS + sc * EPC], kst[ps]);
            to_lds(&Vs[r * VRS + sc * EPC], vst[ps]);
        }
    };

    const int kv_end = min(total, ctx + q0 + kBQ);     // keys this q-block can see
    const int ntiles = (kv_end + kBK - 1) / kBK;

    // per-lane LDS offsets of the fragment reads
    const int k_frag_off = l32 * KRS + hf * 8;                            // + t*32*KRS + kk*16
    const int i16 = lane & 15;
    const int v_frag_off = (4 * hf + (i16 >> 2)) * VRS + 16 * ((lane >> 4) & 1) + 4 * (i16 & 3);

    load_ids(0);
    fetch_tile(0);
    if (ntiles > 1) load_ids(1);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int key0 = tile * kBK;
        __syncthreads(); // everyone finished reading the previous tile
        commit_tile();
        __syncthreads();
        if (tile + 1 < ntiles) {
            fetch_tile(tile + 1);                        // in flight during the MFMAs below
            if (tile + 2 < ntiles) load_ids(tile + 2);   // ... and the block ids of the tile after it
        }

        if (key0 > qpos0w + 31) continue; // whole tile above this wave's diagonal
        // the mask compares ABSOLUTE positions (keys >= c + n are > every valid row's position as well)
        prefill_tile<T, D, true>(
            qf, ot, m_run, l_run, c, qpos - key0 - 4 * hf, key0 + kBK - 1 > qpos0w,
            [&](int t, int kk) { return *reinterpret_cast<const vec8_t<T> *>(&Ks[k_frag_off + t * 32 * KRS + kk * 16]); },
            [&](int t, int ks, int dt, int half) {
                return lds_tr_read(&Vs[v_frag_off + (t * 32 + 16 * ks + 8 * half) * VRS + dt * 32]);
            });
    }

    static_assert(4 * 32 * (D + 8) <= kBK * KRS + kBK * VRS, "the four waves' O tiles must fit the K/V tiles' LDS");
    __syncthreads();                                 // every wave is done with the last K/V tile
    T *obase = static_cast<T *>(p.o) + static_cast<int64_t>(start) * p.o_tok_stride + static_cast<int64_t>(head) * D;
    prefill_store_rows<T, D, FP8>(ot, l_run, v_scale, smem + wave * 32 * (D + 8), obase, p.o_tok_stride, q0w, len, lane, l32, hf);
}

} // namespace swl

// Argument checks and launch of both entries. They differ in what a bad head_dim returns (bad_head_dim), in the scales
// pointer, and FP8 rejects an unknown dtype before the block size is looked at.
template <bool FP8>
static int launch_prefill_attn_paged(void *o, const void *q, const void *k_cache, const void *v_cache, const float *kv_scales,
                                     const int32_t *block_table, const int32_t *seq_ids, const int32_t *cu_seqlens,
                                     const int32_t *ctx_lens, int32_t num_prefill_seqs, int32_t max_new_len,
                                     int32_t max_total_len, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                                     int32_t num_layers, int32_t block_size, int32_t cur_layer, int32_t max_blocks_per_seq,
                                     float softmax_scale, int64_t q_tok_stride, int64_t o_tok_stride, int32_t dtype,
                                     swl_stream_t stream, int bad_head_dim) {
    if (num_prefill_seqs < 0 || max_new_len < 0 || max_total_len < 0) return SWL_ERR_BAD_ARG;
    if (num_prefill_seqs == 0 || max_new_len == 0) return SWL_OK;
    if (!o || !q || !k_cache || !v_cache || (FP8 && !kv_scales) || !block_table || !seq_ids || !cu_seqlens || !ctx_lens)
        return SWL_ERR_BAD_ARG;
    if (num_q_heads <= 0 || num_kv_heads <= 0 || num_q_heads % num_kv_heads != 0) return SWL_ERR_BAD_ARG;
    if (num_layers <= 0 || cur_layer < 0 || cur_layer >= num_layers || max_blocks_per_seq <= 0 || block_size <= 0)
        return SWL_ERR_BAD_ARG;
    if (max_total_len < max_new_len) return SWL_ERR_BAD_ARG;
    if (!(head_dim == 32 || head_dim == 64 || head_dim == 128)) return bad_head_dim;
    if (FP8 && !(dtype == SWL_F16 || dtype == SWL_BF16)) return SWL_ERR_BAD_ARG;
    if (block_size != swl::kBlk) return SWL_ERR_UNSUPPORTED;
    // the longest sequence must fit a block-table row (the kernel reads ceil(total / 16) entries of it)
    if ((static_cast<int64_t>(max_total_len) + block_size - 1) / block_size > max_blocks_per_seq) return SWL_ERR_BAD_ARG;
    if ((q_tok_stride & 7) || (o_tok_stride & 7) || q_tok_stride < static_cast<int64_t>(num_q_heads) * head_dim ||
        o_tok_stride < static_cast<int64_t>(num_q_heads) * head_dim)
        return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(q) || !swl::aligned16(o) || !swl::aligned16(k_cache) || !swl::aligned16(v_cache))
        return SWL_ERR_BAD_ARG;
    swl::PagedPrefillParams p;
    p.o = o;
    p.q = q;
    p.k_cache = k_cache;
    p.v_cache = v_cache;
    p.block_table = block_table;
    p.seq_ids = seq_ids;
    p.cu_seqlens = cu_seqlens;
    p.ctx_lens = ctx_lens;
    p.num_seqs = num_prefill_seqs;
    p.H = num_q_heads;
    p.KVH = num_kv_heads;
    p.num_q_blocks = (max_new_len + swl::kBQ - 1) / swl::kBQ;
    p.num_layers = num_layers;
    p.cur_layer = cur_layer;
    p.max_blocks_per_seq = max_blocks_per_seq;
    p.scale_log2e = softmax_scale * 1.44269504088896340736f;
    p.q_tok_stride = q_tok_stride;
    p.o_tok_stride = o_tok_stride;
    p.kv_scales = kv_scales;
    dim3 grid;
    if (!swl::prefill_grid_blocks(num_prefill_seqs, num_kv_heads, num_q_heads / num_kv_heads, p.num_q_blocks, &grid))
        return SWL_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SWL_DISPATCH_DTYPE(dtype, T, {
        if (head_dim == 128)
            hipLaunchKernelGGL((swl::prefill_attn_paged_kernel<T, 128, FP8>), grid, dim3(256), 0, s, p);
        else if (head_dim == 64)
            hipLaunchKernelGGL((swl::prefill_attn_paged_kernel<T, 64, FP8>), grid, dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((swl::prefill_attn_paged_kernel<T, 32, FP8>), grid, dim3(256), 0, s, p);
    });
    return swl::check_launch();
}

extern "C" int swl_prefill_attn_paged(void *o, const void *q, const void *k_cache, const void *v_cache,
                                      const int32_t *block_table, const int32_t *seq_ids, const int32_t *cu_seqlens,
                                      const int32_t *ctx_lens, int32_t num_prefill_seqs, int32_t max_new_len,
                                      int32_t max_total_len, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                                      int32_t num_layers, int32_t block_size, int32_t cur_layer,
                                      int32_t max_blocks_per_seq, float softmax_scale, int64_t q_tok_stride,
                                      int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    return launch_prefill_attn_paged<false>(o, q, k_cache, v_cache, nullptr, block_table, seq_ids, cu_seqlens, ctx_lens,
                                            num_prefill_seqs, max_new_len, max_total_len, num_q_heads, num_kv_heads,
                                            head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq, softmax_scale,
                                            q_tok_stride, o_tok_stride, dtype, stream, SWL_ERR_UNSUPPORTED);
}

extern "C" int swl_prefill_attn_paged_fp8(void *o, const void *q, const void *k_cache, const void *v_cache,
                                          const float *kv_scales, const int32_t *block_table, const int32_t *seq_ids,
                                          const int32_t *cu_seqlens, const int32_t *ctx_lens, int32_t num_prefill_seqs,
                                          int32_t max_new_len, int32_t max_total_len, int32_t num_q_heads,
                                          int32_t num_kv_heads, int32_t head_dim, int32_t num_layers, int32_t block_size,
                                          int32_t cur_layer, int32_t max_blocks_per_seq, float softmax_scale,
                                          int64_t q_tok_stride, int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    return launch_prefill_attn_paged<true>(o, q, k_cache, v_cache, kv_scales, block_table, seq_ids, cu_seqlens, ctx_lens,
                                           num_prefill_seqs, max_new_len, max_total_len, num_q_heads, num_kv_heads,
                                           head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq, softmax_scale,
                                           q_tok_stride, o_tok_stride, dtype, stream, SWL_ERR_BAD_ARG);
}
