// prefill_attn_paged_fp8.hip — causal flash attention of prompt CHUNKS over the FP8 (e4m3fn) paged KV pool (gfx950).
//
// prefill_attn_paged.hip reading 1-byte pools (storage contract: fp8_kv.h): same grid, same 64-key tiles aligned to
// absolute position 0, same fragment order, same arithmetic and error bounds — on the STORED values, since the
// conversion to the activation dtype is exact. Only the staging differs: it is register-based, 16 bytes per lane per
// pass, and those 16 bytes are now 16 elements, so a pass covers 256 / (D / 16) tile rows (32 / 64 / all 64 of them at
// D = 128 / 64 / 32; at D = 32 threads 128..255 stage nothing) and the conversion (v_cvt_scalef32_pk_*_fp8, scale 1)
// sits between the load and the two 16-byte LDS writes. A pass may span two pool blocks, so block ids are per-lane loads.
// k_scale[layer, kv-head] is folded into the exp2 factor c = scale * log2(e) * k_scale, v_scale into the final
// normalisation before the one rounding. The chunk's own keys are read back QUANTISED: a chunked prompt is not
// bit-equal to a whole-prompt prefill in FP8 mode (which attends to its fresh 16-bit projections).
//
// The masked-garbage rule holds as there: keys >= c + n are never read — their rows are staged as code 0x00 = +0 (a slot
// past the length may hold the NaN codes 0x7f / 0xff) — and keys above a row's diagonal inside [0, c + n) are finite
// values the store has just written.
#include "fp8_kv.h"

namespace swl {

typedef short pg8_short4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float16_t pg8_mfma32(vec8_t<f16> a, vec8_t<f16> b, float16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float16_t pg8_mfma32(vec8_t<bf16> a, vec8_t<bf16> b, float16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// LDS transpose read (see prefill_attn.hip): lane i of a 16-lane group receives column i of a 4 x 16 block.
template <typename T>
__device__ __forceinline__ pg8_short4_t pg8_lds_tr_read(const T *p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((pg8_short4_t __attribute__((address_space(3))) *)(p));
}

struct PagedPrefillFp8Params {
    void *o;
    const void *q;
    const uint8_t *k_cache;
    const uint8_t *v_cache;
    const float *kv_scales;     // [2][L][KVH]
    const int *block_table;
    const int *seq_ids;
    const int *cu_seqlens;
    const int *ctx_lens;
    int num_seqs, H, KVH, num_q_blocks;
    int num_layers, cur_layer, max_blocks_per_seq;
    float scale_log2e;
    int64_t q_tok_stride, o_tok_stride;
};

constexpr float kPg8LazyMax = 4.0f; // = kLazyMax of prefill_attn.hip (p <= 16)
constexpr int kPg8BQ = 128;         // chunk rows per workgroup
constexpr int kPg8BK = 64;          // keys per LDS tile = four pool blocks
constexpr int kPg8Blk = 16;         // tokens per pool block

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void prefill_attn_paged_fp8_kernel(PagedPrefillFp8Params p) {
    constexpr int KRS = D + 8;   // K row pitch (elements): 16 consecutive rows hit 16 distinct 16-B slots
    constexpr int VRS = D + 32;  // V row pitch: 4 rows x two 16-col halves tile the 64 banks exactly
    constexpr int KSTEPS = D / 16;
    constexpr int DT = D / 32;
    constexpr int CPR = D / 8;           // 16-byte chunks per row of the 16-bit output (epilogue)
    constexpr int SCPR = D / 16;         // 16-byte (16-code) chunks per pool row (staging)
    constexpr int RPP = 256 / SCPR < kPg8BK ? 256 / SCPR : kPg8BK;   // rows staged per pass (32 / 64 / 64 at D = 128 / 64 / 32)
    constexpr int NPASS = kPg8BK / RPP;   // passes per tile
    __shared__ __attribute__((aligned(16))) T smem[kPg8BK * KRS + kPg8BK * VRS];   // K tile, V tile; the O tiles of the epilogue
    T *const Ks = smem;
    T *const Vs = smem + kPg8BK * KRS;

    // ---- XCD-aware decode of the 1-D grid (as prefill_attn_kernel) ---------------------------------
    const int G = p.H / p.KVH;
    const int per_unit = G * p.num_q_blocks;
    const int id = blockIdx.x;
    const int xcd = id & 7;
    const int j = id >> 3;
    const int unit = xcd + 8 * (j / per_unit);
    if (unit >= p.num_seqs * p.KVH) return;
    const int inner = j % per_unit;
    const int g = inner % G;
    const int qb = p.num_q_blocks - 1 - inner / G; // most tiles first
    const int seq = unit / p.KVH;
    const int kvh = unit % p.KVH;
    const int head = kvh * G + g;

    const int start = p.cu_seqlens[seq];
    const int len = p.cu_seqlens[seq + 1] - start;      // new tokens (chunk rows)
    const int q0 = qb * kPg8BQ;
    if (q0 >= len) return;
    const int ctx = p.ctx_lens[seq];
    const int total = ctx + len;                        // keys resident once the chunk is stored
    const int last_blk = (total - 1) / kPg8Blk;          // last logical block of the sequence (len >= 1 here)
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
    const float c = p.scale_log2e * p.kv_scales[static_cast<int64_t>(p.cur_layer) * p.KVH + kvh];
    const float v_scale = p.kv_scales[(static_cast<int64_t>(p.num_layers) + p.cur_layer) * p.KVH + kvh];

    const T *qg = static_cast<const T *>(p.q);
    const uint8_t *kc = p.k_cache;
    const uint8_t *vc = p.v_cache;

    // ---- Q^T B-fragments: lane holds Q[qrow][kk*16 + hf*8 .. +8] ---------------------------------
    vec8_t<T> qf[KSTEPS];
    {
        const bool ok = qrow < len;
        const T *qp = qg + (static_cast<int64_t>(start) + (ok ? qrow : 0)) * p.q_tok_stride +
                      static_cast<int64_t>(head) * D + hf * 8;
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) {
            vec8_t<T> t = load8(qp + kk * 16);
            if (!ok) t = vec8_t<T>{};
            qf[kk] = t;
        }
    }

    float16_t ot[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) ot[dt] = float16_t{};
    float m_run = kNegBig;
    float l_run = 0.f;

    // ---- staging: thread -> (tile row srow + pass*RPP, 16-code chunk sc); tile row r = block r / 16 of the tile, slot r % 16
    const int srow = tid / SCPR;
    const int sc = tid % SCPR;
    const bool stager = srow < RPP;                      // (D = 32: a pass is the whole tile, threads 128.. have no row)
    u32x4_t kst[NPASS], vst[NPASS];
    int bid[NPASS];                                      // pool block of each pass, for the tile fetch_tile takes next
    // byte offset of (block 0, this layer, this kv-head, slot 0) and the pitch of one pool block
    const int64_t blk_pitch = static_cast<int64_t>(p.num_layers) * p.KVH * kPg8Blk * D;
    const int64_t slab0 = (static_cast<int64_t>(p.cur_layer) * p.KVH + kvh) * kPg8Blk * D;
    auto load_ids = [&](int tile) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int b = 4 * tile + (((stager ? srow : 0) + ps * RPP) >> 4);
            bid[ps] = bt[min(b, last_blk)];              // indices past the sequence's blocks: clamped, their rows unused
        }
    };
    auto fetch_tile = [&](int tile) {
        const int key0 = tile * kPg8BK;
        const bool whole = key0 + kPg8BK <= total;        // (workgroup-uniform) every key of the tile is resident
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int r = srow + ps * RPP;
            const int64_t off = static_cast<int64_t>(bid[ps]) * blk_pitch + slab0 + (r & 15) * D + sc * 16;
            u32x4_t kt = u32x4_t{0u, 0u, 0u, 0u}, vt = u32x4_t{0u, 0u, 0u, 0u};
            if (stager && (whole || key0 + r < total)) { // keys >= c + n are never read: +0 (see the header)
                kt = *reinterpret_cast<const u32x4_t *>(kc + off);
                vt = *reinterpret_cast<const u32x4_t *>(vc + off);
            }
            kst[ps] = kt;
            vst[ps] = vt;
        }
    };
    auto commit_tile = [&]() {
        if (!stager) return;
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int r = srow + ps * RPP;
            vec8_t<T> lo, hi;
            fp8x16_to_t<T>(kst[ps], lo, hi);
            *reinterpret_cast<vec8_t<T> *>(&Ks[r * KRS + sc * 16]) = lo;
            *reinterpret_cast<vec8_t<T> *>(&Ks[r * KRS + sc * 16 + 8]) = hi;
            fp8x16_to_t<T>(vst[ps], lo, hi);
            *reinterpret_cast<vec8_t<T> *>(&Vs[r * VRS + sc * 16]) = lo;
            *reinterpret_cast<vec8_t<T> *>(&Vs[r * VRS + sc * 16 + 8]) = hi;
        }
    };

    const int kv_end = min(total, ctx + q0 + kPg8BQ);     // keys this q-block can see
    const int ntiles = (kv_end + kPg8BK - 1) / kPg8BK;

    // per-lane LDS offsets of the fragment reads
    const int k_frag_off = l32 * KRS + hf * 8;                            // + t*32*KRS + kk*16
    const int i16 = lane & 15;
    const int v_frag_off = (4 * hf + (i16 >> 2)) * VRS + 16 * ((lane >> 4) & 1) + 4 * (i16 & 3);

    load_ids(0);
    fetch_tile(0);
    if (ntiles > 1) load_ids(1);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int key0 = tile * kPg8BK;
        __syncthreads(); // everyone finished reading the previous tile
        commit_tile();
        __syncthreads();
        if (tile + 1 < ntiles) {
            fetch_tile(tile + 1);                        // in flight during the MFMAs below
            if (tile + 2 < ntiles) load_ids(tile + 2);   // ... and the block ids of the tile after it
        }

        if (key0 > qpos0w + 31) continue; // whole tile above this wave's diagonal

        // ---- S^T = K . Q^T  (two 32-key sub-tiles) ------------------------------------------------
        float16_t st[2];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            st[t] = float16_t{};
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) {
                const vec8_t<T> kf =
                    *reinterpret_cast<const vec8_t<T> *>(&Ks[k_frag_off + t * 32 * KRS + kk * 16]);
                st[t] = pg8_mfma32(kf, qf[kk], st[t]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        // S^T is read by VALU next, behind the diagonal-tile branch (swl_common.h)
        mfma_results_tie(st[0]);
        mfma_results_ready<8>(st[1]);
        // causal mask on the diagonal tiles (keys >= c + n are > every valid row's position as well)
        if (key0 + kPg8BK - 1 > qpos0w) {
            const int dmask = qpos - key0 - 4 * hf;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // key > qpos with key = key0 + 32 t + (r & 3) + 8 (r >> 2) + 4 hf: a compile-time constant against ONE
                    // per-lane value
                    if ((r & 3) + 8 * (r >> 2) + t * 32 > dmask) st[t][r] = kNegBig;
                }
        }
        // ---- online softmax: this lane owns chunk row l32, keys split with lane^32 -----------------
        float mx = st[0][0];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[t][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // lazy running maximum, decided per ROW (prefill_attn.hip): a row's arithmetic depends on its own scores only
        const float m_cand = fmaxf(m_run, mx * c);
        const float m_new = m_cand - m_run > kPg8LazyMax ? m_cand : m_run;
        const float alpha = fast_exp2(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = fast_exp2(fmaf(st[t][r], c, -m_new));
                st[t][r] = pv;
                psum += pv;
            }
        l_run = fmaf(l_run, alpha, psum);
        if (!__all(alpha == 1.0f)) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
        }

        // ---- O^T += V^T . P^T ------------------------------------------------------------------------
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                vec8_t<T> pb;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) pb[jj] = to_t<T>(st[t][8 * ks + jj]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const T *vp = &Vs[v_frag_off + (t * 32 + 16 * ks) * VRS + dt * 32];
                    const pg8_short4_t lo = pg8_lds_tr_read(vp);
                    const pg8_short4_t hi = pg8_lds_tr_read(vp + 8 * VRS);
                    typedef short short8_t __attribute__((ext_vector_type(8)));
                    const short8_t both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    const vec8_t<T> vf = __builtin_bit_cast(vec8_t<T>, both);
                    ot[dt] = pg8_mfma32(vf, pb, ot[dt]);
                }
            }
        __builtin_amdgcn_s_setprio(0);
    }

    // ---- epilogue: O[qrow][d] = O^T[d][qrow] / l, whole rows through LDS (prefill_attn_kernel) ------
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) mfma_results_tie(ot[dt]);
    mfma_results_ready<8>(ot[DT - 1]);
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;                  // (then v_scale, in fp32, before the one rounding)
    constexpr int ORS = D + 8;                       // O row pitch in LDS (elements)
    static_assert(4 * 32 * ORS <= kPg8BK * KRS + kPg8BK * VRS, "the four waves' O tiles must fit the K/V tiles' LDS");
    __syncthreads();                                 // every wave is done with the last K/V tile
    T *ow = smem + wave * 32 * ORS;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            typedef T vec4 __attribute__((ext_vector_type(4)));
            vec4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = to_t<T>((ot[dt][4 * r4 + e] * inv) * v_scale);
            *reinterpret_cast<vec4 *>(ow + l32 * ORS + dt * 32 + 8 * r4 + 4 * hf) = ov;
        }
    // (wave-private tile: LDS operations of one wave complete in order, no barrier needed)
    constexpr int RPI = 64 / CPR;                    // rows per store instruction
    T *obase = static_cast<T *>(p.o) + static_cast<int64_t>(start) * p.o_tok_stride + static_cast<int64_t>(head) * D;
#pragma unroll
    for (int i = 0; i < 32 / RPI; ++i) {
        const int row = i * RPI + lane / CPR, ch = lane % CPR;
        const vec8_t<T> v = *reinterpret_cast<const vec8_t<T> *>(ow + row * ORS + ch * 8);
        if (q0w + row < len)
            store8(obase + static_cast<int64_t>(q0w + row) * p.o_tok_stride + ch * 8, v);
    }
}

} // namespace swl

extern "C" int swl_prefill_attn_paged_fp8(void *o, const void *q, const void *k_cache, const void *v_cache,
                                          const float *kv_scales, const int32_t *block_table, const int32_t *seq_ids, const int32_t *cu_seqlens,
                                      const int32_t *ctx_lens, int32_t num_prefill_seqs, int32_t max_new_len,
                                      int32_t max_total_len, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                                      int32_t num_layers, int32_t block_size, int32_t cur_layer,
                                      int32_t max_blocks_per_seq, float softmax_scale, int64_t q_tok_stride,
                                      int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    if (num_prefill_seqs < 0 || max_new_len < 0 || max_total_len < 0) return SWL_ERR_BAD_ARG;
    if (num_prefill_seqs == 0 || max_new_len == 0) return SWL_OK;
    if (!o || !q || !k_cache || !v_cache || !kv_scales || !block_table || !seq_ids || !cu_seqlens || !ctx_lens) return SWL_ERR_BAD_ARG;
    if (num_q_heads <= 0 || num_kv_heads <= 0 || num_q_heads % num_kv_heads != 0) return SWL_ERR_BAD_ARG;
    if (num_layers <= 0 || cur_layer < 0 || cur_layer >= num_layers || max_blocks_per_seq <= 0 || block_size <= 0)
        return SWL_ERR_BAD_ARG;
    if (max_total_len < max_new_len) return SWL_ERR_BAD_ARG;
    if (!(head_dim == 32 || head_dim == 64 || head_dim == 128)) return SWL_ERR_BAD_ARG;
    if (!(dtype == SWL_F16 || dtype == SWL_BF16)) return SWL_ERR_BAD_ARG;
    if (block_size != swl::kPg8Blk) return SWL_ERR_UNSUPPORTED;
    // the longest sequence must fit a block-table row (the kernel reads ceil(total / 16) entries of it)
    if ((static_cast<int64_t>(max_total_len) + block_size - 1) / block_size > max_blocks_per_seq) return SWL_ERR_BAD_ARG;
    if ((q_tok_stride & 7) || (o_tok_stride & 7) || q_tok_stride < static_cast<int64_t>(num_q_heads) * head_dim ||
        o_tok_stride < static_cast<int64_t>(num_q_heads) * head_dim)
        return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(q) || !swl::aligned16(o) || !swl::aligned16(k_cache) || !swl::aligned16(v_cache))
        return SWL_ERR_BAD_ARG;
    swl::PagedPrefillFp8Params p;
    p.o = o;
    p.q = q;
    p.k_cache = static_cast<const uint8_t *>(k_cache);
    p.v_cache = static_cast<const uint8_t *>(v_cache);
    p.kv_scales = kv_scales;
    p.block_table = block_table;
    p.seq_ids = seq_ids;
    p.cu_seqlens = cu_seqlens;
    p.ctx_lens = ctx_lens;
    p.num_seqs = num_prefill_seqs;
    p.H = num_q_heads;
    p.KVH = num_kv_heads;
    p.num_q_blocks = (max_new_len + swl::kPg8BQ - 1) / swl::kPg8BQ;
    p.num_layers = num_layers;
    p.cur_layer = cur_layer;
    p.max_blocks_per_seq = max_blocks_per_seq;
    p.scale_log2e = softmax_scale * 1.44269504088896340736f;
    p.q_tok_stride = q_tok_stride;
    p.o_tok_stride = o_tok_stride;
    const int64_t units = static_cast<int64_t>(num_prefill_seqs) * num_kv_heads;
    const int64_t units_padded = (units + 7) / 8 * 8;
    const int G = num_q_heads / num_kv_heads;
    const int64_t nblocks = units_padded * G * p.num_q_blocks;
    if (nblocks > 0x7fffffffLL) return SWL_ERR_UNSUPPORTED;
    const dim3 grid(static_cast<unsigned>(nblocks));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SWL_DISPATCH_DTYPE(dtype, T, {
        if (head_dim == 128)
            hipLaunchKernelGGL((swl::prefill_attn_paged_fp8_kernel<T, 128>), grid, dim3(256), 0, s, p);
        else if (head_dim == 64)
            hipLaunchKernelGGL((swl::prefill_attn_paged_fp8_kernel<T, 64>), grid, dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((swl::prefill_attn_paged_fp8_kernel<T, 32>), grid, dim3(256), 0, s, p);
    });
    return swl::check_launch();
}
