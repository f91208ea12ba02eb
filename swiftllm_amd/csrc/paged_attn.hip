// paged_attn.hip — decode-stage paged attention ("paged attention v2" / flash-decoding) for gfx950.
//
// Replaces _fwd_paged_attention_phase1 (swiftllm/worker/kernels/paged_attn.py:9-108) and
// _fwd_paged_attention_phase2 (paged_attn.py:111-149). The north-star kernel: HBM-bound,
// algorithmic bytes per call = sum_i len_i * 2 * KVH * D * e  (every KV byte ONCE per kv-head)
// + q/o (2*Bd*H*D*e) + partials.
//
// Design (MI355X-first, not the reference's one-warp-per-q-head mapping):
//   * grid (seq-block, kv-head, sequence); a workgroup = 4 or 8 waves serves ALL G = H/KVH q-heads of
//     its kv-head, so a KV tile is fetched once instead of G times (the reference leans on L2 for
//     that). The host sizes the sequence block so a launch is ~one 8-wave workgroup per CU in whole
//     rounds (batch_plan.select_seq_block_size); with one sequence block the output is written
//     directly and phase 2 is not launched at all;
//   * the 16-token x D tile of one (block, layer, kv-head) is 4 KiB contiguous in the pool; a wave
//     reads it with fully coalesced 16-byte-per-lane loads (lane -> token = i*TPI + lane/LPT,
//     8-element chunk = lane%LPT), 1 KiB per instruction, non-temporal (read once);
//   * waves stride over the 16-token blocks of the sequence block; the next block's K and V (8 KiB
//     per wave) are in flight while the current one is consumed (register double buffering);
//   * q.k partial dots with v_dot2c_f32_{f16,bf16} (fp32 accumulate), reduced across the LPT lanes
//     of a token with DPP adds — no LDS, no ds_bpermute in the main loop;
//   * every LPT-lane row keeps its own online-softmax state (max, sum, 8-wide slice of the
//     accumulator for each of the G heads) so nothing crosses rows until the end; rows are merged
//     once per workgroup with wave shuffles, waves once through 8 KiB of LDS;
//   * block-table entries are scalar loads (the wave index is made provably uniform);
//   * scores are kept UNscaled; scale*log2(e) is folded into the exp2 argument with one fma.
// Numerics: fp32 scores/softmax/accumulation (the reference rounds scores to fp16,
// paged_attn.py:72-73; ours is closer to the exact value). Partials use the reference's format:
// mid_o = acc/sum (normalised), mid_lse = log2(sum) + max in the scaled base-2 domain
// (paged_attn.py:106-108), so phase 1 can be compared with the reference's phase 1 directly.
#include "decode_attn.h"

namespace swl {

struct PagedAttnParams : DecodeAttnParams {
    // QKV variant: q/k/v of the new token are still the split-K partial slabs of the fused qkv projection
    const float *qkv_slabs; // [ks][Bd][(H + 2*KVH) * D] fp32
    int ks;
    const void *cos_t, *sin_t; // rope tables [positions][D/2]
    const int *pos_idx;        // table row per sequence (NULL: seq_len - 1)
    // deferred RMSNorm (rmsnorm.hip, splitk_add_scale_kernel): the qkv projection ran on un-normalised activations;
    // its fp32 slab sums are multiplied by rstd[seq] = 1/sqrt(sum_p row_ssq[p][seq] / hidden + eps) before their rounding
    const float *row_ssq; // [ssq_parts][Bd], NULL = the slabs are final
    int ssq_parts, hidden;
    float eps;
};

// Ring depth of the K/V register pipeline: a wave keeps kPaDepth 16-token blocks (K + V = 8 KiB, 32 VGPRs each)
// resident — the one it attends plus kPaDepth-1 in flight. Little's law on this part: one CU needs ~31 GB/s
// (8 TB/s / 256) against ~2 us of loaded HBM latency = ~64 KB in flight; 8 waves x 1 block in flight (depth 2) is
// exactly that with nothing to spare, depth 3 doubles it. (r02 A/B builds of deeper rings and of an L2 look-ahead touch
// lost or tied — profiles/r02g_paged_attn_mfma.md; the knobs are gone, the numbers stay there.)
constexpr int kPaMfmaDepth = 2;   // matrix-core path (G >= 2): measured best on MI355X (profiles/r02g_paged_attn_mfma.md)

// NW = waves per workgroup: 4 for short sequence blocks (latency-bound launches that want many
// small workgroups), 8 for long ones (one workgroup per CU, every wave streams many KV blocks and the
// per-workgroup prologue/merge is amortised; 8 waves x 16 KiB of K/V in flight per CU).
//
// QKV = true: the rotary + KV-store step of the layer (rotary_emb.py + kvcache_mgmt.py:50-79) runs in this
// kernel's prologue instead of a launch of its own. The workgroup sums the fused-qkv slabs of its G query
// heads and its kv head, rotates q and k (same arithmetic and rounding as rotary.hip), keeps the rounded q in
// LDS for its waves, and — in the split that owns the last position — writes the new k/v into the pool and
// patches them into the registers of the wave that attends that block (the pool read raced with the write).
template <typename T, int D, int G, int NW, bool QKV = false>
// block_table / seq_lens / seq_ids are passed a second time as __restrict__ kernel arguments: the QKV variant
// stores into the pools before its main loop, and without the no-alias guarantee the compiler must assume those
// stores clobber the block table — it then fetches bt[b] with a VECTOR load and waits vmcnt(0) for it, draining
// the whole K/V ring on every refill (seen in the ISA; the plain variant has no stores and got s_load all along).
__global__ __launch_bounds__(NW * 64) void paged_attn_phase1_kernel(PagedAttnParams p,
                                                                    const int *__restrict__ block_table,
                                                                    const int *__restrict__ seq_lens_r,
                                                                    const int *__restrict__ seq_ids_r) {
    using Tile = DecodeTile<T, D, G>;
    constexpr int LPT = Tile::LPT, TPI = Tile::TPI, NI = Tile::NI;
    __shared__ float sm_ml[NW][G][2];
    __shared__ float sm_acc[NW][G][D];
    __shared__ __attribute__((aligned(16))) T sm_q[QKV ? G * D : 8];
    __shared__ __attribute__((aligned(16))) T sm_kv[QKV ? 2 * D : 8];
    constexpr bool MF = G >= 2;          // matrix-core attend_block (see attend_block_mfma)
    using MT = MfmaTile<T, D>;
    __shared__ __attribute__((aligned(16))) T sm_stage[MF ? NW : 1][MF ? MT::ELEMS : 8];

    const int split = blockIdx.x;
    const int kvh = blockIdx.y;
    const int seq = blockIdx.z;
    const int len = seq_lens_r[seq];
    const int tok_begin = split * p.seq_block_size;
    if (tok_begin >= len) return; // uniform for the workgroup, before any barrier
    const int tok_end = min(len, tok_begin + p.seq_block_size);
    const int blk_end = (tok_end + kBlk - 1) / kBlk;
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

    vec8_t<T> qv[MF ? 1 : G];
    vec8_t<T> qb[MT::QS];               // MF: Q^T B fragments, lane (q, h) -> Q[head h][32 j + 8 q ..], zero for h >= G
    const int mq = lane >> 4, mh = lane & 15;
    if constexpr (!QKV) {
        if constexpr (MF) {
            const T *qp = static_cast<const T *>(p.q) + seq * p.q_tok_stride +
                          (static_cast<int64_t>(kvh) * G + min(mh, G - 1)) * D + 8 * mq;
#pragma unroll
            for (int j = 0; j < MT::QS; ++j) {
                qb[j] = load8(qp + 32 * j);
                if (mh >= G) qb[j] = vec8_t<T>{};
            }
        } else {
            const T *qp = static_cast<const T *>(p.q) + seq * p.q_tok_stride +
                          static_cast<int64_t>(kvh) * G * D + chunk * 8;
#pragma unroll
            for (int g = 0; g < G; ++g) qv[g] = load8(qp + g * D);
        }
    }
    const int pos = len - 1;          // the token being decoded
    const int last_blk = pos / kBlk;

    float m[MF ? 1 : G], l[MF ? 1 : G], acc[MF ? 1 : G][8];
    float4_t acc4[MT::OS];              // MF: O^T[d = 16 mm + 4 q + r][head h]

    // ring slots: what the 256-VGPR budget of a 2-waves-per-SIMD kernel holds without spilling: 4 for the VALU path
    // (G = 1), kPaMfmaDepth for the matrix-core path (D/16 x 4 accumulator registers whatever G is)
    constexpr int ND = G == 1 ? 4 : kPaMfmaDepth;
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
        if constexpr (MF)
            attend_block_mfma<T, D, G>(qb, Kd, Vd, m[0], l[0], acc4, &sm_stage[wave][0], c, tok0, row, chunk, lane, len,
                                       tok0 + kBlk > len);
        else
            attend_block<T, D, G>(qv, Kd, Vd, m, l, acc, c, tok0, row, len, tok0 + kBlk > len);
    };
    // Drain steps only (a wave's last block is always attended there): in the QKV variant the block that holds the
    // token being decoded takes that token's k/v from the prologue's LDS copy — its pool read raced with the store.
    // Kept out of the steady loop: the per-lane patch costs registers the ring needs.
    auto attend_tail = [&](int b, vec8_t<T>(&Kd)[NI], vec8_t<T>(&Vd)[NI]) {
        if constexpr (QKV) {
            const int tok0 = b * kBlk;
            if (b == last_blk) {
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (tok0 + i * TPI + row == pos) {
                        Kd[i] = *reinterpret_cast<const vec8_t<T> *>(&sm_kv[chunk * 8]);
                        Vd[i] = *reinterpret_cast<const vec8_t<T> *>(&sm_kv[D + chunk * 8]);
                    }
            }
        }
        attend(b, Kd, Vd);
    };
    // the first ND blocks of this wave go into slots 0..ND-1 (QKV: issued from inside the prologue)
    auto prefetch_kv = [&](int b0, auto lo_tag, auto hi_tag) {
        kv_ring_prefetch<decltype(lo_tag)::value, decltype(hi_tag)::value, NW>(b0, blk_end, bt, Kr, Vr, load_phys);
    };
    constexpr int NDP = ND < 2 ? ND : 2;    // QKV: slots requested while the slab loads of the prologue are pending

    int b = tok_begin / kBlk + wave;
    if constexpr (!QKV) {
        prefetch_kv(b, IntTag<0>{}, IntTag<ND>{});
    } else {
        // Prologue order matters (loads return in order within a wave): a thread first REQUESTS the slabs of its
        // item, then its wave requests two KV blocks (16 KiB, the stream is running), and only then the item is
        // finished — the slab data never queues behind 16 KiB of KV, and no wave delays its KV requests.
        constexpr int kRot = D / 16;       // rotation items per head
        const bool owner = tok_end == len; // the split that attends (and stores) the new token
        const int n_items = G * kRot + (owner ? kRot + D / 8 : 0); // <= one per thread
        const int64_t qkv_row = static_cast<int64_t>(p.H + 2 * p.KVH) * D;
        const int64_t slab_stride = static_cast<int64_t>(gridDim.z) * qkv_row;
        const int64_t row_off = seq * qkv_row;
        const int item = threadIdx.x;
        const bool has = item < n_items;
        const bool is_rot = item < (G + 1) * kRot;
        const bool is_q = item < G * kRot;
        const int c = is_rot ? item % kRot : item - (G + 1) * kRot;
        const int head = is_q ? kvh * G + item / kRot : (is_rot ? p.H + kvh : p.H + p.KVH + kvh);
        const int64_t off = row_off + static_cast<int64_t>(head) * D + c * 8;
        auto finish = [&](vec8_t<T> x0, vec8_t<T> x1, const vec8_t<T> &cv, const vec8_t<T> &sv) {
            if (is_rot) {
                rotate8<T>(x0, x1, cv, sv);
                T *dst = is_q ? &sm_q[(item / kRot) * D] : &sm_kv[0];
                *reinterpret_cast<vec8_t<T> *>(dst + c * 8) = x0;
                *reinterpret_cast<vec8_t<T> *>(dst + D / 2 + c * 8) = x1;
                if (!is_q) {
                    T *pool = const_cast<T *>(kc) + (static_cast<int64_t>(bt[last_blk]) * blk_pitch + layer_head) *
                                                        tile_elems + (pos % kBlk) * D;
                    store8(pool + c * 8, x0);
                    store8(pool + D / 2 + c * 8, x1);
                }
            } else {
                *reinterpret_cast<vec8_t<T> *>(&sm_kv[D + c * 8]) = x0;
                T *pool = const_cast<T *>(vc) + (static_cast<int64_t>(bt[last_blk]) * blk_pitch + layer_head) *
                                                    tile_elems + (pos % kBlk) * D;
                store8(pool + c * 8, x0);
            }
        };
        auto prologue = [&](auto ks_tag) {
            constexpr int KS = decltype(ks_tag)::value;
            float4_t a0[KS], b0[KS], a1[KS], b1[KS];
            vec8_t<T> cv = {}, sv = {};
            float ssv[8];
            const bool row_scaled = p.row_ssq != nullptr; // (uniform; same memory round trip as the slabs)
            if (row_scaled) {
#pragma unroll
                for (int q2 = 0; q2 < 8; ++q2)
                    ssv[q2] = q2 < p.ssq_parts ? p.row_ssq[q2 * static_cast<int>(gridDim.z) + seq] : 0.f;
            }
            if (has) {
                const float *s0 = p.qkv_slabs + off;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    a0[k] = *reinterpret_cast<const float4_t *>(s0 + k * slab_stride);
                    b0[k] = *reinterpret_cast<const float4_t *>(s0 + k * slab_stride + 4);
                }
                if (is_rot) {
                    const int64_t trow = p.pos_idx ? p.pos_idx[seq] : pos;
                    cv = load8(static_cast<const T *>(p.cos_t) + trow * (D / 2) + c * 8);
                    sv = load8(static_cast<const T *>(p.sin_t) + trow * (D / 2) + c * 8);
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        a1[k] = *reinterpret_cast<const float4_t *>(s0 + D / 2 + k * slab_stride);
                        b1[k] = *reinterpret_cast<const float4_t *>(s0 + D / 2 + k * slab_stride + 4);
                    }
                }
            }
            prefetch_kv(b, IntTag<0>{}, IntTag<NDP>{});
            if (has) {
                // slab order, one rounding: the bits of load8_splitk / the stand-alone reduce kernel
                float4_t sa0 = {0.f, 0.f, 0.f, 0.f}, sb0 = sa0, sa1 = sa0, sb1 = sa0;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    sa0 += a0[k];
                    sb0 += b0[k];
                }
                if (is_rot) {
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        sa1 += a1[k];
                        sb1 += b1[k];
                    }
                }
                float rs = 1.0f; // (x * 1.0f is exact: one code path)
                if (row_scaled) {
                    const float ss = ((ssv[0] + ssv[1]) + (ssv[2] + ssv[3])) + ((ssv[4] + ssv[5]) + (ssv[6] + ssv[7]));
                    rs = 1.0f / sqrtf(ss / static_cast<float>(p.hidden) + p.eps);
                }
                vec8_t<T> x0, x1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    x0[e] = static_cast<T>(sa0[e] * rs);
                    x0[4 + e] = static_cast<T>(sb0[e] * rs);
                    x1[e] = static_cast<T>(sa1[e] * rs);
                    x1[4 + e] = static_cast<T>(sb1[e] * rs);
                }
                finish(x0, x1, cv, sv);
            }
        };
        if (p.ks == 4) prologue(IntTag<4>{});
        else if (p.ks == 2) prologue(IntTag<2>{});
        else if (p.ks == 1) prologue(IntTag<1>{});
        else { // many slabs: too many registers to hold them raw — KV first, then the summing loads
            prefetch_kv(b, IntTag<0>{}, IntTag<NDP>{});
            if (has) {
                vec8_t<T> cv = {}, sv = {}, x1 = {};
                vec8_t<T> x0 = load8_splitk<T>(p.qkv_slabs, p.ks, slab_stride, off);
                if (is_rot) {
                    const int64_t trow = p.pos_idx ? p.pos_idx[seq] : pos;
                    cv = load8(static_cast<const T *>(p.cos_t) + trow * (D / 2) + c * 8);
                    sv = load8(static_cast<const T *>(p.sin_t) + trow * (D / 2) + c * 8);
                    x1 = load8_splitk<T>(p.qkv_slabs, p.ks, slab_stride, off + D / 2);
                }
                finish(x0, x1, cv, sv);
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // do not hoist the next requests above the slab sums (register pressure)
        prefetch_kv(b, IntTag<NDP>{}, IntTag<ND>{}); // the remaining slots: the slab registers are free again
        __syncthreads();
        if constexpr (MF) {
#pragma unroll
            for (int j = 0; j < MT::QS; ++j) {
                qb[j] = *reinterpret_cast<const vec8_t<T> *>(&sm_q[min(mh, G - 1) * D + 32 * j + 8 * mq]);
                if (mh >= G) qb[j] = vec8_t<T>{};
            }
        } else {
#pragma unroll
            for (int g = 0; g < G; ++g) qv[g] = *reinterpret_cast<const vec8_t<T> *>(&sm_q[g * D + chunk * 8]);
        }
    }
#pragma unroll
    for (int g = 0; g < (MF ? 1 : G); ++g) {
        m[g] = kNegBig;
        l[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
    }
#pragma unroll
    for (int mm = 0; mm < MT::OS; ++mm) acc4[mm] = float4_t{0.f, 0.f, 0.f, 0.f};
    kv_ring_stream<ND, NW>(b, blk_end, bt, Kr, Vr, load_phys, attend, attend_tail);

    if constexpr (MF) {
        mfma_wave_finish(m[0], l[0], acc4, sm_ml, sm_acc, wave, lane);
    } else {
    // ---- merge the TPI rows of this wave (each row holds tokens == row mod TPI) ----------------
#pragma unroll
    for (int mask = LPT; mask < 64; mask <<= 1) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float m2 = __shfl_xor(m[g], mask, 64);
            const float l2 = __shfl_xor(l[g], mask, 64);
            const float M = fmaxf(m[g], m2);
            const float w1 = fast_exp2((m[g] - M) * c);
            const float w2 = fast_exp2((m2 - M) * c);
            l[g] = l[g] * w1 + l2 * w2;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float a2 = __shfl_xor(acc[g][j], mask, 64);
                acc[g][j] = acc[g][j] * w1 + a2 * w2;
            }
            m[g] = M;
        }
    }
    if (row == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (chunk == 0) {
                sm_ml[wave][g][0] = m[g];
                sm_ml[wave][g][1] = l[g];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) sm_acc[wave][g][chunk * 8 + j] = acc[g][j];
        }
    }
    } // !MF
    __syncthreads();

    merge_waves_write<T, D, G, NW, false>(p, sm_ml, sm_acc, c, 1.0f, kvh, seq, split);
}

// grid (H, Bd), one wave per (sequence, q-head): LSE-weighted merge of the partials (reference paged_attn.py:
// 108-150). Latency is all there is to this kernel (n <= a few dozen partials of 512 B each), so nothing in it may
// serialise on memory: the n log-sum-exps arrive in ONE load (lane s holds partial s), the weights are computed once
// per lane and handed out with v_readlane, and the partial outputs are requested eight at a time before the first
// FMA — two round trips in all. (r01: one dependent load pair per partial, 10.9 us at 16 partials = more than the
// attention itself at batch 1; profiles/r02d.) The weighted sum keeps the partial order.
template <typename T, int D>
__global__ __launch_bounds__(64) void paged_attn_phase2_kernel(
    T *__restrict__ o, const float *__restrict__ mid_o, const float *__restrict__ mid_lse,
    const int *__restrict__ seq_lens, int H, int seq_block_size, int num_seq_blocks,
    int64_t o_tok_stride) {
    const int head = blockIdx.x;
    const int seq = blockIdx.y;
    const int lane = threadIdx.x;
    const int len = seq_lens[seq];
    if (len <= 0) return; // an inert row of a padded decode batch: phase 1 wrote no partials for it
    const int n = (len + seq_block_size - 1) / seq_block_size;
    const int64_t base = (static_cast<int64_t>(seq) * H + head) * num_seq_blocks;
    constexpr int VD = (D + 63) / 64;
    constexpr int U = 8;

    // first requests: the log-sum-exps of up to 64 partials and the first U partial outputs
    float lse = lane < n ? mid_lse[base + lane] : kNegBig;
    float v[U][VD];
    auto request = [&](int s0) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < VD; ++q) {
                const int d = lane + q * 64;
                v[u][q] = (s0 + u < n && d < D) ? mid_o[(base + s0 + u) * D + d] : 0.f;
            }
    };
    request(0);
    float M = lse;
    for (int s = lane + 64; s < n; s += 64) M = fmaxf(M, mid_lse[base + s]); // (> 64 partials: 128k-token sequences)
    M = wave_allreduce_max(M);

    float acc[VD];
#pragma unroll
    for (int q = 0; q < VD; ++q) acc[q] = 0.f;
    float Lsum = 0.f;
    for (int c0 = 0; c0 < n; c0 += 64) {
        if (c0 > 0) lse = c0 + lane < n ? mid_lse[base + c0 + lane] : kNegBig;
        const float w_lane = c0 + lane < n ? fast_exp2(lse - M) : 0.f;
        Lsum += w_lane;
        const int lim = min(64, n - c0);
        for (int s0 = 0; s0 < lim; s0 += U) {
            if (c0 + s0 > 0) request(c0 + s0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // lanes beyond the last partial hold w = 0 and v = 0: no guard needed
                const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w_lane),
                                                                                    (s0 + u) & 63));
#pragma unroll
                for (int q = 0; q < VD; ++q) acc[q] = fmaf(w, v[u][q], acc[q]);
            }
        }
    }
    Lsum = wave_allreduce_sum(Lsum);
#pragma unroll
    for (int q = 0; q < VD; ++q) {
        const int d = lane + q * 64;
        if (d < D) o[seq * o_tok_stride + static_cast<int64_t>(head) * D + d] = to_t<T>(acc[q] / Lsum);
    }
}

template <typename T, bool QKV>
static int launch_phase1(const PagedAttnParams &p, const int *bt, const int *lens, const int *ids, int Bd, int D,
                         hipStream_t stream) {
    return dispatch_decode_attn(D, p.H / p.KVH, p.seq_block_size, [&](auto d, auto g, auto nw) {
        constexpr int NW = decltype(nw)::value;
        hipLaunchKernelGGL((paged_attn_phase1_kernel<T, decltype(d)::value, decltype(g)::value, NW, QKV>),
                           dim3(p.num_seq_blocks, p.KVH, Bd), dim3(NW * 64), 0, stream, p, bt, lens, ids);
        return check_launch();
    });
}

template <typename T>
static int dispatch_phase2(T *o, const float *mid_o, const float *mid_lse, const int *seq_lens,
                           int Bd, int H, int D, int sbs, int nsb, int64_t o_tok_stride,
                           hipStream_t stream) {
    const dim3 grid(H, Bd);
#define SWL_P2(DD)                                                                               \
    hipLaunchKernelGGL((paged_attn_phase2_kernel<T, DD>), grid, dim3(64), 0, stream, o, mid_o,   \
                       mid_lse, seq_lens, H, sbs, nsb, o_tok_stride)
    switch (D) {
    case 32: SWL_P2(32); break;
    case 64: SWL_P2(64); break;
    case 128: SWL_P2(128); break;
    default: return SWL_ERR_UNSUPPORTED;
    }
#undef SWL_P2
    return check_launch();
}

} // namespace swl

extern "C" size_t swl_paged_attn_scratch_bytes(int32_t num_decoding_seqs, int32_t num_q_heads,
                                               int32_t head_dim, int32_t num_seq_blocks) {
    if (num_decoding_seqs <= 0 || num_q_heads <= 0 || head_dim <= 0 || num_seq_blocks <= 0) return 0;
    const size_t parts = static_cast<size_t>(num_decoding_seqs) * num_q_heads * num_seq_blocks;
    return parts * (static_cast<size_t>(head_dim) + 1) * sizeof(float);
}

extern "C" int swl_paged_attn_phase1(void *o_direct, const void *q, const void *k_cache,
                                     const void *v_cache, const int32_t *block_table,
                                     const int32_t *seq_ids, const int32_t *seq_lens, float *mid_o,
                                     float *mid_lse, float softmax_scale, int32_t num_decoding_seqs,
                                     int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                                     int32_t num_layers, int32_t block_size, int32_t cur_layer,
                                     int32_t max_blocks_per_seq, int32_t seq_block_size,
                                     int32_t num_seq_blocks, int64_t q_tok_stride,
                                     int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    if (num_decoding_seqs < 0) return SWL_ERR_BAD_ARG;
    if (num_decoding_seqs == 0 || num_seq_blocks == 0) return SWL_OK;
    if (!q || !k_cache || !v_cache || !block_table || !seq_ids || !seq_lens) return SWL_ERR_BAD_ARG;
    const swl::DecodeAttnArgs a{o_direct, q, k_cache, v_cache, q_tok_stride, o_tok_stride, num_q_heads, num_kv_heads,
                                head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq, seq_block_size,
                                num_seq_blocks};
    if (const int rc = swl::check_decode_geometry(a)) return rc;
    if (const int rc = swl::check_decode_layout(a)) return rc;
    if (!swl::phase1_outputs_ok(o_direct, mid_o, mid_lse, num_seq_blocks)) return SWL_ERR_BAD_ARG;
    if (!swl::decode_grid_fits(num_decoding_seqs, num_kv_heads)) return SWL_ERR_UNSUPPORTED;
    swl::PagedAttnParams p{};
    swl::fill_decode_params(p, a, mid_o, mid_lse, softmax_scale);
    SWL_DISPATCH_DTYPE(dtype, T, {
        return swl::launch_phase1<T, false>(p, block_table, seq_lens, seq_ids, num_decoding_seqs, head_dim,
                                            static_cast<hipStream_t>(stream));
    });
}

extern "C" int swl_paged_attn_phase2(void *o, const float *mid_o, const float *mid_lse,
                                     const int32_t *seq_lens, int32_t num_decoding_seqs,
                                     int32_t num_q_heads, int32_t head_dim, int32_t seq_block_size,
                                     int32_t num_seq_blocks, int64_t o_tok_stride, int32_t dtype,
                                     swl_stream_t stream) {
    if (num_decoding_seqs < 0) return SWL_ERR_BAD_ARG;
    if (num_decoding_seqs == 0 || num_seq_blocks == 0) return SWL_OK;
    if (!o || !mid_o || !mid_lse || !seq_lens || num_q_heads <= 0 || seq_block_size <= 0 ||
        num_seq_blocks < 0)
        return SWL_ERR_BAD_ARG;
    if (!(head_dim == 32 || head_dim == 64 || head_dim == 128)) return SWL_ERR_UNSUPPORTED;
    if (!swl::aligned16(o) || (o_tok_stride & 7) || o_tok_stride < static_cast<int64_t>(num_q_heads) * head_dim ||
        ((reinterpret_cast<uintptr_t>(mid_o) | reinterpret_cast<uintptr_t>(mid_lse)) & 3u))
        return SWL_ERR_BAD_ARG;
    if (num_decoding_seqs > 65535) return SWL_ERR_UNSUPPORTED;
    SWL_DISPATCH_DTYPE(dtype, T, {
        return swl::dispatch_phase2<T>(static_cast<T *>(o), mid_o, mid_lse, seq_lens,
                                       num_decoding_seqs, num_q_heads, head_dim, seq_block_size,
                                       num_seq_blocks, o_tok_stride,
                                       static_cast<hipStream_t>(stream));
    });
}

extern "C" int swl_paged_attn_decode(void *o, const void *q, const void *k_cache,
                                     const void *v_cache, const int32_t *block_table,
                                     const int32_t *seq_ids, const int32_t *seq_lens, void *scratch,
                                     float softmax_scale, int32_t num_decoding_seqs,
                                     int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                                     int32_t num_layers, int32_t block_size, int32_t cur_layer,
                                     int32_t max_blocks_per_seq, int32_t seq_block_size,
                                     int32_t num_seq_blocks, int64_t q_tok_stride,
                                     int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    if (num_decoding_seqs < 0) return SWL_ERR_BAD_ARG;
    if (num_decoding_seqs == 0 || num_seq_blocks == 0) return SWL_OK;
    if (!o) return SWL_ERR_BAD_ARG;
    float *mid_o, *mid_lse;
    if (!swl::split_scratch(scratch, num_decoding_seqs, num_q_heads, head_dim, num_seq_blocks, mid_o, mid_lse))
        return SWL_ERR_BAD_ARG;
    int rc = swl_paged_attn_phase1(o, q, k_cache, v_cache, block_table, seq_ids, seq_lens, mid_o,
                                   mid_lse, softmax_scale, num_decoding_seqs, num_q_heads,
                                   num_kv_heads, head_dim, num_layers, block_size, cur_layer,
                                   max_blocks_per_seq, seq_block_size, num_seq_blocks, q_tok_stride,
                                   o_tok_stride, dtype, stream);
    if (rc != SWL_OK || num_seq_blocks == 1) return rc;
    return swl_paged_attn_phase2(o, mid_o, mid_lse, seq_lens, num_decoding_seqs, num_q_heads,
                                 head_dim, seq_block_size, num_seq_blocks, o_tok_stride, dtype,
                                 stream);
}

/* Decode attention fed by the split-K slabs of the fused qkv projection: rotary + KV-store of the new token run
 * in the attention kernel's prologue (no launch of their own), the new k/v are attended from registers. */
static int paged_attn_decode_qkv_impl(void *o, const float *qkv_slabs, int32_t k_splits, const void *cos_table,
                                         const void *sin_table, const int32_t *pos_idx, void *k_cache,
                                         void *v_cache, const int32_t *block_table, const int32_t *seq_ids,
                                         const int32_t *seq_lens, void *scratch, float softmax_scale,
                                         int32_t num_decoding_seqs, int32_t num_q_heads, int32_t num_kv_heads,
                                         int32_t head_dim, int32_t num_layers, int32_t block_size,
                                         int32_t cur_layer, int32_t max_blocks_per_seq, int32_t seq_block_size,
                                         int32_t num_seq_blocks, int64_t o_tok_stride, int32_t dtype,
                                         swl_stream_t stream, const float *row_ssq, int32_t ssq_parts, int32_t hidden,
                                         float eps, bool merge) {
    if (num_decoding_seqs < 0) return SWL_ERR_BAD_ARG;
    if (num_decoding_seqs == 0 || num_seq_blocks == 0) return SWL_OK;
    if ((!o && (merge || num_seq_blocks == 1)) || !qkv_slabs || !cos_table || !sin_table || !k_cache || !v_cache ||
        !block_table || !seq_ids || !seq_lens || k_splits <= 0)
        return SWL_ERR_BAD_ARG;
    const swl::DecodeAttnArgs a{o, qkv_slabs, k_cache, v_cache, 0, o_tok_stride, num_q_heads, num_kv_heads, head_dim,
                                num_layers, block_size, cur_layer, max_blocks_per_seq, seq_block_size, num_seq_blocks};
    if (const int rc = swl::check_decode_geometry(a)) return rc;
    if (const int rc = swl::check_decode_layout(a, false)) return rc;
    if (!swl::aligned16(cos_table) || !swl::aligned16(sin_table)) return SWL_ERR_BAD_ARG;
    if (!swl::decode_grid_fits(num_decoding_seqs, num_kv_heads)) return SWL_ERR_UNSUPPORTED;
    float *mid_o, *mid_lse;
    if (!swl::split_scratch(scratch, num_decoding_seqs, num_q_heads, head_dim, num_seq_blocks, mid_o, mid_lse))
        return SWL_ERR_BAD_ARG;
    swl::PagedAttnParams p{};
    swl::fill_decode_params(p, a, mid_o, mid_lse, softmax_scale);
    p.qkv_slabs = qkv_slabs;
    p.ks = k_splits;
    p.cos_t = cos_table;
    p.sin_t = sin_table;
    p.pos_idx = pos_idx;
    p.row_ssq = row_ssq;
    p.ssq_parts = ssq_parts;
    p.hidden = hidden;
    p.eps = eps;
    int rc;
    SWL_DISPATCH_DTYPE(dtype, T, {
        rc = swl::launch_phase1<T, true>(p, block_table, seq_lens, seq_ids, num_decoding_seqs, head_dim,
                                         static_cast<hipStream_t>(stream));
    });
    if (rc != SWL_OK || num_seq_blocks == 1 || !merge) return rc;
    return swl_paged_attn_phase2(o, mid_o, mid_lse, seq_lens, num_decoding_seqs, num_q_heads, head_dim,
                                 seq_block_size, num_seq_blocks, o_tok_stride, dtype, stream);
}

extern "C" int swl_paged_attn_decode_qkv(void *o, const float *qkv_slabs, int32_t k_splits, const void *cos_table,
                                         const void *sin_table, const int32_t *pos_idx, void *k_cache,
                                         void *v_cache, const int32_t *block_table, const int32_t *seq_ids,
                                         const int32_t *seq_lens, void *scratch, float softmax_scale,
                                         int32_t num_decoding_seqs, int32_t num_q_heads, int32_t num_kv_heads,
                                         int32_t head_dim, int32_t num_layers, int32_t block_size,
                                         int32_t cur_layer, int32_t max_blocks_per_seq, int32_t seq_block_size,
                                         int32_t num_seq_blocks, int64_t o_tok_stride, int32_t dtype,
                                         swl_stream_t stream) {
    return paged_attn_decode_qkv_impl(o, qkv_slabs, k_splits, cos_table, sin_table, pos_idx, k_cache, v_cache, block_table,
                                      seq_ids, seq_lens, scratch, softmax_scale, num_decoding_seqs, num_q_heads,
                                      num_kv_heads, head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq,
                                      seq_block_size, num_seq_blocks, o_tok_stride, dtype, stream, nullptr, 0, 0, 0.f,
                                      true);
}

/* swl_paged_attn_decode_qkv on the slabs of a qkv projection whose input had its RMSNorm scale deferred
 * (swl_splitk_add_scale): row_ssq[ssq_parts][num_decoding_seqs] are the per-1024-column sums of squares of the residual
 * rows, `hidden` their length; the slab sums are multiplied by 1/sqrt(sum/hidden + eps) in fp32 before they are rounded,
 * rotated and stored. k_splits in {1, 2, 4}, ssq_parts <= 8. */
extern "C" int swl_paged_attn_decode_qkv_rs(void *o, const float *qkv_slabs, int32_t k_splits, const float *row_ssq,
                                            int32_t ssq_parts, int32_t hidden, float eps, const void *cos_table,
                                            const void *sin_table, const int32_t *pos_idx, void *k_cache,
                                            void *v_cache, const int32_t *block_table, const int32_t *seq_ids,
                                            const int32_t *seq_lens, void *scratch, float softmax_scale,
                                            int32_t num_decoding_seqs, int32_t num_q_heads, int32_t num_kv_heads,
                                            int32_t head_dim, int32_t num_layers, int32_t block_size,
                                            int32_t cur_layer, int32_t max_blocks_per_seq, int32_t seq_block_size,
                                            int32_t num_seq_blocks, int64_t o_tok_stride, int32_t dtype,
                                            swl_stream_t stream) {
    if (num_decoding_seqs == 0 || num_seq_blocks == 0) return num_decoding_seqs < 0 ? SWL_ERR_BAD_ARG : SWL_OK;
    if (!row_ssq || ssq_parts <= 0 || hidden <= 0) return SWL_ERR_BAD_ARG;
    if (ssq_parts > 8 || !(k_splits == 1 || k_splits == 2 || k_splits == 4)) return SWL_ERR_UNSUPPORTED;
    return paged_attn_decode_qkv_impl(o, qkv_slabs, k_splits, cos_table, sin_table, pos_idx, k_cache, v_cache, block_table,
                                      seq_ids, seq_lens, scratch, softmax_scale, num_decoding_seqs, num_q_heads,
                                      num_kv_heads, head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq,
                                      seq_block_size, num_seq_blocks, o_tok_stride, dtype, stream, row_ssq, ssq_parts,
                                      hidden, eps, true);
}

/* swl_paged_attn_decode_qkv_rs stopped after phase 1 when the sequences are split (num_seq_blocks > 1): the partials stay
 * in `scratch` (mid_o fp32 [Bd][H][nsb][D] followed by mid_lse fp32 [Bd][H][nsb], the reference's format,
 * paged_attn.py:106-108) for a consumer that merges them itself (swl_gemm_tiny_partial_from_attn). With one split per
 * sequence it is swl_paged_attn_decode_qkv_rs: the output goes to `o`. */
extern "C" int swl_paged_attn_decode_qkv_rs_partials(void *o, const float *qkv_slabs, int32_t k_splits,
                                                     const float *row_ssq, int32_t ssq_parts, int32_t hidden, float eps,
                                                     const void *cos_table, const void *sin_table,
                                                     const int32_t *pos_idx, void *k_cache, void *v_cache,
                                                     const int32_t *block_table, const int32_t *seq_ids,
                                                     const int32_t *seq_lens, void *scratch, float softmax_scale,
                                                     int32_t num_decoding_seqs, int32_t num_q_heads,
                                                     int32_t num_kv_heads, int32_t head_dim, int32_t num_layers,
                                                     int32_t block_size, int32_t cur_layer, int32_t max_blocks_per_seq,
                                                     int32_t seq_block_size, int32_t num_seq_blocks,
                                                     int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    if (num_decoding_seqs == 0 || num_seq_blocks == 0) return num_decoding_seqs < 0 ? SWL_ERR_BAD_ARG : SWL_OK;
    if (!row_ssq || ssq_parts <= 0 || hidden <= 0) return SWL_ERR_BAD_ARG;
    if (ssq_parts > 8 || !(k_splits == 1 || k_splits == 2 || k_splits == 4)) return SWL_ERR_UNSUPPORTED;
    return paged_attn_decode_qkv_impl(o, qkv_slabs, k_splits, cos_table, sin_table, pos_idx, k_cache, v_cache, block_table,
                                      seq_ids, seq_lens, scratch, softmax_scale, num_decoding_seqs, num_q_heads,
                                      num_kv_heads, head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq,
                                      seq_block_size, num_seq_blocks, o_tok_stride, dtype, stream, row_ssq, ssq_parts,
                                      hidden, eps, false);
}
