// paged_attn_fp8.hip — flash-decoding phase 1 over the FP8 (e4m3fn) KV pool (gfx950). Storage contract: fp8_kv.h.
//
// The kernel of paged_attn.hip (paged_attn_phase1_kernel, matrix-core form) with half the bytes behind it: same grid
// (seq-block, kv-head, sequence), one workgroup serving all G query heads of its kv-head, the same split-K contract, the
// same partial format (mid_o = acc / sum, mid_lse = log2(sum) + max in the scaled base-2 domain), direct output with one
// split — so swl_paged_attn_phase2 and swl_paged_attn_scratch_bytes serve both. Algorithmic bytes per call:
// sum_i len_i * 2 * KVH * D * 1 + q/o + partials.
//   * a 16-token x D tile of one (block, layer, kv-head) is 16 D BYTES, contiguous (2 KiB at D = 128); a lane's 16-byte
//     non-temporal load carries 16 elements: two 1 KiB instructions per tile at D = 128 (the 16-bit kernel: four), one at
//     D = 64, half a wave's worth at D = 32 (lanes 32..63 re-read the tile and do not stage it);
//   * the raw codes wait in the register ring (kPa8Depth blocks per wave, K + V = 16 VGPRs each at D = 128; see
//     SWL_PA8_DEPTH below for the depth); conversion to the activation dtype
//     is exact (v_cvt_scalef32_pk_{f16,bf16}_fp8, scale 1) and sits between the ring and the wave-private LDS stage;
//   * from the stage on it is attend_block_mfma: S = K.Q^T on 16x16x32 MFMA, one (m, l) pair per lane, P as hi + lo
//     16-bit halves, O^T += V^T.P^T through ds_read_b64_tr_b16, mfma_results_ready before VALU reads the scores. ONE path
//     for every G: at G = 1 the columns 1..15 of Q^T are zero;
//   * k_scale[layer, kv-head] is uniform per workgroup: it is folded into c = scale * log2(e) * k_scale, the factor of
//     every exp2 argument (scores stay un-scaled dot products of q with the stored codes' values); v_scale multiplies the
//     normalised output / partial in fp32, before the one rounding;
//   * the masked-garbage rule: 0x7f / 0xff are NaN and a slot past the sequence's length may hold them. A block that
//     crosses the length has the codes of its rows >= len replaced by 0x00 (= +0) in registers before conversion, K and V
//     alike; blocks wholly past it are never loaded. p = 0 then meets v = 0, never NaN.
#include "decode_attn.h"
#include "fp8_kv.h"

// Ring depth (16-token blocks resident per wave, one of them being attended). 2: at D = 128 the 8-wave kernel builds to
// 158 VGPRs (181 with the ring written out in this file, which is the source the deeper rings were tried on); at depth
// 3 / 4 it needed 256 + 320 / 596 spilled registers under the 2-waves-per-SIMD budget
// (hipcc of ROCm 7.2, -Rpass-analysis=kernel-resource-usage), so deeper rings are an experiment build
// (python -m swiftllm_amd.csrc.build --tag d3 -D SWL_PA8_DEPTH=3), not the product.
#ifndef SWL_PA8_DEPTH
#define SWL_PA8_DEPTH 2
#endif

namespace swl {

constexpr int kPa8Depth = SWL_PA8_DEPTH;

struct PagedAttnFp8Params : DecodeAttnParams {
    const float *kv_scales;     // [2][L][KVH]
};

// How a wave's 16-byte lanes cover the 16-token x D-byte tile of one (block, layer, kv-head); the stage's pitches are
// MfmaTile's (attn_mfma.h).
template <int D>
struct Fp8DecodeTile {
    static constexpr int LPT = D / 16;                          // lanes per token row (16 codes each)
    static constexpr int TPI = 64 / LPT < kBlk ? 64 / LPT : kBlk;   // token rows per load instruction
    static constexpr int NI = kBlk / TPI;                       // load instructions per 16-token block
    static constexpr bool ALL = LPT * kBlk >= 64;               // every lane owns a chunk of the tile (D >= 64)
};

// One 16-token block of one wave: codes -> stage -> attend_block_mfma's arithmetic (paged_attn.hip), unchanged. From the
// scores on, the text is that function's on purpose: as a shared __forceinline__ helper it compiled to another register
// allocation in this kernel (one SGPR at D = 128, two VGPRs at D = 32; hipcc of ROCm 7.2) with the fp32 adds commuted,
// and the rings of both kernels are sized against the 256-VGPR budget.
template <typename T, int D>
__device__ __forceinline__ void attend_block_fp8(const vec8_t<T> (&qb)[MfmaTile<T, D>::QS],
                                                 const u32x4_t (&Kraw)[Fp8DecodeTile<D>::NI],
                                                 const u32x4_t (&Vraw)[Fp8DecodeTile<D>::NI], float &m, float &l,
                                                 float4_t (&acc)[MfmaTile<T, D>::OS], T *stage, float c, int tok0,
                                                 int row, int chunk, int lane, int len, bool partial) {
    using Tile = Fp8DecodeTile<D>;
    using MT = MfmaTile<T, D>;
    constexpr int NI = Tile::NI;
    const int q = lane >> 4, i16 = lane & 15;
    u32x4_t Kc[NI], Vc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        Kc[i] = Kraw[i];
        Vc[i] = Vraw[i];
    }
    if (partial) {   // rows at or beyond the length: +0 instead of whatever the slot holds (NaN codes included)
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (tok0 + i * Tile::TPI + row >= len) {
                Kc[i] = u32x4_t{0u, 0u, 0u, 0u};
                Vc[i] = u32x4_t{0u, 0u, 0u, 0u};
            }
    }
    // the codes are converted HERE, one block at a time: tied to this point so that no pass widens a whole ring slot (or
    // several) into 16-bit registers ahead of its turn
#pragma unroll
    for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(Kc[i]));
    const bool stager = Tile::ALL || row < kBlk;
    if (stager) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            vec8_t<T> lo, hi;
            fp8x16_to_t<T>(Kc[i], lo, hi);
            T *dst = stage + (i * Tile::TPI + row) * MT::KRS + chunk * 16;
            *reinterpret_cast<vec8_t<T> *>(dst) = lo;
            *reinterpret_cast<vec8_t<T> *>(dst + 8) = hi;
        }
    }
    float4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < MT::QS; ++j) {
        const vec8_t<T> kf = *reinterpret_cast<const vec8_t<T> *>(stage + i16 * MT::KRS + 32 * j + 8 * q);
        s = mfma16x32(kf, qb[j], s);
    }
    mfma_results_ready<4>(s); // the scores are read by VALU next, behind a branch (swl_common.h)
    // V goes into the same tile once the K fragments are out (same wave: LDS executes in order)
#pragma unroll
    for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(Vc[i]));
    if (stager) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            vec8_t<T> lo, hi;
            fp8x16_to_t<T>(Vc[i], lo, hi);
            T *dst = stage + (i * Tile::TPI + row) * MT::VRS + chunk * 16;
            *reinterpret_cast<vec8_t<T> *>(dst) = lo;
            *reinterpret_cast<vec8_t<T> *>(dst + 8) = hi;
        }
    }
    // s[r] = score of token tok0 + 4q + r for head i16
    if (partial) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (tok0 + 4 * q + r >= len) s[r] = kNegBig;
    }
    float mb = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
    mb = rows_allreduce_max(mb);
    const float m_new = fmaxf(m, mb);
    const float alpha = fast_exp2((m - m_new) * c); // difference first (see attend_block.h)
    const float mc = m_new * c;
    float pf[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pf[r] = fast_exp2(fmaf(s[r], c, -mc));
    if (partial) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (tok0 + 4 * q + r >= len) pf[r] = 0.f;
    }
    l = fmaf(l, alpha, (pf[0] + pf[1]) + (pf[2] + pf[3]));
    m = m_new;
    typename Vec4<T>::type ph, pl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ph[r] = to_t<T>(pf[r]);
        pl[r] = to_t<T>(pf[r] - to_f(ph[r]));
    }
    if (!__all(alpha == 1.0f)) {
#pragma unroll
        for (int mm = 0; mm < MT::OS; ++mm) acc[mm] *= alpha;
    }
#pragma unroll
    for (int mm = 0; mm < MT::OS; ++mm) {
        const short4_t vf = lds_tr_read(stage + (4 * q + (i16 >> 2)) * MT::VRS + 16 * mm + 4 * (i16 & 3));
        acc[mm] = mfma16x16(vf, ph, acc[mm]);
        acc[mm] = mfma16x16(vf, pl, acc[mm]);
    }
}

// NW = waves per workgroup (4 for short sequence blocks, 8 for long ones: dispatch_decode_attn). The block table, the
// lengths and the sequence ids are __restrict__ kernel arguments so their reads stay scalar loads (paged_attn.hip).
template <typename T, int D, int G, int NW>
__global__ __launch_bounds__(NW * 64) void paged_attn_fp8_phase1_kernel(PagedAttnFp8Params p,
                                                                        const int *__restrict__ block_table,
                                                                        const int *__restrict__ seq_lens_r,
                                                                        const int *__restrict__ seq_ids_r) {
    using Tile = Fp8DecodeTile<D>;
    using MT = MfmaTile<T, D>;
    constexpr int NI = Tile::NI;
    constexpr int ND = kPa8Depth;
    __shared__ float sm_ml[NW][G][2];
    __shared__ float sm_acc[NW][G][D];
    __shared__ __attribute__((aligned(16))) T sm_stage[NW][MT::ELEMS];

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
    const int chunk = lane % Tile::LPT;
    const int row = lane / Tile::LPT;
    const float k_scale = p.kv_scales[static_cast<int64_t>(p.layer) * p.KVH + kvh];
    const float v_scale = p.kv_scales[(static_cast<int64_t>(p.L) + p.layer) * p.KVH + kvh];
    const float c = p.scale_log2e * k_scale;

    const uint8_t *kc = static_cast<const uint8_t *>(p.k_cache);
    const uint8_t *vc = static_cast<const uint8_t *>(p.v_cache);
    const int64_t tile_bytes = static_cast<int64_t>(kBlk) * D;
    const int64_t layer_head = static_cast<int64_t>(p.layer) * p.KVH + kvh;
    const int64_t blk_pitch = static_cast<int64_t>(p.L) * p.KVH;
    // D = 32: a tile is 512 bytes, lanes 32..63 read it a second time (in bounds) and never stage it
    const int lane_off = (Tile::ALL ? lane : (lane & 31)) * 16;

    vec8_t<T> qb[MT::QS];               // Q^T B fragments, lane (q, h) -> Q[head h][32 j + 8 q ..], zero for h >= G
    const int mq = lane >> 4, mh = lane & 15;
    {
        const T *qp = static_cast<const T *>(p.q) + seq * p.q_tok_stride +
                      (static_cast<int64_t>(kvh) * G + min(mh, G - 1)) * D + 8 * mq;
#pragma unroll
        for (int j = 0; j < MT::QS; ++j) {
            qb[j] = load8(qp + 32 * j);
            if (mh >= G) qb[j] = vec8_t<T>{};
        }
    }

    float m = kNegBig, l = 0.f;
    float4_t acc4[MT::OS];              // O^T[d = 16 mm + 4 q + r][head h]
#pragma unroll
    for (int mm = 0; mm < MT::OS; ++mm) acc4[mm] = float4_t{0.f, 0.f, 0.f, 0.f};

    u32x4_t Kr[ND][NI], Vr[ND][NI];
    auto load_phys = [&](int64_t phys, u32x4_t(&Kd)[NI], u32x4_t(&Vd)[NI]) {
        const int64_t base = (phys * blk_pitch + layer_head) * tile_bytes + lane_off;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            Kd[i] = load16b_nt(kc + base + i * 1024);
            Vd[i] = load16b_nt(vc + base + i * 1024);
        }
    };
    auto attend = [&](int b, u32x4_t(&Kd)[NI], u32x4_t(&Vd)[NI]) {
        const int tok0 = b * kBlk;
        attend_block_fp8<T, D>(qb, Kd, Vd, m, l, acc4, &sm_stage[wave][0], c, tok0, row, chunk, lane, len,
                               tok0 + kBlk > len);
    };

    const int b = tok_begin / kBlk + wave;
    kv_ring_prefetch<0, ND, NW>(b, blk_end, bt, Kr, Vr, load_phys);
    kv_ring_stream<ND, NW>(b, blk_end, bt, Kr, Vr, load_phys, attend, attend);
    mfma_wave_finish(m, l, acc4, sm_ml, sm_acc, wave, lane);
    __syncthreads();
    merge_waves_write<T, D, G, NW, true>(p, sm_ml, sm_acc, c, v_scale, kvh, seq, split);
}

template <typename T>
static int launch_fp8_phase1(const PagedAttnFp8Params &p, const int *bt, const int *lens, const int *ids, int Bd, int D,
                             hipStream_t stream) {
    return dispatch_decode_attn(D, p.H / p.KVH, p.seq_block_size, [&](auto d, auto g, auto nw) {
        constexpr int NW = decltype(nw)::value;
        hipLaunchKernelGGL((paged_attn_fp8_phase1_kernel<T, decltype(d)::value, decltype(g)::value, NW>),
                           dim3(p.num_seq_blocks, p.KVH, Bd), dim3(NW * 64), 0, stream, p, bt, lens, ids);
        return check_launch();
    });
}

} // namespace swl

extern "C" int swl_paged_attn_phase1_fp8(void *o_direct, const void *q, const void *k_cache, const void *v_cache,
                                         const float *kv_scales, const int32_t *block_table, const int32_t *seq_ids,
                                         const int32_t *seq_lens, float *mid_o, float *mid_lse, float softmax_scale,
                                         int32_t num_decoding_seqs, int32_t num_q_heads, int32_t num_kv_heads,
                                         int32_t head_dim, int32_t num_layers, int32_t block_size, int32_t cur_layer,
                                         int32_t max_blocks_per_seq, int32_t seq_block_size, int32_t num_seq_blocks,
                                         int64_t q_tok_stride, int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    if (num_decoding_seqs < 0) return SWL_ERR_BAD_ARG;
    if (num_decoding_seqs == 0 || num_seq_blocks == 0) return SWL_OK;
    if (!q || !k_cache || !v_cache || !kv_scales || !block_table || !seq_ids || !seq_lens) return SWL_ERR_BAD_ARG;
    const swl::DecodeAttnArgs a{o_direct, q, k_cache, v_cache, q_tok_stride, o_tok_stride, num_q_heads, num_kv_heads,
                                head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq, seq_block_size,
                                num_seq_blocks};
    // this entry refuses a head_dim or dtype it has no kernel for up front, as a bad argument (the 16-bit entries leave
    // them to the launch ladder: SWL_ERR_UNSUPPORTED for the head_dim, after every other check)
    if (!(head_dim == 32 || head_dim == 64 || head_dim == 128) || !(dtype == SWL_F16 || dtype == SWL_BF16))
        return SWL_ERR_BAD_ARG;
    if (const int rc = swl::check_decode_geometry(a)) return rc;
    if (const int rc = swl::check_decode_layout(a)) return rc;
    if (!swl::phase1_outputs_ok(o_direct, mid_o, mid_lse, num_seq_blocks)) return SWL_ERR_BAD_ARG;
    if (!swl::decode_grid_fits(num_decoding_seqs, num_kv_heads)) return SWL_ERR_UNSUPPORTED;
    swl::PagedAttnFp8Params p{};
    swl::fill_decode_params(p, a, mid_o, mid_lse, softmax_scale);
    p.kv_scales = kv_scales;
    SWL_DISPATCH_DTYPE(dtype, T, {
        return swl::launch_fp8_phase1<T>(p, block_table, seq_lens, seq_ids, num_decoding_seqs, head_dim,
                                         static_cast<hipStream_t>(stream));
    });
}

extern "C" int swl_paged_attn_decode_fp8(void *o, const void *q, const void *k_cache, const void *v_cache,
                                         const float *kv_scales, const int32_t *block_table, const int32_t *seq_ids,
                                         const int32_t *seq_lens, void *scratch, float softmax_scale,
                                         int32_t num_decoding_seqs, int32_t num_q_heads, int32_t num_kv_heads,
                                         int32_t head_dim, int32_t num_layers, int32_t block_size, int32_t cur_layer,
                                         int32_t max_blocks_per_seq, int32_t seq_block_size, int32_t num_seq_blocks,
                                         int64_t q_tok_stride, int64_t o_tok_stride, int32_t dtype, swl_stream_t stream) {
    if (num_decoding_seqs < 0) return SWL_ERR_BAD_ARG;
    if (num_decoding_seqs == 0 || num_seq_blocks == 0) return SWL_OK;
    if (!o) return SWL_ERR_BAD_ARG;
    if (num_seq_blocks > 1 && (num_q_heads <= 0 || head_dim <= 0)) return SWL_ERR_BAD_ARG;
    float *mid_o, *mid_lse;
    if (!swl::split_scratch(scratch, num_decoding_seqs, num_q_heads, head_dim, num_seq_blocks, mid_o, mid_lse))
        return SWL_ERR_BAD_ARG;
    const int rc = swl_paged_attn_phase1_fp8(o, q, k_cache, v_cache, kv_scales, block_table, seq_ids, seq_lens, mid_o,
                                             mid_lse, softmax_scale, num_decoding_seqs, num_q_heads, num_kv_heads,
                                             head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq,
                                             seq_block_size, num_seq_blocks, q_tok_stride, o_tok_stride, dtype, stream);
    if (rc != SWL_OK || num_seq_blocks == 1) return rc;
    return swl_paged_attn_phase2(o, mid_o, mid_lse, seq_lens, num_decoding_seqs, num_q_heads, head_dim, seq_block_size,
                                 num_seq_blocks, o_tok_stride, dtype, stream);
}
