// decode_attn.h — what the decode-stage paged-attention kernels share (gfx950): paged_attn.hip (16-bit pools, plain q and
// fused-QKV prologue), paged_attn_fp8.hip (e4m3 pools) and paged_attn_verify.hip (speculative-decoding verify).
// Device side: the parameter base, the K/V register ring, the matrix-core wave epilogue and the merge of a workgroup's
// waves. Host side: the argument checks, the scratch split and the launch ladder of their entry points.
#pragma once

#include "attn_mfma.h"

namespace swl {

// What every decode attention kernel is told; a variant derives from it and adds only what it alone reads.
struct DecodeAttnParams {
    void *o;                        // written directly when num_seq_blocks == 1
    const void *q;
    const void *k_cache;
    const void *v_cache;
    float *mid_o;
    float *mid_lse;
    float scale_log2e;
    int H, KVH, L, layer, max_blocks_per_seq, seq_block_size, num_seq_blocks;
    int64_t q_tok_stride, o_tok_stride;
};

// ---- the K/V register ring -------------------------------------------------------------------------------------------
// A wave strides over the 16-token blocks b, b + NW, ... < blk_end of its sequence block and keeps ND of them resident
// in registers (Kr[d], Vr[d]: NI 16-byte loads each for K and for V) — the one it attends plus ND-1 in flight.
// load_phys(phys, Kd, Vd) requests physical block `phys` into a slot; attend(b, Kd, Vd) consumes one.

// The first requests of the ring: blocks b0 + d*NW into slots d = LO..HI-1. It is the kernels that call this (the QKV
// prologue interleaves it with its slab loads); bt[b] is a scalar load, b being wave-uniform.
template <int LO, int HI, int NW, int ND, int NI, typename Slot, typename LoadPhys>
__device__ __forceinline__ void kv_ring_prefetch(int b0, int blk_end, const int *__restrict__ bt, Slot (&Kr)[ND][NI],
                                                 Slot (&Vr)[ND][NI], LoadPhys load_phys) {
#pragma unroll
    for (int d = LO; d < HI; ++d)
        if (b0 + d * NW < blk_end) load_phys(bt[b0 + d * NW], Kr[d], Vr[d]);
}

// Steady state and drain, behind kv_ring_prefetch<0, ND>. attend_tail is what the drain calls instead of attend (a
// wave's last block is always attended there): the QKV variant patches the token being decoded into its block there.
template <int ND, int NW, int NI, typename Slot, typename LoadPhys, typename Attend, typename AttendTail>
__device__ __forceinline__ void kv_ring_stream(int b, int blk_end, const int *__restrict__ bt, Slot (&Kr)[ND][NI],
                                               Slot (&Vr)[ND][NI], LoadPhys load_phys, Attend attend,
                                               AttendTail attend_tail) {
    // steady state: every refill is unconditional, so the waits between slots are exact counted vmcnt waits (a
    // conditional load in the body makes the compiler wait for one slot more than needed); slot d attends block
    // b + d*NW and is refilled with block b + (d+ND)*NW
    if (b + (2 * ND - 1) * NW < blk_end) {
        // The first ND requests are conditional (short sequence blocks), so on entry the compiler cannot know how
        // many loads are outstanding and would size EVERY wait of the loop for the fewest — i.e. wait for the newest
        // slot before touching the oldest (seen in the ISA of the r01 kernel as well: its prefetch never overlapped
        // its own compute). One full wait here — all ND slots were requested long ago, this is the pipeline fill —
        // hands the loop an exact state; from then on every wait in it is a counted vmcnt.
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0), expcnt/lgkmcnt untouched
        do {
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                // scheduling fences: left alone, the compiler computes all ND blocks back to back behind ONE vmcnt(0)
                // and sinks every refill to the end of the iteration — nothing in flight while it computes (seen in
                // the ISA: 34 us instead of 27 at batch 32 x 1k). Pinned, the wait before slot d+1 is a counted one.
                // (the block-table entry of the refill is requested BEFORE the block is attended: behind the fence its
                // scalar-load round trip would sit between every attend and the refill it feeds)
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
    // drain: at most 2*ND-1 blocks left, the first ND of them already in their slots
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        if (b + d * NW < blk_end) {
            attend_tail(b + d * NW, Kr[d], Vr[d]);
            __builtin_amdgcn_sched_barrier(0);
            if (b + (d + ND) * NW < blk_end) load_phys(bt[b + (d + ND) * NW], Kr[d], Vr[d]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int d = 0; d < ND - 1; ++d)
        if (b + (d + ND) * NW < blk_end) {
            attend_tail(b + (d + ND) * NW, Kr[d], Vr[d]);
            __builtin_amdgcn_sched_barrier(0); // one block's fragments live at a time (FP8: the converted codes)
        }
}

// ---- end of a matrix-core wave ---------------------------------------------------------------------------------------
// Hands the wave's state to the merge: lane (mq = lane / 16, mh = lane % 16) holds O^T[d = 16 mm + 4 mq + r][column mh],
// the four lanes of a column share m and each hold the row sum of their own tokens. C = columns the kernel merges: the
// G heads in decode (columns >= G are padding and are not written), all 16 in verify. The caller's barrier follows.
template <int NW, int C, int D>
__device__ __forceinline__ void mfma_wave_finish(float m, float l, float4_t (&acc4)[D / 16], float (&sm_ml)[NW][C][2],
                                                 float (&sm_acc)[NW][C][D], int wave, int lane) {
    const int mq = lane >> 4, mh = lane & 15;
    // O^T of the last block is stored by DS instructions below (swl_common.h)
#pragma unroll
    for (int mm = 0; mm < D / 16; ++mm) mfma_results_tie(acc4[mm]);
    mfma_results_ready<4>(acc4[D / 16 - 1]);
    const float lt = rows_allreduce_sum(l);
    if (mh < C) {
        if (mq == 0) {
            sm_ml[wave][mh][0] = m;
            sm_ml[wave][mh][1] = lt;
        }
#pragma unroll
        for (int mm = 0; mm < D / 16; ++mm)
#pragma unroll
            for (int r = 0; r < 4; ++r) sm_acc[wave][mh][16 * mm + 4 * mq + r] = acc4[mm][r];
    }
}

// ---- merge of the workgroup's waves (after the barrier that follows their LDS writes) ---------------------------------
// Element d of column `col`: LSE-weighted sum over the NW waves, written as the partial of this split — or as the final
// output when there is one split. Partials use the reference's format: mid_o = acc / sum, mid_lse = log2(sum) + max in
// the scaled base-2 domain. VSCALE: the normalised output is multiplied by v_scale in fp32 before the one rounding (FP8
// pools); without it the argument is not read and no multiply is emitted.
template <typename T, int D, int NW, int C, bool VSCALE>
__device__ __forceinline__ void merge_waves_elem(const DecodeAttnParams &p, const float (&sm_ml)[NW][C][2],
                                                 const float (&sm_acc)[NW][C][D], float c, float v_scale, int col, int d,
                                                 int64_t orow, int head, int split) {
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
    float out = A / Lsum;
    if constexpr (VSCALE) out *= v_scale;
    const int nsb = p.num_seq_blocks;
    if (nsb == 1) {
        static_cast<T *>(p.o)[orow * p.o_tok_stride + static_cast<int64_t>(head) * D + d] = to_t<T>(out);
    } else {
        const int64_t part = (orow * p.H + head) * nsb + split;
        p.mid_o[part * D + d] = out;
        if (d == 0) p.mid_lse[part] = fast_log2(Lsum) + M * c;
    }
}

// Decode: column g = q-head kvh * G + g of sequence `seq`, every column is real.
template <typename T, int D, int G, int NW, bool VSCALE>
__device__ __forceinline__ void merge_waves_write(const DecodeAttnParams &p, const float (&sm_ml)[NW][G][2],
                                                  const float (&sm_acc)[NW][G][D], float c, float v_scale, int kvh,
                                                  int seq, int split) {
    for (int oidx = threadIdx.x; oidx < G * D; oidx += NW * 64)
        merge_waves_elem<T, D, NW, G, VSCALE>(p, sm_ml, sm_acc, c, v_scale, oidx / D, oidx % D, seq, kvh * G + oidx / D,
                                              split);
}

// ---- host side: what the entry points of the three files do alike -----------------------------------------------------
// Their refusals differ in places (an unsupported head_dim is SWL_ERR_UNSUPPORTED from the launch ladder in one entry
// and SWL_ERR_BAD_ARG up front in another) and callers are promised every one of them, so the shared checks are two
// steps, each returning one code, and an entry point puts the checks of its own before, between or after them.
struct DecodeAttnArgs {
    const void *o, *q, *k_cache, *v_cache; // q: the query rows, or the qkv slabs they are still in
    int64_t q_tok_stride, o_tok_stride;
    int num_q_heads, num_kv_heads, head_dim, num_layers, block_size, cur_layer, max_blocks_per_seq, seq_block_size,
        num_seq_blocks;
};

// Heads, layers and the block table: SWL_ERR_BAD_ARG; then the pool's block size: SWL_ERR_UNSUPPORTED.
inline int check_decode_geometry(const DecodeAttnArgs &a) {
    if (a.num_seq_blocks < 0 || a.num_q_heads <= 0 || a.num_kv_heads <= 0 || a.num_q_heads % a.num_kv_heads != 0 ||
        a.num_layers <= 0 || a.cur_layer < 0 || a.cur_layer >= a.num_layers || a.max_blocks_per_seq <= 0)
        return SWL_ERR_BAD_ARG;
    return a.block_size == kBlk ? SWL_OK : SWL_ERR_UNSUPPORTED;
}

// The sequence block and the 16-byte accesses of the kernels: SWL_ERR_BAD_ARG. o is only looked at when it is given (it
// may be NULL when the sequences are split and the caller merges the partials itself); q_rows = false: q is the slabs,
// which have no token stride to check.
inline int check_decode_layout(const DecodeAttnArgs &a, bool q_rows = true) {
    if (a.seq_block_size <= 0 || a.seq_block_size % a.block_size != 0) return SWL_ERR_BAD_ARG;
    const int64_t hd = static_cast<int64_t>(a.num_q_heads) * a.head_dim;
    if (!aligned16(a.q) || !aligned16(a.k_cache) || !aligned16(a.v_cache) ||
        (q_rows && ((a.q_tok_stride & 7) || a.q_tok_stride < hd)))
        return SWL_ERR_BAD_ARG;
    if (a.o && (!aligned16(a.o) || (a.o_tok_stride & 7) || a.o_tok_stride < hd)) return SWL_ERR_BAD_ARG;
    return SWL_OK;
}

// The phase-1 entries are handed o, mid_o and mid_lse one by one: the destination that the split count calls for is there,
// the partials fp32-aligned.
inline bool phase1_outputs_ok(const void *o, const float *mid_o, const float *mid_lse, int num_seq_blocks) {
    if (num_seq_blocks == 1) return o != nullptr;
    return mid_o && mid_lse && !((reinterpret_cast<uintptr_t>(mid_o) | reinterpret_cast<uintptr_t>(mid_lse)) & 3u);
}

// The grid is (split, kv-head, sequence): y and z hold 65535.
inline bool decode_grid_fits(int num_seqs, int num_kv_heads) { return num_seqs <= 65535 && num_kv_heads <= 65535; }

// scratch -> mid_o fp32 [rows][H][nsb][D], mid_lse fp32 [rows][H][nsb] (swl_paged_attn_scratch_bytes); both NULL with
// one split, when nothing is staged. false: the scratch is needed and missing or misaligned.
inline bool split_scratch(void *scratch, int rows, int num_q_heads, int head_dim, int num_seq_blocks, float *&mid_o,
                          float *&mid_lse) {
    mid_o = mid_lse = nullptr;
    if (num_seq_blocks <= 1) return true;
    if (!scratch || !aligned16(scratch)) return false;
    mid_o = static_cast<float *>(scratch);
    mid_lse = mid_o + static_cast<size_t>(rows) * num_q_heads * num_seq_blocks * head_dim;
    return true;
}

inline void fill_decode_params(DecodeAttnParams &p, const DecodeAttnArgs &a, float *mid_o, float *mid_lse,
                               float softmax_scale) {
    p.o = const_cast<void *>(a.o);
    p.q = a.q;
    p.k_cache = a.k_cache;
    p.v_cache = a.v_cache;
    p.mid_o = mid_o;
    p.mid_lse = mid_lse;
    p.scale_log2e = softmax_scale * 1.44269504088896340736f;
    p.H = a.num_q_heads;
    p.KVH = a.num_kv_heads;
    p.L = a.num_layers;
    p.layer = a.cur_layer;
    p.max_blocks_per_seq = a.max_blocks_per_seq;
    p.seq_block_size = a.seq_block_size;
    p.num_seq_blocks = a.num_seq_blocks;
    p.q_tok_stride = a.q_tok_stride;
    p.o_tok_stride = a.o_tok_stride;
}

// The launch ladder: launch(IntTag<D>, IntTag<G>, IntTag<NW>) for head_dim D in {32, 64, 128}, G = H / KVH in {1, 2, 4,
// 8} and NW waves per workgroup — 8 from 32 KV blocks per sequence block on (>= 4 blocks per wave), else 4. (A VALU
// kernel of G = 8 would need > 256 registers per lane; the matrix-core ones do not.)
template <typename Launch>
inline int dispatch_decode_attn(int D, int G, int seq_block_size, Launch launch) {
    auto on_g = [&](auto d, auto g) {
        return seq_block_size >= 32 * kBlk ? launch(d, g, IntTag<8>{}) : launch(d, g, IntTag<4>{});
    };
    auto on_d = [&](auto d) {
        switch (G) {
        case 1: return on_g(d, IntTag<1>{});
        case 2: return on_g(d, IntTag<2>{});
        case 4: return on_g(d, IntTag<4>{});
        case 8: return on_g(d, IntTag<8>{});
        default: return SWL_ERR_UNSUPPORTED;
        }
    };
    switch (D) {
    case 32: return on_d(IntTag<32>{});
    case 64: return on_d(IntTag<64>{});
    case 128: return on_d(IntTag<128>{});
    default: return SWL_ERR_UNSUPPORTED;
    }
}

} // namespace swl
