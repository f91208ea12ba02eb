// attn_mfma.h — the matrix-core pieces the attention kernels share (gfx950): MFMA wrappers, the LDS transpose read, the
// 16-lane-row reductions and the wave-private tile of decode attention with its attend_block (what the decode kernels
// share beyond that: decode_attn.h).
#pragma once

#include "swl_common.h"
#include "attend_block.h"

namespace swl {

typedef short short4_t __attribute__((ext_vector_type(4)));
template <typename T>
struct Vec4 {
    typedef T type __attribute__((ext_vector_type(4)));
};

// Prefill: a row moves its running maximum only when a tile raised it by more than this (base-2 exponent units), so
// p <= 2^kLazyMax = 16 (see the softmax step of prefill_tile.h)
constexpr float kLazyMax = 4.0f;

__device__ __forceinline__ float16_t mfma32(vec8_t<f16> a, vec8_t<f16> b, float16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float16_t mfma32(vec8_t<bf16> a, vec8_t<bf16> b, float16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float4_t mfma16x32(vec8_t<f16> a, vec8_t<f16> b, float4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float4_t mfma16x32(vec8_t<bf16> a, vec8_t<bf16> b, float4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float4_t mfma16x16(short4_t a, typename Vec4<f16>::type b, float4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(typename Vec4<f16>::type, a), b, c, 0, 0, 0);
}
__device__ __forceinline__ float4_t mfma16x16(short4_t a, typename Vec4<bf16>::type b, float4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(short4_t, b), c, 0, 0, 0);
}

// LDS transpose read (gfx950, ds_read_b64_tr_b16): the 16 lanes of a group each give the address of 4 consecutive 16-bit
// elements (lanes 4r..4r+3 = the four quarters of row r); lane i receives column i of that 4 x 16 block:
// {row0[i], row1[i], row2[i], row3[i]}.
template <typename T>
__device__ __forceinline__ short4_t lds_tr_read(const T *p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4_t __attribute__((address_space(3))) *)(p));
}

// All-reduce over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48), VALU only:
// v_permlane16_swap(a, a) -> {rows 0,0,2,2 | rows 1,1,3,3}, v_permlane32_swap(b, b) -> {lo, lo | hi, hi}.
__device__ __forceinline__ float rows_allreduce_max(float v) {
    const auto r1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r1[0]), __uint_as_float(r1[1]));
    const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r2[0]), __uint_as_float(r2[1]));
}
__device__ __forceinline__ float rows_allreduce_sum(float v) {
    const auto r1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r1[0]) + __uint_as_float(r1[1]);
    const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
}

// The wave-private LDS tile of matrix-core decode attention (attend_block_mfma in paged_attn.hip): K rows, then V rows.
template <typename T, int D>
struct MfmaTile {
    static constexpr int KRS = D + 8;    // K row pitch (elements): 16 rows -> 16 distinct 16-byte slots for ds_read_b128
    static constexpr int VRS = D + 16;   // V row pitch: 8 rows x 32 B tile the 64 banks exactly for the b64 transpose read
    static constexpr int ELEMS = 16 * VRS;
    static constexpr int QS = D / 32;    // QK^T MFMAs per block
    static constexpr int OS = D / 16;    // PV MFMA pairs per block
};

// ---- matrix-core variant of attend_block (paged_attn.hip: G >= 2; paged_attn_verify.hip: every G) --------------------------------------------------------------------
// With G query heads per kv head the VALU version (attend_block.h) does G x (dot products + 16-lane reductions + 8-wide FMAs) per
// 16-byte K/V fragment: measured on MI355X the arithmetic costs 22-28 % of the kernel at G = 4 (batch 32 x 1k context:
// 32.0 us, 25.0 us with the arithmetic compiled out; G = 1: 2 % — profiles/r02f_paged_attn_nomath.md). Here the G heads
// become the N dimension of 16 x 16 MFMA tiles (columns >= G are zero padding) and a block's 16 tokens the M / K one:
//   S[token][head]  = K_blk . Q^T   D/32 x v_mfma_f32_16x16x32  (A = K rows from LDS, B = Q^T in registers all kernel long)
//   O^T[d][head]   += V_blk^T . P^T D/16 x v_mfma_f32_16x16x16  (A = V^T via ds_read_b64_tr_b16, B = P^T = the S registers)
// The K/V registers arrive in the coalesced layout of the ring (lane -> token row, 16-byte chunk); one wave-private LDS
// tile turns them into A fragments (in-order LDS pipeline of one wave: no barrier). In the 16 x 16 C layout lane
// (q = l/16, h = l%16) holds tokens 4q..4q+3 of head h: the scores a lane gets from QK^T are exactly the B fragment PV
// needs from it, the online-softmax state is ONE (m, l) pair per lane, and O^T costs D/16 x 4 registers for ANY G
// (the VALU version: 8 G). P is fed as hi + lo 16-bit halves (two MFMAs): the product keeps fp32-level accuracy
// instead of the storage dtype's, so the numerics stay those of the VALU version (and of the reference's fp32 p,
// paged_attn.py:74-79) at 16 more MFMA issues per block.
template <typename T, int D, int G>
__device__ __forceinline__ void attend_block_mfma(const vec8_t<T> (&qb)[MfmaTile<T, D>::QS],
                                                  const vec8_t<T> (&Kv)[DecodeTile<T, D, G>::NI],
                                                  const vec8_t<T> (&Vv)[DecodeTile<T, D, G>::NI], float &m, float &l,
                                                  float4_t (&acc)[MfmaTile<T, D>::OS], T *stage, float c, int tok0,
                                                  int row, int chunk, int lane, int len, bool partial) {
    using Tile = DecodeTile<T, D, G>;
    using MT = MfmaTile<T, D>;
    constexpr int NI = Tile::NI;
    const int q = lane >> 4, i16 = lane & 15;
    // K: ring layout -> row-major tile -> A fragments (row = token i16, k = d)
#pragma unroll
    for (int i = 0; i < NI; ++i)
        *reinterpret_cast<vec8_t<T> *>(stage + (i * Tile::TPI + row) * MT::KRS + chunk * 8) = Kv[i];
    float4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < MT::QS; ++j) {
        const vec8_t<T> kf = *reinterpret_cast<const vec8_t<T> *>(stage + i16 * MT::KRS + 32 * j + 8 * q);
        s = mfma16x32(kf, qb[j], s);
    }
    mfma_results_ready<4>(s); // the scores are read by VALU next, behind a branch (swl_common.h)
    // V goes into the same tile once the K fragments are out (same wave: LDS executes in order)
#pragma unroll
    for (int i = 0; i < NI; ++i)
        *reinterpret_cast<vec8_t<T> *>(stage + (i * Tile::TPI + row) * MT::VRS + chunk * 8) = Vv[i];
    // s[r] = score of token tok0 + 4q + r for head i16
    if (partial) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (tok0 + 4 * q + r >= len) s[r] = kNegBig;
    }
    // block maximum of head i16 over its 16 tokens = over the four lanes q = 0..3: v_permlane16_swap / v_permlane32_swap
    // (VALU only; 1.2x cheaper than two ds_bpermute round trips through the LDS pipe this loop keeps busy)
    float mb = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
    mb = rows_allreduce_max(mb);
    const float m_new = fmaxf(m, mb);
    const float alpha = fast_exp2((m - m_new) * c); // difference first (see attend_block)
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
    // rescale only when some head of this wave raised its maximum (wave-uniform branch; alpha == 1 is the common case
    // after the first blocks of a sequence)
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

} // namespace swl
