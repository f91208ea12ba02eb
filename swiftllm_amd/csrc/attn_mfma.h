// attn_mfma.h — the matrix-core pieces the attention kernels share (gfx950): MFMA wrappers, the LDS transpose read, the
// 16-lane-row reductions, the wave-private tile of decode attention, and the end of decode phase 1, which does not depend
// on how the KV pool is stored (paged_attn.hip: 16-bit pools, paged_attn_fp8.hip: e4m3 pools): the merge of a workgroup's
// waves.
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
// p <= 2^kLazyMax = 16 (see the softmax step of prefill_attn.hip)
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

// ---- decode phase 1, end of the kernel -------------------------------------------------------------------------------
// Merge the NW waves of the workgroup (after the barrier that follows their LDS writes) and write the partial of this
// split — or the final output when there is one split. P = the kernel's parameter struct (o_direct, mid_o, mid_lse, H,
// num_seq_blocks, o_tok_stride). VSCALE: the normalised output is multiplied by v_scale in fp32 before the one rounding
// (FP8 pools); without it the argument is not read and no multiply is emitted.
template <typename T, int D, int G, int NW, bool VSCALE, typename P>
__device__ __forceinline__ void merge_waves_write(const P &p, const float (&sm_ml)[NW][G][2],
                                                  const float (&sm_acc)[NW][G][D], float c, float v_scale, int kvh,
                                                  int seq, int split) {
    const int nsb = p.num_seq_blocks;
    for (int oidx = threadIdx.x; oidx < G * D; oidx += NW * 64) {
        const int g = oidx / D;
        const int d = oidx % D;
        float M = sm_ml[0][g][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) M = fmaxf(M, sm_ml[w][g][0]);
        float Lsum = 0.f, A = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float wgt = fast_exp2((sm_ml[w][g][0] - M) * c);
            Lsum = fmaf(sm_ml[w][g][1], wgt, Lsum);
            A = fmaf(sm_acc[w][g][d], wgt, A);
        }
        float out = A / Lsum;
        if constexpr (VSCALE) out *= v_scale;
        const int head = kvh * G + g;
        if (nsb == 1) {
            static_cast<T *>(p.o_direct)[seq * p.o_tok_stride + static_cast<int64_t>(head) * D + d] = to_t<T>(out);
        } else {
            const int64_t part = (static_cast<int64_t>(seq) * p.H + head) * nsb + split;
            p.mid_o[part * D + d] = out;
            if (d == 0) p.mid_lse[part] = fast_log2(Lsum) + M * c;
        }
    }
}

} // namespace swl
