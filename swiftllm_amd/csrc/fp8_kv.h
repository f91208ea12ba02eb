// fp8_kv.h — the FP8 (OCP e4m3fn) KV-cache storage contract, device side (gfx950). DESIGN.md section 3.
//
// Pool layout: [num_blocks, L, KVH, 16, D] bytes, one e4m3fn code per element (a (block, layer, kv-head) tile is 2 KiB at
// D = 128). Scales: fp32 [2, L, KVH] (k_scale rows first, then v_scale), and next to them inv = fp32(1 / scale), computed
// on the host, same shape.
//   quantise    stored = RNE_e4m3(clamp(fp32(x) * inv, -448, +448))   — the clamp is explicit: nothing relies on what
//               v_cvt_pk_fp8_f32 does beyond the largest finite code. Bit-exact twin on the host:
//               x.float().mul(inv).clamp(-448, 448).to(torch.float8_e4m3fn)
//   dequantise  e4m3 -> the 16-bit activation dtype is EXACT (4 significant bits, exponents -9..8: every finite code is a
//               float16 and a bfloat16 value), so a kernel reading the pool computes on the stored values; k_scale goes
//               into the exp2 factor, v_scale into the final normalisation (one rounding at the output, as before).
//   NaN codes   0x7f / 0xff decode to NaN and an unowned slot may hold them: readers zero every key at or beyond the
//               sequence length before it can reach a product (the masked-garbage rule of prefill_attn_paged.hip).
#pragma once

#include "swl_common.h"

namespace swl {

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

constexpr float kFp8Max = 448.0f;

__device__ __forceinline__ u32x4_t load16b_nt(const uint8_t *p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(p));
}

// two e4m3 codes (the low or the high half of a dword) -> two T, exact: v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1
template <typename T, bool HI>
__device__ __forceinline__ vec2_t<T> fp8x2_to_t(unsigned w);
template <>
__device__ __forceinline__ vec2_t<f16> fp8x2_to_t<f16, false>(unsigned w) {
    return __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false);
}
template <>
__device__ __forceinline__ vec2_t<f16> fp8x2_to_t<f16, true>(unsigned w) {
    return __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true);
}
template <>
__device__ __forceinline__ vec2_t<bf16> fp8x2_to_t<bf16, false>(unsigned w) {
    return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
}
template <>
__device__ __forceinline__ vec2_t<bf16> fp8x2_to_t<bf16, true>(unsigned w) {
    return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true);
}

// 16 consecutive codes (one 16-byte load) -> elements 0..7 and 8..15 in memory order
template <typename T>
__device__ __forceinline__ void fp8x16_to_t(const u32x4_t &raw, vec8_t<T> &lo, vec8_t<T> &hi) {
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const vec2_t<T> a = fp8x2_to_t<T, false>(raw[w]), b = fp8x2_to_t<T, true>(raw[w]);
        const vec2_t<T> c = fp8x2_to_t<T, false>(raw[2 + w]), d = fp8x2_to_t<T, true>(raw[2 + w]);
        lo[4 * w] = a[0], lo[4 * w + 1] = a[1], lo[4 * w + 2] = b[0], lo[4 * w + 3] = b[1];
        hi[4 * w] = c[0], hi[4 * w + 1] = c[1], hi[4 * w + 2] = d[0], hi[4 * w + 3] = d[1];
    }
}

// the value handed to the conversion: fp32 product (one rounding), clamped; a NaN stays a NaN as torch.clamp keeps it
__device__ __forceinline__ float fp8_prescale(float x, float inv) {
    const float y = __fmul_rn(x, inv);
    return y != y ? y : fminf(fmaxf(y, -kFp8Max), kFp8Max);
}

// 16 elements of T -> 16 codes (v_cvt_pk_fp8_f32: round to nearest even, e4m3 subnormals included)
template <typename T>
__device__ __forceinline__ u32x4_t quantise16(const vec8_t<T> &x0, const vec8_t<T> &x1, float inv) {
    u32x4_t r;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        int a = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(to_f(x0[4 * w]), inv), fp8_prescale(to_f(x0[4 * w + 1]), inv),
                                                0, false);
        a = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(to_f(x0[4 * w + 2]), inv), fp8_prescale(to_f(x0[4 * w + 3]), inv), a,
                                            true);
        int b = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(to_f(x1[4 * w]), inv), fp8_prescale(to_f(x1[4 * w + 1]), inv),
                                                0, false);
        b = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(to_f(x1[4 * w + 2]), inv), fp8_prescale(to_f(x1[4 * w + 3]), inv), b,
                                            true);
        r[w] = static_cast<unsigned>(a);
        r[2 + w] = static_cast<unsigned>(b);
    }
    return r;
}

} // namespace swl
