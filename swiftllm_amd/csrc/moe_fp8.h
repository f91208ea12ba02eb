// moe_fp8.h — the FP8 (OCP e4m3fn) expert-weight storage contract and the device pieces the two FP8 expert-GEMM translation
// units share (moe_fp8.hip: quantiser + 16-row form; moe_fp8_wide.hip: row-tile form), gfx950. DESIGN.md section 4.20.
//
// Storage. expert_up_gate is codes [E, 2 I, H], expert_down codes [E, H, I]: one e4m3fn byte per element in the row-major
// order of the 16-bit stacks, ONE copy. One fp32 scale per OUTPUT ROW: up_gate_scale [E, 2 I], down_scale [E, H]. The
// weight MEANS fp(code) * scale[row].
//   quantise    per row of the 16-bit checkpoint tensor, at load: amax = max |w_row|, scale = fp32(amax / 448) (a zero row:
//               1), inv = fp32(1 / scale), both computed by the host side with torch; code = RNE_e4m3(clamp(fp32(w) * inv,
//               -448, +448)) — quantise16 of fp8_kv.h, the KV store's arithmetic. Bit-exact twin on the host:
//               w.float().mul(inv[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
//   dequantise  code -> T (float16 / bfloat16) is EXACT (fp8x2_to_t of fp8_kv.h). The GEMMs multiply the 16-bit activations
//               with the dequantised codes in v_mfma_f32_16x16x32, accumulate in fp32 and multiply the finished fp32 sum ONCE
//               by scale[row]: before the rounding to T for up and gate, as the last fp32 operation for y.
//   NaN codes   the quantiser clamps, so a stack built by it holds no 0x7f / 0xff unless the checkpoint held a NaN.
//
// The walk. A k step is 64 wide. Lane (i16 = lane & 15, q = lane >> 4) owns the 16 consecutive k [k0 + 16 q, k0 + 16 q + 16)
// of weight row i16: ONE 16-byte load per lane, and a wave asks for 16 rows x 64 contiguous bytes = 1 KiB per row group and
// instruction — the request shape of the 16-bit kernels (16 bytes a lane, 64 contiguous bytes a row). The 16 codes feed two
// MFMAs: the first takes k 16 q .. 16 q + 7, the second 16 q + 8 .. 16 q + 15, and the A fragments (two 16-byte loads of
// the lane's x row at the same 16 k) are permuted the same way; which k a lane group multiplies inside one MFMA is free as
// long as A and B agree. Wave w of 8 takes the steps w, w + 8, ... in ascending order, low half before high half; the eight
// partials are added in wave order 0..7. Both forms keep exactly this chain per output element, so they write the same bits.
#pragma once

#include "attn_mfma.h"
#include "fp8_kv.h"
#include "moe_common.h"

namespace swl {

constexpr int kFp8KStep = 64;                               // k per wave and step: 16 codes a lane
constexpr int kFp8Round = kFp8KStep * kMoeWaves;            // k one round of all waves covers

inline bool moe_fp8_geometry_ok(int hidden, int inter) {
    return hidden > 0 && inter > 0 && hidden % kFp8KStep == 0 && inter % kFp8KStep == 0 && hidden / 16 <= 65535 &&
           inter / 16 <= 65535;
}

// the A side of one step: this lane's 16 k of its x / act row (zeros for a padding row)
template <typename T>
struct Fp8AFrag {
    vec8_t<T> lo, hi;
};

template <typename T>
__device__ __forceinline__ Fp8AFrag<T> fp8_load_a(const T *p, bool on) {
    Fp8AFrag<T> f;
    if (on) {
        f.lo = load8(p);
        f.hi = load8(p + 8);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f.lo[j] = to_t<T>(0.f), f.hi[j] = to_t<T>(0.f);
    }
    return f;
}

// acc += A[16 k] . dequantised(codes)[16 k]: low half, then high half
template <typename T>
__device__ __forceinline__ float4_t fp8_step_mfma(const Fp8AFrag<T> &a, const u32x4_t &codes, float4_t acc) {
    vec8_t<T> wlo, whi;
    fp8x16_to_t<T>(codes, wlo, whi);
    acc = mfma16x32(a.lo, wlo, acc);
    return mfma16x32(a.hi, whi, acc);
}

// blk[0] + blk[1] + ... + blk[7] of one element, in wave order
__device__ __forceinline__ float fp8_wave_sum(const float (*blk)[16][16], int rr, int cc) {
    float s = blk[0][rr][cc];
#pragma unroll
    for (int wv = 1; wv < kMoeWaves; ++wv) s += blk[wv][rr][cc];
    return s;
}

// act = T(up) *_T T(silu(T(gate))) from the two finished fp32 sums and their rows' scales: moe_up_gate_silu_kernel's
// epilogue behind one fp32 multiply each
template <typename T>
__device__ __forceinline__ T fp8_up_gate_act(float su, float sg, float scale_up, float scale_gate) {
    const T up = to_t<T>(__fmul_rn(su, scale_up));
    const float g = to_f(to_t<T>(__fmul_rn(sg, scale_gate)));
    const T silu = to_t<T>(g / (1.0f + expf(-g)));
    return mul_t<T>(up, silu);
}

} // namespace swl
