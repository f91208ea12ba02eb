// moe_fp8_block.h — the BLOCK-SCALED FP8 (OCP e4m3fn) expert-weight contract, as the published fine-grained FP8 checkpoints
// store it (quantization_config: quant_method fp8, fmt e4m3, weight_block_size [128, 128]), and the device pieces the two
// translation units that serve it share (moe_fp8_block.hip: 16-row form; moe_fp8_block_wide.hip: row-tile form), gfx950.
// DESIGN.md section 4.21. The load shape, the A/B fragment permutation and the exact dequantisation are moe_fp8.h's.
//
// Storage. expert_up_gate is codes [E, 2 I, H] ([up ; gate] per expert), expert_down codes [E, H, I]: one e4m3fn byte per
// element, ONE copy — the checkpoint's own bytes, never re-quantised. With RB_x = KB_x = ceil(x / 128):
//   expert_up_gate_bscale  fp32 [E, 2 RB_I, KB_H]: the up projection's RB_I row blocks first, then gate's. Gate's row block r
//                          is at RB_I + r (NOT at (I + 128 r) / 128: the two differ when I % 128 != 0).
//   expert_down_bscale     fp32 [E, RB_H, KB_I].
// The weight MEANS fp(code) * bscale[row / 128][k / 128] (rows counted inside the projection). H % 64 == 0 and I % 64 == 0
// (swl_moe_fp8_supported); a last row block or k block may be partial, which indexing by row / 128 and k / 128 covers. A
// 16-column tile (and the 32- and 64-column tiles of the row-tile form, which start at multiples of their width) lies
// inside one row block. NaN codes (0x7f, 0xff) dequantise to NaN and propagate: no special case.
//
// The chain of one output element (row m of the step, column n; s[j] = bscale[n / 128][j], the same for a workgroup's whole
// column tile). A k step is 64 wide; step t covers k [64 t, 64 t + 64) and lies inside k block t / 2. Wave w of 8:
//     R_w = 0
//     for t = w, w + 8, w + 16, ... (ascending, while 64 t < K):
//         P = 0; P = mfma(A_lo(t), W_lo(t), P); P = mfma(A_hi(t), W_hi(t), P)      (low half of the lanes' 16 k, then high)
//         R_w = fmaf(P, s[t / 2], R_w)                                              (the FOLD: one rounding, every step)
//     sum = ((((((R_0 + R_1) + R_2) + R_3) + R_4) + R_5) + R_6) + R_7                (through LDS, wave order)
// then the epilogue: up, gate = T(sum); act = up *_T T(silu(gate)) — or y = sum itself, unrounded. An element is folded
// ceil(K / 64) times in all. Steps keep the wave assignment of moe_fp8.h (every step folded) and not "one wave per
// 128-k block": with I = 768 the latter leaves two of eight waves without work. Both forms — and any number of tiles or
// column blocks under one wave — keep exactly this chain, so they write the same bits.
//
// Scales are read as wave-uniform values through the scalar data path (a pointer into the constant address space at a
// uniform index: one scalar load per weight row block and step, issued with that step's vector loads), never per lane.
#pragma once

#include "moe_fp8.h"

namespace swl {

constexpr int kFp8BlockSide = 128;                          // rows and k of one scale

__host__ __device__ inline int moe_fp8_blocks(int x) { return (x + kFp8BlockSide - 1) / kFp8BlockSide; }

typedef const float __attribute__((address_space(4))) *fp8_bscale_ptr;

// a scale row as the scalar unit reads it (uniform pointer, uniform index)
__device__ __forceinline__ fp8_bscale_ptr fp8_bscale_row(const float *p) { return (fp8_bscale_ptr)p; }

// the wave's index as a scalar: what makes k, and with it the scale index, uniform for the compiler
__device__ __forceinline__ int fp8_block_wave() { return __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)); }

// P = A[16 k] . dequantised(codes)[16 k] from a zero accumulator: low half, then high half
template <typename T>
__device__ __forceinline__ float4_t fp8_block_partial(const Fp8AFrag<T> &a, const u32x4_t &codes) {
    vec8_t<T> wlo, whi;
    fp8x16_to_t<T>(codes, wlo, whi);
    float4_t p = {0.f, 0.f, 0.f, 0.f};
    p = mfma16x32(a.lo, wlo, p);
    return mfma16x32(a.hi, whi, p);
}

// The fold: run = fmaf(P, scale, run), ONE rounding per element. P is read by VALU here: the callers build all partials
// of a pass, mfma_results_tie() each and mfma_results_ready() the last one before the first fold (swl_common.h: the
// matrix pipe's wait states are not padded on the taken side of a branch, and the walks' loops put branches here).
__device__ __forceinline__ float4_t fp8_block_fold(const float4_t &p, float scale, float4_t run) {
#pragma unroll
    for (int r = 0; r < 4; ++r) run[r] = __fmaf_rn(p[r], scale, run[r]);
    return run;
}

// act = T(up) *_T T(silu(T(gate))) from the two finished fp32 sums: moe_up_gate_silu_kernel's epilogue
template <typename T>
__device__ __forceinline__ T fp8_block_up_gate_act(float su, float sg) {
    const T up = to_t<T>(su);
    const float g = to_f(to_t<T>(sg));
    const T silu = to_t<T>(g / (1.0f + expf(-g)));
    return mul_t<T>(up, silu);
}

} // namespace swl
