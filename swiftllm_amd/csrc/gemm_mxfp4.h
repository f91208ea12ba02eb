// gemm_mxfp4.h — the MXFP4 (OCP Microscaling v1.0: e2m1 elements, one e8m0 scale per 32) contract of the DENSE projections
// of a 16-bit checkpoint quantised at load (q/k/v, o, up/gate, down of a Llama-shaped model served with dense_weight_dtype
// "mxfp4"), the PACKED order of its codes and scales and the host / device arithmetic gemm_mxfp4.hip shares with its
// callers, gfx950, bfloat16. DESIGN.md section 4.24. The work split is gemm_fp8_row.h's.
//
// Numbers. A block is 32 consecutive k of one output row. With amax = max |w| over the block in fp32,
//     e = clamp(floor(log2 amax) - 2, -126, 127)          (the floor is the fp32 exponent field - 127; a zero block: e = 0)
// and the scale BYTE is e + 127, in [1, 254]: 0 and 255 are never written. An element is w * 2^-e (exact in fp32) rounded
// to the e2m1 grid +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}: to nearest, a tie to the code with an even mantissa bit, saturating at
// +-6 (mxfp4_code below: seven comparisons, no table). The weight MEANS e2m1(code) * 2^e, which is exact in bfloat16: the
// GEMMs need no fold, no epilogue multiply and no per-row scale. Two codes share a byte, the lower k in the low nibble —
// the order v_cvt_scalef32_pk_bf16_fp4 reads. float16 is refused: 2^e leaves its range.
//
// Storage. A projection is `codes` (uint8, N K / 2 bytes) and `scales` (uint8); N % 16 == 0, K % 128 == 0, KT = K / 128.
// The codes are PACKED like gemm_fp8_row.h's: the tile of weight rows [16 nt, 16 nt + 16) x k [128 kt, 128 kt + 128) is the
// 1 KiB at byte
//     1024 * (nt * KT + kt)
// and inside it lane (i16 = lane & 15, q = lane >> 4) owns the 16 bytes at 16 * lane: row 16 nt + i16, k 128 kt + 32 q ..
// + 31, in k order — exactly ONE MX block. So the code of (row n, column k) is the low (k even) or high nibble of byte
//     1024 * ((n / 16) * KT + k / 128) + 16 * (16 * ((k % 128) / 32) + n % 16) + (k % 32) / 2.
// The k tiles of a row group follow each other: a wave that walks K reads one contiguous run. The scales are in lane order
// too: with KG = ceil(KT / 4), the 256 bytes at
//     256 * (nt * KG + kt / 4)
// hold the scale bytes of the k tiles 4 (kt / 4) .. + 3, lane's four at 4 * lane, one per k tile: the scale of (row n,
// column k) is byte 256 * ((n / 16) * KG + k / 512) + 4 * (16 * ((k % 128) / 32) + n % 16) + (k / 128) % 4. A lane gets its
// next four scales with one dword load and a wave with one contiguous 256 B. Entries past KT are 127. A fused projection
// is the concatenated rows of its tensors, each quantised into its own slice (16 rows: 8 K bytes of codes, 256 KG of scales).
// mxfp4_unpack_kernel (swl_mxfp4_dequant) is the executable definition of both orders.
//
// The walk (gemm_mxfp4.hip). 4 waves a workgroup, wave w owns row group 4 * blockIdx.x + w over ONE k slice of whole k
// tiles, slice j = tiles [j KT / k_splits, (j + 1) KT / k_splits); split-K slabs are fp32 in the caller's workspace, added
// in slice order by the finishing kernel of gemm_fp8_row.h at scale 1.
//   x       through LDS in chunks of 256 k (two k tiles), one chunk ahead, two buffers, one barrier a chunk.
//   codes   global -> a register ring of EIGHT 1 KiB tiles per row group (1024 k, 8 KiB in flight), a slot asked for again
//           (unconditionally; past the slice: nothing) as soon as its codes are converted.
//   scales  a lane's dword holds the scales of four k tiles. The dword of scale group g + 1 is asked for when the walk
//           ENTERS group g, four tiles before its first use, and is copied to the register in use at the next entry. The
//           memory counter retires loads in issue order, so that copy also waits for the code loads issued before the
//           request — group g + 1's own four tiles, the first of which the walk needs at that moment anyway; the four
//           tiles of group g + 2 stay in flight. A three-register form that asks two groups ahead and never copies a
//           pending register was tried: the compiler merged its two arms into one dynamically indexed copy through
//           scratch, which this kernel may not use.
//   a tile  the scale is uint(byte) << 23 as fp32; dword s of the lane's 16 bytes (k 128 kt + 32 q + 8 s .. + 7) becomes
//           one 8-element bfloat16 fragment with four v_cvt_scalef32_pk_bf16_fp4 (16 a tile) and feeds one
//           v_mfma_f32_16x16x32_bf16 per token tile; the x fragment is read from LDS at the same k. The MFMA sums over k,
//           so the permutation both operands share is free. Every code byte is read once for all ceil(M / 16) token tiles.
//
// The chain of one output element (row m, column n), slice j over tiles [t0_j, t1_j):
//     R_j = 0;  for t = t0_j .. t1_j - 1 (ascending), s = 0 .. 3: R_j = mfma(A_s(t), W_s(t), R_j)
//     sum = (((R_0 + R_1) + R_2) + ...) + R_{k_splits - 1}
// then y = T(sum), or act = fp8_up_gate_act(sum_up, sum_gate, 1, 1) of moe_fp8.h. Padding token rows are zeros and the MFMA
// computes rows independently, so a row's bits depend on that row's activations and the weights only; no atomics: a launch
// of a given (shape, split) is run-to-run deterministic and graph replay writes the bits of eager launches.
#pragma once

#include "gemm_fp8_row.h"

namespace swl {

constexpr int kMxKStep = 128;                               // k per tile: 32 codes (16 bytes, one MX block) a lane
constexpr int kMxBlock = 32;
constexpr int kMxMaxM = 64;                                 // four token tiles of 16
constexpr int kMxWaves = 4;                                 // = row groups of a workgroup
constexpr int kMxChunk = 256;                               // k of x one LDS buffer holds: 2 k tiles
constexpr int kMxRing = 8;                                  // k tiles of codes a wave keeps in flight per row group
constexpr int kMxMaxSplits = 8;
constexpr int kMxTileBytes = 1024;
constexpr int kMxScaleGroup = 4;                            // k tiles whose scales share a lane's dword

inline bool mxfp4_geometry_ok(int n, int k) { return n > 0 && k > 0 && n % 16 == 0 && k % kMxKStep == 0; }

inline bool mxfp4_splits_ok(int ks, int k) {
    return ks >= 1 && ks <= kMxMaxSplits && !(ks & (ks - 1)) && ks <= k / kMxKStep;
}

__host__ __device__ inline int mxfp4_scale_groups(int KT) { return (KT + kMxScaleGroup - 1) / kMxScaleGroup; }

// byte of the 16 code bytes lane `lane` owns in tile (nt, kt) of a projection with KT k tiles
__host__ __device__ inline int64_t mxfp4_tile_byte(int nt, int kt, int KT, int lane) {
    return (static_cast<int64_t>(nt) * KT + kt) * kMxTileBytes + 16 * lane;
}

// byte of the scale dword lane `lane` owns in scale group kg (k tiles 4 kg .. + 3) of row group nt
__host__ __device__ inline int64_t mxfp4_scale_byte(int nt, int kg, int KG, int lane) {
    return (static_cast<int64_t>(nt) * KG + kg) * 256 + 4 * lane;
}

// e of a block from its fp32 amax (>= 0): the exponent field - 127 - 2, clamped; a zero block: 0
__host__ __device__ inline int mxfp4_block_exponent(unsigned amax_bits) {
    if (amax_bits == 0u) return 0;
    const int e = static_cast<int>((amax_bits >> 23) & 0xffu) - 129;
    return e < -126 ? -126 : e > 127 ? 127 : e;
}

// the e2m1 code of v = w * 2^-e: the grid's midpoints, a tie to the even mantissa bit, +-6 beyond; a NaN: 0
__host__ __device__ inline unsigned mxfp4_code(float v) {
    const float a = v < 0.f ? -v : v;
    const unsigned mag = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
    return mag | (v < 0.f ? 8u : 0u);
}

} // namespace swl
