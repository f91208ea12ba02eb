// gemm_fp8_row.h — the PER-ROW FP8 (OCP e4m3fn) contract of the DENSE projections of a 16-bit checkpoint quantised at load
// (q/k/v, o, up/gate, down of a Llama-shaped model served with dense_weight_dtype "fp8_e4m3"), the PACKED order of its
// codes and the host / device arithmetic gemm_fp8_row.hip shares with its callers, gfx950. DESIGN.md section 4.23. The
// numeric contract, the A/B fragment permutation and the exact dequantisation are moe_fp8.h's.
//
// Numbers. Per OUTPUT ROW of the 16-bit tensor: scale = fp32(max |w_row| / 448) (a zero row: 1), inv = fp32(1 / scale), both
// computed by the caller with torch (kernels/moe.py: row_scales, the expert stacks' own); code = RNE_e4m3(clamp(fp32(w) * inv, -448, +448)) (quantise16 of
// fp8_kv.h). The weight MEANS fp32(code) * scale[row]. A fused projection (qkv_proj = [q ; k ; v], up_gate_proj =
// [up ; gate]) is the concatenated rows of its tensors: per-row scales need no segment table.
//
// Storage. A projection is `codes`, N x K bytes, and `scale`, fp32 [N]; N % 16 == 0, K % 64 == 0. The codes are PACKED: with
// KT = K / 64, the tile of weight rows [16 nt, 16 nt + 16) x k [64 kt, 64 kt + 64) is the 1 KiB at byte
//     1024 * (nt * KT + kt)
// and inside it lane (i16 = lane & 15, q = lane >> 4) finds its 16 codes — row 16 nt + i16, k 64 kt + 16 q .. + 15, in k
// order — at byte 16 * lane. So the code of (row n, column k) is byte
//     1024 * ((n / 16) * KT + k / 64) + 16 * (16 * ((k % 64) / 16) + n % 16) + k % 16.
// The k tiles of one row group follow each other: a wave that walks a row group's K reads ONE contiguous run of 16 K bytes,
// 1 KiB per wave-wide 16-byte-per-lane load (row-major codes: 16 rows x 64 bytes per load). fp8_row_unpack_kernel
// (swl_fp8_row_dequant) is the executable definition of this order.
//
// The work split. A workgroup is 4 waves and owns 4 neighbouring row groups (64 output columns; the SiLU-gate form: 64
// columns of act = row group n of up AND row group I / 16 + n of gate) over ONE k slice; wave w owns row group
// 4 * blockIdx.x + w for the whole slice, so no two waves ever add into one element. K is cut into `k_splits` slices of
// whole k tiles: slice j covers the k tiles [j * KT / k_splits, (j + 1) * KT / k_splits). The split is a function of
// (N, K) alone (swl_gemm_fp8_row_choose_splits) or forced by the caller — never of M.
//   x       reaches the waves through LDS in chunks of 256 k, one chunk ahead of the one being multiplied (global ->
//           registers while chunk c is multiplied -> LDS, one barrier a chunk, two buffers), rows 528 bytes apart: the
//           staging of gemm_fp8_block.h, kept so that the two FP8 forms differ in the storage form alone — what the
//           measurement is about. All four waves read the same chunk: x crosses the L1 once per 64 columns.
//   codes   global -> registers: a ring of EIGHT 1 KiB tiles per row group (16 KiB for up + gate), a slot asked for again
//           (the tile 512 k ahead) as soon as its codes are dequantised. Eight is the depth at which the row-major kernel
//           was measured; here the eight loads in flight are one contiguous 8 KiB. 4 waves a workgroup keep 2 workgroups a
//           CU inside the register budget of four token tiles. Every code byte is read once for all ceil(M / 16) tiles.
//   scales  not touched by the walk at all: there is NO fold. The MFMAs of a slice chain into one accumulator per token
//           tile, which no VALU instruction reads before the slice ends.
//
// The chain of one output element (row m, column n). A step t is the k tile t; for slice j over tiles [t0_j, t1_j):
//     R_j = 0;  for t = t0_j .. t1_j - 1 (ascending): R_j = mfma(A_lo(t), W_lo(t), R_j); R_j = mfma(A_hi(t), W_hi(t), R_j)
//     sum = (((R_0 + R_1) + R_2) + ...) + R_{k_splits - 1}       (k_splits > 1: fp32 slabs in the caller's workspace, added
//                                                                in slice order by the finishing kernel)
// then y = T(sum *_fp32 scale[n]), or act = fp8_up_gate_act(sum_up, sum_gate, scale[n], scale[I + n]) of moe_fp8.h. Behind
// the MFMAs an element sees k_splits - 1 adds and ONE multiply. The MFMA computes the rows of a token tile independently and
// padding rows are zeros, so a row's bits depend on that row's activations and the weights only — not on M, the row's
// position or the other rows — and a launch of a given (shape, split) is run-to-run deterministic (no atomics).
#pragma once

#include "gemm_host.h"
#include "moe_fp8.h"

namespace swl {

constexpr int kFp8RowMaxM = 64;                             // four token tiles of 16
constexpr int kFp8RowWaves = 4;                             // = row groups of a workgroup
constexpr int kFp8RowChunk = 256;                           // k of x one LDS buffer holds: 4 k tiles
constexpr int kFp8RowRing = 8;                              // k tiles of codes a wave keeps in flight per row group
constexpr int kFp8RowMaxSplits = 8;
constexpr int kFp8RowTileBytes = 16 * kFp8KStep;            // 1 KiB

inline bool fp8_row_geometry_ok(int n, int k) { return n > 0 && k > 0 && n % 16 == 0 && k % kFp8KStep == 0; }

// the first k tile of slice j of ks over kt k tiles (j == ks: kt); every slice is non-empty when ks <= kt
__host__ __device__ inline int fp8_row_split_first(int j, int ks, int kt) { return static_cast<int>(static_cast<int64_t>(j) * kt / ks); }

// byte of the 16 codes lane `lane` owns in tile (nt, kt) of a projection with KT k tiles
__host__ __device__ inline int64_t fp8_row_tile_byte(int nt, int kt, int KT, int lane) {
    return (static_cast<int64_t>(nt) * KT + kt) * kFp8RowTileBytes + 16 * lane;
}

inline bool fp8_row_splits_ok(int ks, int k) {
    return ks >= 1 && ks <= kFp8RowMaxSplits && !(ks & (ks - 1)) && ks <= k / kFp8KStep;
}

// The finishing kernel of a split launch: four neighbouring columns a thread, the slabs added in slice order, then the
// scale and the epilogue of the unsplit kernel. SCALED = false (gemm_mxfp4.hip: the weights carry their scales): `scale` is
// not read and every scale is 1.
template <typename T, bool SILU, bool SCALED = true>
__global__ __launch_bounds__(256) void gemm_fp8_row_finish_kernel(T *__restrict__ out, const float *__restrict__ slabs,
                                                                  const float *__restrict__ scale, int ks, int M, int n_out,
                                                                  int n_w) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int per_row = n_out / 4;
    if (i >= static_cast<int64_t>(M) * per_row) return;
    const int row = static_cast<int>(i / per_row), col = 4 * static_cast<int>(i % per_row);
    const float *p = slabs + static_cast<int64_t>(row) * n_w + col;
    const int64_t slab = static_cast<int64_t>(M) * n_w;
    float4_t a = *reinterpret_cast<const float4_t *>(p), g = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SILU) g = *reinterpret_cast<const float4_t *>(p + n_out);
    for (int j = 1; j < ks; ++j) {
        a += *reinterpret_cast<const float4_t *>(p + j * slab);
        if constexpr (SILU) g += *reinterpret_cast<const float4_t *>(p + j * slab + n_out);
    }
    float4_t sa = {1.f, 1.f, 1.f, 1.f}, sg = {1.f, 1.f, 1.f, 1.f};
    if constexpr (SCALED) sa = *reinterpret_cast<const float4_t *>(scale + col);
    if constexpr (SILU && SCALED) sg = *reinterpret_cast<const float4_t *>(scale + n_out + col);
    typedef T T4 __attribute__((ext_vector_type(4)));
    T4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = SILU ? fp8_up_gate_act<T>(a[e], g[e], sa[e], sg[e]) : to_t<T>(__fmul_rn(a[e], sa[e]));
    *reinterpret_cast<T4 *>(out + static_cast<int64_t>(row) * n_out + col) = o;
}

} // namespace swl
