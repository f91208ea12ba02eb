// gemm_fp8_block.h — the BLOCK-SCALED FP8 (OCP e4m3fn) contract of the DENSE projections (q/k/v, o, up/gate, down of a
// Llama-shaped model whose checkpoint was written by the fine-grained FP8 quantiser: quant_method fp8, fmt e4m3,
// weight_block_size [128, 128]) and the host / device arithmetic gemm_fp8_block.hip shares with its callers, gfx950.
// DESIGN.md section 4.22. The load shape of the codes, the A/B fragment permutation and the exact dequantisation are
// moe_fp8.h's; the fold and the SiLU-gate epilogue are moe_fp8_block.h's.
//
// Storage. A projection is codes [N, K]: one e4m3fn byte per element, row-major, ONE copy — the checkpoint's own bytes. A
// fused projection is a row-wise concatenation of at most three SEGMENTS (qkv_proj = [q ; k ; v], up_gate_proj = [up ; gate];
// o_proj and down_proj are one segment), and every segment keeps the scale rows of the tensor it came from. With
// RB(x) = KB(x) = ceil(x / 128):
//   bscale   fp32 [sum_s RB(rows_s), KB(K)]; row block r of segment s is scale row  sum_{s' < s} RB(rows_s') + r
//            (NOT (first row of s + 128 r) / 128: the two differ when a segment is no multiple of 128 rows).
// The weight MEANS fp(code) * bscale[that scale row][k / 128]. K % 64 == 0; every segment is a multiple of 16 rows, so a
// 16-column tile lies inside one segment and one row block; a last row block or k block may be partial. NaN codes (0x7f,
// 0xff) dequantise to NaN and propagate: no special case.
//
// The work split. A workgroup is 4 waves and owns 4 neighbouring 16-column tiles (64 output columns; the SiLU-gate form: 64
// columns of act = tile n of up AND tile I / 16 + n of gate) over ONE k slice; wave w owns tile 4 * blockIdx.x + w for the
// whole slice, so no two waves ever add into one element. K is cut into `k_splits` slices of whole 128-wide k blocks: slice
// j covers the k blocks [j * KB / k_splits, (j + 1) * KB / k_splits). The split is a function of (N, K) alone
// (swl_gemm_fp8_block_choose_splits) or forced by the caller — never of M.
//   x        reaches the waves through LDS in chunks of 256 k: the whole workgroup loads the chunk's rows as full lines (32
//            lanes x 16 bytes = one row's 512 contiguous bytes, two rows an instruction), one chunk ahead of the one being
//            multiplied (global -> registers while chunk c is multiplied -> LDS, one barrier a chunk, two buffers). Rows
//            are 528 bytes apart in LDS, so the sixteen rows an A-fragment read touches fall into sixteen distinct 16-byte
//            bank groups. All four waves read the same chunk: x crosses the L1 once per 64 columns, not once per tile.
//   codes    16 bytes a lane, 16 rows x 64 contiguous bytes = 1 KiB per wave, tile and 64-wide step (moe_fp8.h). A wave keeps
//            EIGHT steps in flight per tile (8 KiB; 16 KiB for up + gate): a ring of two chunks' codes in registers, and a
//            slot is asked for again (the step 512 k ahead) as soon as its codes are dequantised. Every weight byte is
//            read once for all ceil(M / 16) token tiles: up to four tiles of running sums and partials live in registers.
//   scales   one scalar load per tile and k block (fp8_bscale_row of moe_fp8_block.h): wave-uniform, never per lane.
//
// The chain of one output element (row m, column n; s[b] = bscale[scale row of n][b]). A step t is 64 wide and lies in k
// block t / 2. For the slice j = 0 .. k_splits - 1 that holds k blocks [b0_j, b1_j):
//     R_j = 0
//     for b = b0_j .. b1_j - 1 (ascending):
//         P = 0
//         for t = 2 b, 2 b + 1 (while 64 t < K): P = mfma(A_lo(t), W_lo(t), P); P = mfma(A_hi(t), W_hi(t), P)
//         R_j = fmaf(P, s[b], R_j)                                        (the FOLD: one rounding per k BLOCK)
//     sum = (((R_0 + R_1) + R_2) + ...) + R_{k_splits - 1}                 (k_splits > 1: fp32 slabs in the caller's workspace,
//                                                                          added in slice order by the finishing kernel)
// then y = T(sum), or up, gate = T(sum); act = up *_T T(silu(gate)) (fp8_block_up_gate_act). An element is folded KB(K)
// times and merged k_splits - 1 times: F = KB(K) + k_splits - 1 fp32 roundings behind the MFMAs. The fold is per k block and
// not per 64-wide step as in the expert GEMMs: a wave here walks consecutive steps, so both steps of a block are its own,
// and half the folds is half the VALU work between the MFMAs. The MFMA computes the rows of a token tile independently and
// padding rows are zeros, so a row's bits depend on that row's activations and the weights only — not on M, the row's
// position or the other rows — and a launch of a given (shape, split) is run-to-run deterministic (no atomics).
#pragma once

#include "gemm_host.h"
#include "moe_fp8_block.h"

namespace swl {

constexpr int kGemmFp8MaxM = 64;                            // four token tiles of 16
constexpr int kGemmFp8Waves = 4;                            // = column tiles of a workgroup
constexpr int kGemmFp8Chunk = 256;                          // k of x one LDS buffer holds: 4 steps, 2 k blocks
constexpr int kGemmFp8MaxSplits = 8;
constexpr int kGemmFp8MaxSegments = 3;

struct Fp8Segments {
    int rows[kGemmFp8MaxSegments];                          // unused segments: 0
};

__host__ __device__ inline int fp8_segments_rows(const Fp8Segments &s) { return s.rows[0] + s.rows[1] + s.rows[2]; }

__host__ __device__ inline int fp8_segments_scale_rows(const Fp8Segments &s) {
    return moe_fp8_blocks(s.rows[0]) + moe_fp8_blocks(s.rows[1]) + moe_fp8_blocks(s.rows[2]);
}

// the scale row of weight row `row` of the concatenation
__host__ __device__ inline int fp8_segments_scale_row(const Fp8Segments &s, int row) {
    int base = 0, sr = 0;
#pragma unroll
    for (int i = 0; i < kGemmFp8MaxSegments - 1; ++i) {
        if (row < base + s.rows[i]) break;
        base += s.rows[i];
        sr += moe_fp8_blocks(s.rows[i]);
    }
    return sr + (row - base) / kFp8BlockSide;
}

// the first k block of slice j of ks over kb k blocks (j == ks: kb); every slice is non-empty when ks <= kb
__host__ __device__ inline int fp8_split_first_block(int j, int ks, int kb) { return static_cast<int>(static_cast<int64_t>(j) * kb / ks); }

inline bool gemm_fp8_geometry_ok(int k) { return k > 0 && k % kFp8KStep == 0; }

inline bool gemm_fp8_segments_ok(const Fp8Segments &s) {
    bool ended = false;
    for (int i = 0; i < kGemmFp8MaxSegments; ++i) {
        if (s.rows[i] < 0 || s.rows[i] % 16 || (ended && s.rows[i] > 0)) return false;
        ended |= s.rows[i] == 0;
    }
    return s.rows[0] > 0;
}

// The finishing kernel of a split launch: four neighbouring columns a thread, the slabs added in slice order.
template <typename T, bool SILU>
__global__ __launch_bounds__(256) void gemm_fp8_block_finish_kernel(T *__restrict__ out, const float *__restrict__ slabs, int ks,
                                                                    int M, int n_out, int n_w) {
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
    typedef T T4 __attribute__((ext_vector_type(4)));
    T4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = SILU ? fp8_block_up_gate_act<T>(a[e], g[e]) : to_t<T>(a[e]);
    *reinterpret_cast<T4 *>(out + static_cast<int64_t>(row) * n_out + col) = o;
}

// ---- host: what the entries of gemm_fp8_block.hip and gemm_fp8_block_wide.hip check alike ----
inline bool splits_ok(int ks, int k) { return ks >= 1 && ks <= kGemmFp8MaxSplits && !(ks & (ks - 1)) && ks <= moe_fp8_blocks(k); }

// What both GEMM entries check alike, in this order: counts (M == 0 leaves with SWL_OK), operands, shape, strides,
// alignment (gemm_host.h), then the scale table's block counts, the split and the workspace. `a.N` is the number of output
// columns, `n_w` of weight rows, `chosen` what the ENTRY'S OWN chooser answers for the shape (used where k_splits is 0).
inline bool fp8_gemm_settled(const GemmArgs &a, const float *bscale, const Fp8Segments &seg, int n_w, int scale_rows,
                             int k_blocks, int chosen, int &ks, int &rc) {
    if ((rc = check_gemm_counts(a)) != SWL_OK || a.M == 0) return true;
    if ((rc = check_gemm_operands(a)) != SWL_OK) return true;
    if (!bscale) return rc = SWL_ERR_BAD_ARG, true;
    if (a.M > a.max_m || !gemm_fp8_geometry_ok(a.K) || !gemm_fp8_segments_ok(seg)) return rc = SWL_ERR_UNSUPPORTED, true;
    if ((rc = check_gemm_strides(a)) != SWL_OK || (rc = check_gemm_alignment(a)) != SWL_OK) return true;
    if (scale_rows != fp8_segments_scale_rows(seg) || k_blocks != moe_fp8_blocks(a.K)) return rc = SWL_ERR_BAD_ARG, true;
    ks = a.k_splits ? a.k_splits : chosen;
    if (!splits_ok(ks, a.K)) return rc = SWL_ERR_BAD_ARG, true;
    if (ks > 1 && (!a.workspace || a.workspace_bytes < static_cast<size_t>(ks) * a.M * n_w * sizeof(float)))
        return rc = SWL_ERR_BAD_ARG, true;
    return false;
}

} // namespace swl
