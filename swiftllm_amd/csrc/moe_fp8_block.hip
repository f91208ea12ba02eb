// moe_fp8_block.hip — block-scaled FP8 (e4m3, one fp32 scale per 128 x 128 block) expert weights for the mixture-of-experts
// FFN, gfx950: the 16-row-tile form of the two expert GEMMs. The contract and the chain: moe_fp8_block.h.
//
//   swl_moe_up_gate_silu_fp8_block   moe_fp8.hip's workgroup and load shape — (tile, 16 columns), 8 waves, 64-wide k steps,
//   swl_moe_down_fp8_block           one 16-byte load of codes per lane and weight row block, kDepth = 4 steps of loads in
//                                    flight before their MFMAs — with a walk of its own: the scale changes every 128 k, so a
//                                    step's two MFMAs start from a zero accumulator and their partial is folded into the
//                                    wave's running sum with one fmaf by the step's scale. The scales of a workgroup are one
//                                    row of KB floats (down) or two (up and gate): each step's scale is a scalar load issued
//                                    with the step's vector loads. The eight running sums are added in wave order through
//                                    LDS; then the epilogue of the 16-bit kernels.
//
// They read the tables of swl_moe_align and take the grids of their twins — (max_tiles, I / 16) and (max_tiles, H / 16).
// Unused tiles leave before any barrier. moe_fp8_block_wide.hip holds the row-tile form (same bits).
#include "moe_fp8_block.h"

namespace swl {

// One (tile, 16 output columns) block of rows(A)[16, K] x (dequantised(W[e][n0 .. n0 + 16, K]) * s[k / 128])^T for NB weight
// row blocks `nb_stride` bytes apart that share the A rows; sc[b] is the scale row (KB floats) of row block b. Leaves the
// sums, added in wave order, in `sum[b]` of the thread that owns (row tid >> 4, column tid & 15), tid < 256.
template <typename T, int NB>
__device__ __forceinline__ void moe_fp8_block_tile_gemm(float (&sum)[NB], float (*red)[kMoeWaves][16][16],
                                                        const T *__restrict__ a, int64_t a_row, bool a_on,
                                                        const uint8_t *__restrict__ w, int64_t nb_stride,
                                                        const fp8_bscale_ptr (&sc)[NB], int K) {
    const int lane = threadIdx.x & 63, wave = fp8_block_wave();
    const int i16 = lane & 15, q = lane >> 4;
    const T *ap = a + a_row + 16 * q;
    const uint8_t *wp = w + static_cast<int64_t>(i16) * K + 16 * q;
    float4_t run[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) run[b] = float4_t{0.f, 0.f, 0.f, 0.f};
    constexpr int kDepth = 4;                               // k steps of loads in flight before their MFMAs
    int k = kFp8KStep * wave;                               // (uniform)
    for (; k + (kDepth - 1) * kFp8Round < K; k += kDepth * kFp8Round) {
        Fp8AFrag<T> af[kDepth];
        u32x4_t wf[NB][kDepth];
        float s[NB][kDepth];
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            af[u] = fp8_load_a(ap + k + u * kFp8Round, a_on);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                wf[b][u] = load16b_nt(wp + b * nb_stride + k + u * kFp8Round);
                s[b][u] = sc[b][(k + u * kFp8Round) / kFp8BlockSide];
            }
        }
        float4_t p[NB][kDepth];
#pragma unroll
        for (int u = 0; u < kDepth; ++u)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                p[b][u] = fp8_block_partial<T>(af[u], wf[b][u]);
                mfma_results_tie(p[b][u]);
            }
        mfma_results_ready<4>(p[NB - 1][kDepth - 1]);
#pragma unroll
        for (int u = 0; u < kDepth; ++u)                    // steps ascending
#pragma unroll
            for (int b = 0; b < NB; ++b) run[b] = fp8_block_fold(p[b][u], s[b][u], run[b]);
    }
    for (; k < K; k += kFp8Round) {
        const Fp8AFrag<T> af = fp8_load_a(ap + k, a_on);
        float4_t p[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            p[b] = fp8_block_partial<T>(af, load16b_nt(wp + b * nb_stride + k));
            mfma_results_tie(p[b]);
        }
        mfma_results_ready<4>(p[NB - 1]);
#pragma unroll
        for (int b = 0; b < NB; ++b) run[b] = fp8_block_fold(p[b], sc[b][k / kFp8BlockSide], run[b]);
    }
    // run[b][r] = running sum of (tile row 4q + r, column i16): VALU results, no matrix-pipe wait to pad
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[b][wave][4 * q + r][i16] = run[b][r];
    __syncthreads();
    if (threadIdx.x < 256) {
#pragma unroll
        for (int b = 0; b < NB; ++b) sum[b] = fp8_wave_sum(red[b], threadIdx.x >> 4, threadIdx.x & 15);
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kMoeWaves) void moe_up_gate_silu_fp8_block_kernel(
    T *__restrict__ act, const T *__restrict__ x, const uint8_t *__restrict__ w, const float *__restrict__ bscale,
    const int32_t *__restrict__ tile_rows, const int32_t *__restrict__ tile_experts, int P, int top_k, int H, int I, int E,
    int64_t x_row_stride) {
    __shared__ __attribute__((aligned(16))) float red[2][kMoeWaves][16][16];
    const int tile = blockIdx.x;
    const int e = tile_experts[tile];
    if (e < 0 || e >= E) return;                            // (uniform; before the barrier)
    const int n0 = blockIdx.y * 16;
    int pair = tile_rows[tile * 16 + (threadIdx.x & 15)];
    if (pair >= P) pair = -1;
    const bool on = pair >= 0;
    const int64_t tok = on ? pair / top_k : 0;
    const int64_t up_row = static_cast<int64_t>(e) * 2 * I + n0;
    const int rb = moe_fp8_blocks(I), kb = moe_fp8_blocks(H);
    // up's row block n0 / 128 of expert e, and gate's: rb row blocks further
    const float *s_up = bscale + (static_cast<int64_t>(e) * 2 * rb + n0 / kFp8BlockSide) * kb;
    const fp8_bscale_ptr sc[2] = {fp8_bscale_row(s_up), fp8_bscale_row(s_up + static_cast<int64_t>(rb) * kb)};
    float sum[2];
    moe_fp8_block_tile_gemm<T, 2>(sum, red, x, tok * x_row_stride, on, w + up_row * H, static_cast<int64_t>(I) * H, sc, H);
    if (threadIdx.x >= 256) return;
    const int orow = tile_rows[tile * 16 + (threadIdx.x >> 4)];
    if (orow < 0 || orow >= P) return;
    act[static_cast<int64_t>(orow) * I + n0 + (threadIdx.x & 15)] = fp8_block_up_gate_act<T>(sum[0], sum[1]);
}

template <typename T>
__global__ __launch_bounds__(64 * kMoeWaves) void moe_down_fp8_block_kernel(
    float *__restrict__ y, const T *__restrict__ act, const uint8_t *__restrict__ w, const float *__restrict__ bscale,
    const int32_t *__restrict__ tile_rows, const int32_t *__restrict__ tile_experts, int P, int H, int I, int E) {
    __shared__ __attribute__((aligned(16))) float red[1][kMoeWaves][16][16];
    const int tile = blockIdx.x;
    const int e = tile_experts[tile];
    if (e < 0 || e >= E) return;                            // (uniform; before the barrier)
    const int n0 = blockIdx.y * 16;
    int pair = tile_rows[tile * 16 + (threadIdx.x & 15)];
    if (pair >= P) pair = -1;
    const bool on = pair >= 0;
    const int64_t w_row = static_cast<int64_t>(e) * H + n0;
    const int rb = moe_fp8_blocks(H), kb = moe_fp8_blocks(I);
    const fp8_bscale_ptr sc[1] = {fp8_bscale_row(bscale + (static_cast<int64_t>(e) * rb + n0 / kFp8BlockSide) * kb)};
    float sum[1];
    moe_fp8_block_tile_gemm<T, 1>(sum, red, act, (on ? pair : 0) * static_cast<int64_t>(I), on, w + w_row * I, 0, sc, I);
    if (threadIdx.x >= 256) return;
    const int orow = tile_rows[tile * 16 + (threadIdx.x >> 4)];
    if (orow < 0 || orow >= P) return;
    y[static_cast<int64_t>(orow) * H + n0 + (threadIdx.x & 15)] = sum[0];
}

} // namespace swl

extern "C" int swl_moe_fp8_block_supported(int32_t hidden, int32_t inter, int32_t num_experts, int32_t top_k, int32_t dtype) {
    return swl_moe_fp8_supported(hidden, inter, num_experts, top_k, dtype);
}

extern "C" int swl_moe_up_gate_silu_fp8_block(void *act, const void *x, const void *expert_up_gate,
                                              const float *up_gate_bscale, int32_t row_blocks, int32_t k_blocks,
                                              const int32_t *tile_rows, const int32_t *tile_experts, int32_t max_tiles,
                                              int32_t num_tokens, int32_t top_k, int32_t hidden, int32_t inter,
                                              int32_t num_experts, int64_t x_row_stride, int32_t dtype, swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0 || x_row_stride < hidden) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_fp8_block_supported(hidden, inter, num_experts, top_k, dtype) || x_row_stride % 8 != 0)
        return SWL_ERR_UNSUPPORTED;
    if (row_blocks != swl::moe_fp8_blocks(inter) || k_blocks != swl::moe_fp8_blocks(hidden)) return SWL_ERR_BAD_ARG;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!act || !x || !expert_up_gate || !up_gate_bscale || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(x) || !swl::aligned16(expert_up_gate)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>(max_tiles), static_cast<unsigned>(inter / 16));
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::moe_up_gate_silu_fp8_block_kernel<T>), grid, dim3(64 * swl::kMoeWaves), 0,
                           static_cast<hipStream_t>(stream), static_cast<T *>(act), static_cast<const T *>(x),
                           static_cast<const uint8_t *>(expert_up_gate), up_gate_bscale, tile_rows, tile_experts,
                           num_tokens * top_k, top_k, hidden, inter, num_experts, x_row_stride);
    });
    return swl::check_launch();
}

extern "C" int swl_moe_down_fp8_block(float *y, const void *act, const void *expert_down, const float *down_bscale,
                                      int32_t row_blocks, int32_t k_blocks, const int32_t *tile_rows,
                                      const int32_t *tile_experts, int32_t max_tiles, int32_t num_tokens, int32_t top_k,
                                      int32_t hidden, int32_t inter, int32_t num_experts, int32_t dtype,
                                      swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_fp8_block_supported(hidden, inter, num_experts, top_k, dtype)) return SWL_ERR_UNSUPPORTED;
    if (row_blocks != swl::moe_fp8_blocks(hidden) || k_blocks != swl::moe_fp8_blocks(inter)) return SWL_ERR_BAD_ARG;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!y || !act || !expert_down || !down_bscale || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(act) || !swl::aligned16(expert_down)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>(max_tiles), static_cast<unsigned>(hidden / 16));
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::moe_down_fp8_block_kernel<T>), grid, dim3(64 * swl::kMoeWaves), 0,
                           static_cast<hipStream_t>(stream), y, static_cast<const T *>(act),
                           static_cast<const uint8_t *>(expert_down), down_bscale, tile_rows, tile_experts,
                           num_tokens * top_k, hidden, inter, num_experts);
    });
    return swl::check_launch();
}
