// moe_fp8.hip — FP8 (e4m3) expert weights for the mixture-of-experts FFN, gfx950: the row quantiser the loader uses and the
// 16-row-tile form of the two expert GEMMs with the codes dequantised in registers. The contract and the walk: moe_fp8.h.
//
//   swl_moe_quantise_rows      rows of T [num_rows, row_len] + fp32 inv [num_rows] -> codes. One wave per row, a lane turns
//                              16 elements (two 16-byte loads) into one 16-byte store and strides the row by 64 x 16.
//   swl_moe_up_gate_silu_fp8   moe.hip's workgroup — (tile, 16 columns of I), 8 waves, the tile's gathered x rows as the M side
//   swl_moe_down_fp8           of v_mfma_f32_16x16x32 — over one-byte weights: 64-wide k steps, one 16-byte load of codes per
//                              lane and weight row block feeding two MFMAs, kDepth = 4 steps of loads in flight before their
//                              MFMAs (the bytes of weights a wave has in flight are those of the 16-bit kernel: 4 x 16 bytes
//                              a lane and row block, covering twice the k). The eight waves are added in wave order through
//                              LDS, the sum is multiplied once by the row's scale, then the epilogue of the 16-bit kernels.
//
// They read the tables of swl_moe_align and take the grids of their 16-bit twins — (max_tiles, I / 16) and (max_tiles,
// H / 16): functions of (tokens, k, E) and the geometry alone. A row's sums never see another row's data, and their order is
// fixed by (H, I) alone. Unused tiles leave before any barrier. moe_fp8_wide.hip holds the row-tile form (same bits).
#include "moe_fp8.h"

namespace swl {

template <typename T>
__global__ __launch_bounds__(256) void moe_quantise_rows_kernel(uint8_t *__restrict__ codes, const T *__restrict__ rows,
                                                                const float *__restrict__ inv, int64_t num_rows,
                                                                int row_len) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = blockIdx.x * 4ll + wave; r < num_rows; r += static_cast<int64_t>(gridDim.x) * 4ll) {
        const float s = inv[r];
        const T *src = rows + r * row_len;
        uint8_t *dst = codes + r * row_len;
        for (int c = 16 * lane; c < row_len; c += 16 * 64)
            *reinterpret_cast<u32x4_t *>(dst + c) = quantise16<T>(load8(src + c), load8(src + c + 8), s);
    }
}

// One (tile, 16 output columns) block of rows(A)[16, K] x dequantised(W[e][n0 .. n0 + 16, K])^T for NB weight row blocks
// `nb_stride` bytes apart that share the A rows. Leaves the sums, added in wave order, in `sum[b]` of the thread that owns
// (row tid >> 4, column tid & 15), tid < 256.
template <typename T, int NB>
__device__ __forceinline__ void moe_fp8_tile_gemm(float (&sum)[NB], float (*red)[kMoeWaves][16][16], const T *__restrict__ a,
                                                  int64_t a_row, bool a_on, const uint8_t *__restrict__ w, int64_t nb_stride,
                                                  int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const T *ap = a + a_row + 16 * q;
    const uint8_t *wp = w + static_cast<int64_t>(i16) * K + 16 * q;
    float4_t acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = float4_t{0.f, 0.f, 0.f, 0.f};
    constexpr int kDepth = 4;                               // k steps of loads in flight before their MFMAs
    int k = kFp8KStep * wave;
    for (; k + (kDepth - 1) * kFp8Round < K; k += kDepth * kFp8Round) {
        Fp8AFrag<T> af[kDepth];
        u32x4_t wf[NB][kDepth];
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            af[u] = fp8_load_a(ap + k + u * kFp8Round, a_on);
#pragma unroll
            for (int b = 0; b < NB; ++b) wf[b][u] = load16b_nt(wp + b * nb_stride + k + u * kFp8Round);
        }
#pragma unroll
        for (int u = 0; u < kDepth; ++u)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = fp8_step_mfma<T>(af[u], wf[b][u], acc[b]);
    }
    for (; k < K; k += kFp8Round) {
        const Fp8AFrag<T> af = fp8_load_a(ap + k, a_on);
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = fp8_step_mfma<T>(af, load16b_nt(wp + b * nb_stride + k), acc[b]);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) mfma_results_tie(acc[b]);
    mfma_results_ready<4>(acc[NB - 1]);
    // acc[b][r] = partial of (tile row 4q + r, column i16)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[b][wave][4 * q + r][i16] = acc[b][r];
    __syncthreads();
    if (threadIdx.x < 256) {
#pragma unroll
        for (int b = 0; b < NB; ++b) sum[b] = fp8_wave_sum(red[b], threadIdx.x >> 4, threadIdx.x & 15);
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kMoeWaves) void moe_up_gate_silu_fp8_kernel(
    T *__restrict__ act, const T *__restrict__ x, const uint8_t *__restrict__ w, const float *__restrict__ scale,
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
    float sum[2];
    moe_fp8_tile_gemm<T, 2>(sum, red, x, tok * x_row_stride, on, w + up_row * H, static_cast<int64_t>(I) * H, H);
    if (threadIdx.x >= 256) return;
    const int orow = tile_rows[tile * 16 + (threadIdx.x >> 4)];
    if (orow < 0 || orow >= P) return;
    const int cc = threadIdx.x & 15;
    act[static_cast<int64_t>(orow) * I + n0 + cc] =
        fp8_up_gate_act<T>(sum[0], sum[1], scale[up_row + cc], scale[up_row + I + cc]);
}

template <typename T>
__global__ __launch_bounds__(64 * kMoeWaves) void moe_down_fp8_kernel(float *__restrict__ y, const T *__restrict__ act,
                                                                      const uint8_t *__restrict__ w,
                                                                      const float *__restrict__ scale,
                                                                      const int32_t *__restrict__ tile_rows,
                                                                      const int32_t *__restrict__ tile_experts, int P, int H,
                                                                      int I, int E) {
    __shared__ __attribute__((aligned(16))) float red[1][kMoeWaves][16][16];
    const int tile = blockIdx.x;
    const int e = tile_experts[tile];
    if (e < 0 || e >= E) return;                            // (uniform; before the barrier)
    const int n0 = blockIdx.y * 16;
    int pair = tile_rows[tile * 16 + (threadIdx.x & 15)];
    if (pair >= P) pair = -1;
    const bool on = pair >= 0;
    const int64_t w_row = static_cast<int64_t>(e) * H + n0;
    float sum[1];
    moe_fp8_tile_gemm<T, 1>(sum, red, act, (on ? pair : 0) * static_cast<int64_t>(I), on, w + w_row * I, 0, I);
    if (threadIdx.x >= 256) return;
    const int orow = tile_rows[tile * 16 + (threadIdx.x >> 4)];
    if (orow < 0 || orow >= P) return;
    const int cc = threadIdx.x & 15;
    y[static_cast<int64_t>(orow) * H + n0 + cc] = __fmul_rn(sum[0], scale[w_row + cc]);
}

} // namespace swl

extern "C" int swl_moe_fp8_supported(int32_t hidden, int32_t inter, int32_t num_experts, int32_t top_k, int32_t dtype) {
    if (!swl::moe_dtype_ok(dtype) || !swl::moe_fp8_geometry_ok(hidden, inter)) return 0;
    if (num_experts <= 0 || num_experts > swl::kMoeMaxExperts) return 0;
    if (top_k <= 0 || top_k > swl::kMoeMaxTopK || top_k > num_experts) return 0;
    return 1;
}

extern "C" int swl_moe_quantise_rows(void *codes, const void *rows, const float *inv, int64_t num_rows, int32_t row_len,
                                     int32_t dtype, swl_stream_t stream) {
    if (num_rows < 0 || row_len <= 0 || !swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (row_len % 16 != 0) return SWL_ERR_UNSUPPORTED;
    if (num_rows == 0) return SWL_OK;
    if (!codes || !rows || !inv || !swl::aligned16(codes) || !swl::aligned16(rows)) return SWL_ERR_BAD_ARG;
    const int64_t blocks = (num_rows + 3) / 4;
    const unsigned grid = static_cast<unsigned>(blocks < 65536 ? blocks : 65536);
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::moe_quantise_rows_kernel<T>), dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<uint8_t *>(codes), static_cast<const T *>(rows), inv, num_rows, row_len);
    });
    return swl::check_launch();
}

extern "C" int swl_moe_up_gate_silu_fp8(void *act, const void *x, const void *expert_up_gate, const float *up_gate_scale,
                                        const int32_t *tile_rows, const int32_t *tile_experts, int32_t max_tiles,
                                        int32_t num_tokens, int32_t top_k, int32_t hidden, int32_t inter, int32_t num_experts,
                                        int64_t x_row_stride, int32_t dtype, swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0 || x_row_stride < hidden) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_fp8_supported(hidden, inter, num_experts, top_k, dtype) || x_row_stride % 8 != 0) return SWL_ERR_UNSUPPORTED;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!act || !x || !expert_up_gate || !up_gate_scale || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(x) || !swl::aligned16(expert_up_gate)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>(max_tiles), static_cast<unsigned>(inter / 16));
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::moe_up_gate_silu_fp8_kernel<T>), grid, dim3(64 * swl::kMoeWaves), 0,
                           static_cast<hipStream_t>(stream), static_cast<T *>(act), static_cast<const T *>(x),
                           static_cast<const uint8_t *>(expert_up_gate), up_gate_scale, tile_rows, tile_experts,
                           num_tokens * top_k, top_k, hidden, inter, num_experts, x_row_stride);
    });
    return swl::check_launch();
}

extern "C" int swl_moe_down_fp8(float *y, const void *act, const void *expert_down, const float *down_scale,
                                const int32_t *tile_rows, const int32_t *tile_experts, int32_t max_tiles, int32_t num_tokens,
                                int32_t top_k, int32_t hidden, int32_t inter, int32_t num_experts, int32_t dtype,
                                swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_fp8_supported(hidden, inter, num_experts, top_k, dtype)) return SWL_ERR_UNSUPPORTED;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!y || !act || !expert_down || !down_scale || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(act) || !swl::aligned16(expert_down)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>(max_tiles), static_cast<unsigned>(hidden / 16));
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::moe_down_fp8_kernel<T>), grid, dim3(64 * swl::kMoeWaves), 0,
                           static_cast<hipStream_t>(stream), y, static_cast<const T *>(act),
                           static_cast<const uint8_t *>(expert_down), down_scale, tile_rows, tile_experts,
                           num_tokens * top_k, hidden, inter, num_experts);
    });
    return swl::check_launch();
}
