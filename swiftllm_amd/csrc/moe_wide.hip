// moe_wide.hip — the expert GEMMs of moe.hip in a weight-reusing row-tile form for prompt-sized steps, gfx950.
//
// moe.hip's workgroup is ONE 16-row tile of one expert x 16 output columns: every tile streams its expert's weights again,
// which is right for decode (an expert has a row or two) and wrong for a prompt (an expert has hundreds). Here a workgroup is
//
//     (MT consecutive tile slots)  x  (NT * 16 output columns)  x  NB weight row blocks (2: up and gate, 1: down),  8 waves,
//
// and per 32-wide k step a wave holds MT A fragments (the gathered rows of MT tiles) and NT * NB W fragments and issues
// MT * NT * NB v_mfma_f32_16x16x32 into as many float4 accumulators: a column block of the weights is fetched once per RUN of
// tiles instead of once per tile, and an A fragment feeds NT * NB MFMAs instead of NB.
//
// The bits are those of the 16-row kernels, on every row. What fixes an output element's sum there is kept here:
//   * wave w of 8 accumulates the k steps w, w + 8, ... in ascending order, from a zero accumulator (the MFMA's rows and
//     columns are independent: more tiles or column blocks under one wave change no element's chain),
//   * the eight partials are added in wave order 0..7 in fp32 (`wide_block_sum`),
//   * up and gate are rounded to T, silu is evaluated in fp32 and rounded to T, the product is rounded to T; y stays fp32.
// So a token's FFN does not depend on which form served the step, and the choice can follow the step's size.
//
// Runs. Slots [g * MT, g * MT + MT) belong to workgroup column g. An expert's tiles are consecutive in tile_experts, so the
// workgroup walks its slots as sub-runs: maximal stretches of ONE expert (length 1..MT), each one pass over the weights with
// the tiles beyond the stretch as rows of zeros. Slots with tile_experts outside [0, E) are skipped, as the 16-row kernels
// skip them. Everything that decides the walk is read from tile_experts at workgroup-uniform addresses: a workgroup whose
// slots are all unused leaves before any barrier, and every barrier inside a sub-run is reached by all 512 threads. The
// tables of swl_moe_align are used as they are; the grid is (ceil(max_tiles / MT), columns / (16 NT)): (T, k, E) alone.
//
// Operands come straight from global memory as 16-byte fragments, the k step after the current one in flight behind the
// current one's MFMAs (two register sets); staging them through LDS as full lines is not built. The epilogue goes through
// LDS one tile at a time (NT * NB blocks of 8 x 16 x 16 partials, two buffers so a pass costs one barrier): 64 KiB whatever MT.
//
// MT is 2 or 4. MT = 8 (32 accumulators = 128 VGPRs next to 2 x 48 of fragments) does not fit the 256 VGPRs a wave has at
// 8 waves a workgroup: the compiler spills 15 - 60 registers to scratch in every arrangement tried, so it is not shipped.
//
// Forcing this form on a step with few rows per expert is for tests and measurements: a sub-run issues all MT * NT * NB MFMAs
// whatever its length, and a workgroup whose slots hold MT different experts walks them one after the other.
#include "attn_mfma.h"
#include "moe_common.h"

namespace swl {

constexpr int kWideThreads = 64 * kMoeWaves;
constexpr int kWideBlocks = 4;            // NT * NB: 16 x 16 blocks per tile and pass (up/gate: 2 x 2, down: 4 x 1)

typedef float WideRed[kWideBlocks][kMoeWaves][16][16];

inline bool moe_wide_tiles_ok(int row_tiles) { return row_tiles == 2 || row_tiles == 4; }

// red[0] + red[1] + ... + red[7] of one element: the order of moe_tile_gemm
__device__ __forceinline__ float wide_block_sum(const float (*blk)[16][16], int rr, int cc) {
    float s = blk[0][rr][cc];
#pragma unroll
    for (int wv = 1; wv < kMoeWaves; ++wv) s += blk[wv][rr][cc];
    return s;
}

// The first slot at or after `s` (below `end`) that holds a tile, its expert and the length of the stretch of that expert:
// all three workgroup-uniform. Returns false when no tile is left.
__device__ __forceinline__ bool wide_next_run(const int32_t *__restrict__ tile_experts, int &s, int end, int E, int &e,
                                              int &run) {
    for (; s < end; ++s) {
        e = __builtin_amdgcn_readfirstlane(tile_experts[s]);
        if (e >= 0 && e < E) break;
    }
    if (s >= end) return false;
    run = 1;
    while (s + run < end && __builtin_amdgcn_readfirstlane(tile_experts[s + run]) == e) ++run;
    return true;
}

// rows(A)[MT x 16, K] x W[n0 .. n0 + 16 NT, K]^T for NB weight row blocks `nb_stride` elements apart that share the A rows.
// a_row[m] / a_on[m]: this lane's row (i16 = lane & 15) of tile m. `emit(m, buf)` runs once per live tile m < run after a
// barrier, with the eight waves' partials of block c = n * NB + b in buf[c]; it must not write LDS.
template <typename T, int MT, int NT, int NB, typename Emit>
__device__ __forceinline__ void moe_wide_gemm(WideRed *red, const T *__restrict__ a, const int64_t (&a_row)[MT],
                                              const bool (&a_on)[MT], const T *__restrict__ w, int64_t nb_stride, int K,
                                              int run, Emit emit) {
    static_assert(NT * NB == kWideBlocks, "one tile per epilogue pass");
    constexpr int NW = NT * NB, kStep = 32 * kMoeWaves;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const T *ap = a + 8 * q;
    const T *wp = w + static_cast<int64_t>(i16) * K + 8 * q;
    vec8_t<T> zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = to_t<T>(0.f);
    float4_t acc[MT][NW];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int c = 0; c < NW; ++c) acc[m][c] = float4_t{0.f, 0.f, 0.f, 0.f};

    auto fetch = [&](vec8_t<T>(&af)[MT], vec8_t<T>(&wf)[NW], int k) {
#pragma unroll
        for (int c = 0; c < NW; ++c)
            wf[c] = load8_nt(wp + (c % NB) * nb_stride + static_cast<int64_t>((c / NB) * 16) * K + k);
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = a_on[m] ? load8(ap + a_row[m] + k) : zero;
    };
    auto multiply = [&](const vec8_t<T>(&af)[MT], const vec8_t<T>(&wf)[NW]) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int c = 0; c < NW; ++c) acc[m][c] = mfma16x32(af[m], wf[c], acc[m][c]);
    };
    // wave w: k steps w, w + 8, ... ascending; the step after the current one is in flight behind its MFMAs
    const int k0 = 32 * wave;
    const int steps = K > k0 ? (K - k0 + kStep - 1) / kStep : 0;
    vec8_t<T> a0[MT], w0[NW], a1[MT], w1[NW];
    if (steps > 0) fetch(a0, w0, k0);
    for (int s = 0; s < steps; s += 2) {
        const bool pair = s + 1 < steps;
        if (pair) fetch(a1, w1, k0 + (s + 1) * kStep);
        multiply(a0, w0);
        if (pair) {
            if (s + 2 < steps) fetch(a0, w0, k0 + (s + 2) * kStep);
            multiply(a1, w1);
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int c = 0; c < NW; ++c) mfma_results_tie(acc[m][c]);
    mfma_results_ready<4>(acc[MT - 1][NW - 1]);

    // acc[m][c][r] = partial of (row 4q + r of tile m, column i16 of block c). One tile per pass, alternating buffers: a
    // buffer is written again two passes later, behind the barrier all readers of its last use have passed.
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (m < run) {                                      // (uniform)
            float(*buf)[kMoeWaves][16][16] = red[m & 1];
#pragma unroll
            for (int c = 0; c < NW; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) buf[c][wave][4 * q + r][i16] = acc[m][c][r];
            __syncthreads();
            emit(m, buf);
        }
    }
    __syncthreads();                                        // the next sub-run writes red[0] again
}

template <typename T, int MT>
__global__ __launch_bounds__(kWideThreads) void moe_up_gate_silu_wide_kernel(
    T *__restrict__ act, const T *__restrict__ x, const T *__restrict__ w, const int32_t *__restrict__ tile_rows,
    const int32_t *__restrict__ tile_experts, int max_tiles, int P, int top_k, int H, int I, int E, int64_t x_row_stride) {
    constexpr int NT = 2;
    __shared__ __attribute__((aligned(16))) WideRed red[2];
    const int end = min(static_cast<int>(blockIdx.x) * MT + MT, max_tiles);
    const int n0 = blockIdx.y * (16 * NT);                  // (I % 32 == 0: no column tail)
    const int i16 = threadIdx.x & 15;
    int s = blockIdx.x * MT, e = -1, run = 0;
    while (wide_next_run(tile_experts, s, end, E, e, run)) {
        int64_t a_row[MT];
        bool a_on[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            int pair = m < run ? tile_rows[(s + m) * 16 + i16] : -1;
            if (pair >= P) pair = -1;
            a_on[m] = pair >= 0;
            a_row[m] = (a_on[m] ? pair / top_k : 0) * x_row_stride;
        }
        const int s0 = s;
        moe_wide_gemm<T, MT, NT, 2>(
            red, x, a_row, a_on, w + (static_cast<int64_t>(e) * 2 * I + n0) * H, static_cast<int64_t>(I) * H, H, run,
            [&](int m, const float(*buf)[kMoeWaves][16][16]) {
                // 16 rows x 32 columns: one element a thread
                const int n = threadIdx.x >> 8, rr = (threadIdx.x >> 4) & 15, cc = threadIdx.x & 15;
                const float su = wide_block_sum(buf[2 * n], rr, cc);
                const float sg = wide_block_sum(buf[2 * n + 1], rr, cc);
                const int orow = tile_rows[(s0 + m) * 16 + rr];
                if (orow < 0 || orow >= P) return;
                const T up = to_t<T>(su);
                const float g = to_f(to_t<T>(sg));
                const T silu = to_t<T>(g / (1.0f + expf(-g)));
                act[static_cast<int64_t>(orow) * I + n0 + 16 * n + cc] = mul_t<T>(up, silu);
            });
        s += run;
    }
}

template <typename T, int MT>
__global__ __launch_bounds__(kWideThreads) void moe_down_wide_kernel(float *__restrict__ y, const T *__restrict__ act,
                                                                      const T *__restrict__ w,
                                                                      const int32_t *__restrict__ tile_rows,
                                                                      const int32_t *__restrict__ tile_experts,
                                                                      int max_tiles, int P, int H, int I, int E) {
    constexpr int NT = 4;
    __shared__ __attribute__((aligned(16))) WideRed red[2];
    const int end = min(static_cast<int>(blockIdx.x) * MT + MT, max_tiles);
    const int n0 = blockIdx.y * (16 * NT);                  // (H % 64 == 0: no column tail)
    const int i16 = threadIdx.x & 15;
    int s = blockIdx.x * MT, e = -1, run = 0;
    while (wide_next_run(tile_experts, s, end, E, e, run)) {
        int64_t a_row[MT];
        bool a_on[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            int pair = m < run ? tile_rows[(s + m) * 16 + i16] : -1;
            if (pair >= P) pair = -1;
            a_on[m] = pair >= 0;
            a_row[m] = (a_on[m] ? pair : 0) * static_cast<int64_t>(I);
        }
        const int s0 = s;
        moe_wide_gemm<T, MT, NT, 1>(red, act, a_row, a_on, w + (static_cast<int64_t>(e) * H + n0) * I, 0, I, run,
                                    [&](int m, const float(*buf)[kMoeWaves][16][16]) {
                                        // 16 rows x 64 columns: two elements a thread
                                        const int rr = (threadIdx.x >> 4) & 15, cc = threadIdx.x & 15;
                                        const int orow = tile_rows[(s0 + m) * 16 + rr];
#pragma unroll
                                        for (int n = threadIdx.x >> 8; n < NT; n += 2) {
                                            const float sum = wide_block_sum(buf[n], rr, cc);
                                            if (orow >= 0 && orow < P)
                                                y[static_cast<int64_t>(orow) * H + n0 + 16 * n + cc] = sum;
                                        }
                                    });
        s += run;
    }
}

} // namespace swl

extern "C" int swl_moe_wide_row_tiles(int32_t num_tokens, int32_t top_k, int32_t num_experts, int32_t hidden,
                                      int32_t inter) {
    // Host arithmetic, a function of its arguments only (capture and replay agree). 0: take the 16-row form.
    if (swl::moe_step_check(num_tokens, top_k, num_experts) != SWL_OK || hidden <= 0 || inter <= 0) return 0;
    if (num_tokens <= 32) return 0;                         // decode launches exactly what it launched
    const int rows_per_expert = num_tokens * top_k / num_experts;
    if (rows_per_expert < 32) return 0;                     // fewer than two tiles an expert on average: no reuse to have
    // Measured (profiles/moe_wide_micro.json): experts as wide as Mixtral's gain most from 4 tiles from 32 rows an expert on;
    // experts as small as Qwen3-30B-A3B's (at most 32 rows in a 4096-pair call, the only region measured) are as fast or
    // faster with 2, so smaller experts take 2 everywhere.
    return static_cast<int64_t>(hidden) * inter >= (int64_t{1} << 24) ? 4 : 2;
}

extern "C" int swl_moe_up_gate_silu_wide(void *act, const void *x, const void *expert_up_gate, const int32_t *tile_rows,
                                         const int32_t *tile_experts, int32_t max_tiles, int32_t num_tokens, int32_t top_k,
                                         int32_t hidden, int32_t inter, int32_t num_experts, int64_t x_row_stride,
                                         int32_t row_tiles, int32_t dtype, swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0 || x_row_stride < hidden || row_tiles <= 0) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_supported(hidden, inter, num_experts, top_k, dtype) || x_row_stride % 8 != 0) return SWL_ERR_UNSUPPORTED;
    if (!swl::moe_wide_tiles_ok(row_tiles)) return SWL_ERR_UNSUPPORTED;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!act || !x || !expert_up_gate || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(x) || !swl::aligned16(expert_up_gate)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>((max_tiles + row_tiles - 1) / row_tiles), static_cast<unsigned>(inter / 32));
#define SWL_MOE_WIDE(MT)                                                                                                    \
    SWL_DISPATCH_DTYPE(dtype, T, {                                                                                          \
        hipLaunchKernelGGL((swl::moe_up_gate_silu_wide_kernel<T, MT>), grid, dim3(swl::kWideThreads), 0,                    \
                           static_cast<hipStream_t>(stream), static_cast<T *>(act), static_cast<const T *>(x),              \
                           static_cast<const T *>(expert_up_gate), tile_rows, tile_experts, max_tiles, num_tokens * top_k,  \
                           top_k, hidden, inter, num_experts, x_row_stride);                                                \
    })
    if (row_tiles == 2) SWL_MOE_WIDE(2);
    else SWL_MOE_WIDE(4);
#undef SWL_MOE_WIDE
    return swl::check_launch();
}

extern "C" int swl_moe_down_wide(float *y, const void *act, const void *expert_down, const int32_t *tile_rows,
                                 const int32_t *tile_experts, int32_t max_tiles, int32_t num_tokens, int32_t top_k,
                                 int32_t hidden, int32_t inter, int32_t num_experts, int32_t row_tiles, int32_t dtype,
                                 swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0 || row_tiles <= 0) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_supported(hidden, inter, num_experts, top_k, dtype)) return SWL_ERR_UNSUPPORTED;
    if (!swl::moe_wide_tiles_ok(row_tiles)) return SWL_ERR_UNSUPPORTED;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!y || !act || !expert_down || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(act) || !swl::aligned16(expert_down)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>((max_tiles + row_tiles - 1) / row_tiles), static_cast<unsigned>(hidden / 64));
#define SWL_MOE_WIDE(MT)                                                                                                    \
    SWL_DISPATCH_DTYPE(dtype, T, {                                                                                          \
        hipLaunchKernelGGL((swl::moe_down_wide_kernel<T, MT>), grid, dim3(swl::kWideThreads), 0,                            \
                           static_cast<hipStream_t>(stream), y, static_cast<const T *>(act),                                \
                           static_cast<const T *>(expert_down), tile_rows, tile_experts, max_tiles, num_tokens * top_k,     \
                           hidden, inter, num_experts);                                                                     \
    })
    if (row_tiles == 2) SWL_MOE_WIDE(2);
    else SWL_MOE_WIDE(4);
#undef SWL_MOE_WIDE
    return swl::check_launch();
}
