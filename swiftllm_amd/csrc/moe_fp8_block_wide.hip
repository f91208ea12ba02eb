// moe_fp8_block_wide.hip — the block-scaled FP8 expert GEMMs of moe_fp8_block.hip in the weight-reusing row-tile form of
// moe_wide.hip, for prompt-sized steps, gfx950. The contract and the chain: moe_fp8_block.h.
//
// A workgroup is (MT consecutive tile slots) x (NT * 16 output columns) x NB weight row blocks (2: up and gate, 1: down),
// 8 waves. Per 64-wide k step a wave holds MT A fragment pairs, NT * NB 16-byte code fragments and NB scales (its NT * 16
// columns start at a multiple of their width, so they lie inside ONE 128-row block: one scalar load per weight row block
// and step), dequantises each code fragment ONCE, builds MT * NT * NB partials of two v_mfma_f32_16x16x32 each from zero
// accumulators and folds each into its running sum with one fmaf by the step's scale.
//
// The bits are those of the 16-row kernels, on every row: moe_fp8_block.h's chain per element — wave w takes the steps w,
// w + 8, ... ascending, every step low half then high half from zero and folded once, the eight running sums added in wave
// order. More tiles or column blocks under one wave change no element's chain.
//
// Runs, slots, barriers and the epilogue's LDS passes are moe_fp8_wide.hip's (moe_wide.hip's): slots [g * MT, g * MT + MT)
// belong to workgroup column g, walked as maximal stretches of ONE expert; what decides the walk is read from tile_experts
// at workgroup-uniform addresses, so a workgroup whose slots are all unused leaves before any barrier and every barrier
// inside a sub-run is reached by all 512 threads. The step after the current one is in flight behind the current one's
// MFMAs (two register sets). Grid: (ceil(max_tiles / MT), columns / (16 NT)). MT is 2 (see moe_fp8_block_wide_tiles_ok).
#include "moe_fp8_block.h"

namespace swl {

constexpr int kFp8BlockWideThreads = 64 * kMoeWaves;
constexpr int kFp8BlockWideBlocks = 4;    // NT * NB: 16 x 16 blocks per tile and pass (up/gate: 2 x 2, down: 4 x 1)

typedef float Fp8BlockWideRed[kFp8BlockWideBlocks][kMoeWaves][16][16];

// 2 only: with 4 tiles the 16 running sums and the partials next to two register sets of fragments need more than the 256
// registers a wave of a 512-thread workgroup has (the compiler spills to scratch), so that instantiation is not built
inline bool moe_fp8_block_wide_tiles_ok(int row_tiles) { return row_tiles == 2; }

// The first slot at or after `s` (below `end`) that holds a tile, its expert and the length of the stretch of that expert:
// all three workgroup-uniform. Returns false when no tile is left.
__device__ __forceinline__ bool fp8_block_wide_next_run(const int32_t *__restrict__ tile_experts, int &s, int end, int E,
                                                        int &e, int &run) {
    for (; s < end; ++s) {
        e = __builtin_amdgcn_readfirstlane(tile_experts[s]);
        if (e >= 0 && e < E) break;
    }
    if (s >= end) return false;
    run = 1;
    while (s + run < end && __builtin_amdgcn_readfirstlane(tile_experts[s + run]) == e) ++run;
    return true;
}

// rows(A)[MT x 16, K] x (dequantised(W[n0 .. n0 + 16 NT, K]) * s[k / 128])^T for NB weight row blocks `nb_stride` bytes
// apart that share the A rows; sc[b] is the scale row (KB floats) of row block b. a_row[m] / a_on[m]: this lane's row
// (i16 = lane & 15) of tile m. `emit(m, buf)` runs once per live tile m < run after a barrier, with the eight waves'
// running sums of block c = n * NB + b in buf[c]; it must not write LDS.
template <typename T, int MT, int NT, int NB, typename Emit>
__device__ __forceinline__ void moe_fp8_block_wide_gemm(Fp8BlockWideRed *red, const T *__restrict__ a,
                                                        const int64_t (&a_row)[MT], const bool (&a_on)[MT],
                                                        const uint8_t *__restrict__ w, int64_t nb_stride,
                                                        const fp8_bscale_ptr (&sc)[NB], int K, int run, Emit emit) {
    static_assert(NT * NB == kFp8BlockWideBlocks, "one tile per epilogue pass");
    constexpr int NW = NT * NB;
    const int lane = threadIdx.x & 63, wave = fp8_block_wave();
    const int i16 = lane & 15, q = lane >> 4;
    const T *ap = a + 16 * q;
    const uint8_t *wp = w + static_cast<int64_t>(i16) * K + 16 * q;
    float4_t acc[MT][NW];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int c = 0; c < NW; ++c) acc[m][c] = float4_t{0.f, 0.f, 0.f, 0.f};

    auto fetch = [&](Fp8AFrag<T>(&af)[MT], u32x4_t(&wf)[NW], float(&sf)[NB], int k) {
#pragma unroll
        for (int c = 0; c < NW; ++c)
            wf[c] = load16b_nt(wp + (c % NB) * nb_stride + static_cast<int64_t>((c / NB) * 16) * K + k);
#pragma unroll
        for (int b = 0; b < NB; ++b) sf[b] = sc[b][k / kFp8BlockSide];
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = fp8_load_a(ap + a_row[m] + k, a_on[m]);
    };
    auto multiply = [&](const Fp8AFrag<T>(&af)[MT], const u32x4_t(&wf)[NW], const float(&sf)[NB]) {
        float4_t p[MT][NW];
#pragma unroll
        for (int c = 0; c < NW; ++c) {
            vec8_t<T> wlo, whi;
            fp8x16_to_t<T>(wf[c], wlo, whi);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                p[m][c] = float4_t{0.f, 0.f, 0.f, 0.f};
                p[m][c] = mfma16x32(af[m].lo, wlo, p[m][c]);
                p[m][c] = mfma16x32(af[m].hi, whi, p[m][c]);
                mfma_results_tie(p[m][c]);
            }
        }
        mfma_results_ready<4>(p[MT - 1][NW - 1]);
#pragma unroll
        for (int c = 0; c < NW; ++c)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m][c] = fp8_block_fold(p[m][c], sf[c % NB], acc[m][c]);
    };
    // wave w: steps w, w + 8, ... ascending; the step after the current one is in flight behind its MFMAs
    const int k0 = kFp8KStep * wave;                        // (uniform)
    const int steps = K > k0 ? (K - k0 + kFp8Round - 1) / kFp8Round : 0;
    Fp8AFrag<T> a0[MT], a1[MT];
    u32x4_t w0[NW], w1[NW];
    float s0[NB], s1[NB];
    if (steps > 0) fetch(a0, w0, s0, k0);
    for (int s = 0; s < steps; s += 2) {
        const bool pair = s + 1 < steps;
        if (pair) fetch(a1, w1, s1, k0 + (s + 1) * kFp8Round);
        multiply(a0, w0, s0);
        if (pair) {
            if (s + 2 < steps) fetch(a0, w0, s0, k0 + (s + 2) * kFp8Round);
            multiply(a1, w1, s1);
        }
    }

    // acc[m][c][r] = running sum of (row 4q + r of tile m, column i16 of block c): VALU results. One tile per pass,
    // alternating buffers: a buffer is written again two passes later, behind the barrier all readers of its last use
    // have passed.
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
__global__ __launch_bounds__(kFp8BlockWideThreads) void moe_up_gate_silu_fp8_block_wide_kernel(
    T *__restrict__ act, const T *__restrict__ x, const uint8_t *__restrict__ w, const float *__restrict__ bscale,
    const int32_t *__restrict__ tile_rows, const int32_t *__restrict__ tile_experts, int max_tiles, int P, int top_k, int H,
    int I, int E, int64_t x_row_stride) {
    constexpr int NT = 2;
    __shared__ __attribute__((aligned(16))) Fp8BlockWideRed red[2];
    const int end = min(static_cast<int>(blockIdx.x) * MT + MT, max_tiles);
    const int n0 = blockIdx.y * (16 * NT);                  // (I % 64 == 0: no column tail; 32 columns: one row block)
    const int i16 = threadIdx.x & 15;
    const int rb = moe_fp8_blocks(I), kb = moe_fp8_blocks(H);
    int s = blockIdx.x * MT, e = -1, run = 0;
    while (fp8_block_wide_next_run(tile_experts, s, end, E, e, run)) {
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
        const int64_t up_row = static_cast<int64_t>(e) * 2 * I + n0;
        const float *s_up = bscale + (static_cast<int64_t>(e) * 2 * rb + n0 / kFp8BlockSide) * kb;
        const fp8_bscale_ptr sc[2] = {fp8_bscale_row(s_up), fp8_bscale_row(s_up + static_cast<int64_t>(rb) * kb)};
        moe_fp8_block_wide_gemm<T, MT, NT, 2>(
            red, x, a_row, a_on, w + up_row * H, static_cast<int64_t>(I) * H, sc, H, run,
            [&](int m, const float(*buf)[kMoeWaves][16][16]) {
                // 16 rows x 32 columns: one element a thread
                const int n = threadIdx.x >> 8, rr = (threadIdx.x >> 4) & 15, cc = threadIdx.x & 15;
                const float su = fp8_wave_sum(buf[2 * n], rr, cc);
                const float sg = fp8_wave_sum(buf[2 * n + 1], rr, cc);
                const int orow = tile_rows[(s0 + m) * 16 + rr];
                if (orow < 0 || orow >= P) return;
                act[static_cast<int64_t>(orow) * I + n0 + 16 * n + cc] = fp8_block_up_gate_act<T>(su, sg);
            });
        s += run;
    }
}

template <typename T, int MT>
__global__ __launch_bounds__(kFp8BlockWideThreads) void moe_down_fp8_block_wide_kernel(
    float *__restrict__ y, const T *__restrict__ act, const uint8_t *__restrict__ w, const float *__restrict__ bscale,
    const int32_t *__restrict__ tile_rows, const int32_t *__restrict__ tile_experts, int max_tiles, int P, int H, int I,
    int E) {
    constexpr int NT = 4;
    __shared__ __attribute__((aligned(16))) Fp8BlockWideRed red[2];
    const int end = min(static_cast<int>(blockIdx.x) * MT + MT, max_tiles);
    const int n0 = blockIdx.y * (16 * NT);                  // (H % 64 == 0: no column tail; 64 columns: one row block)
    const int i16 = threadIdx.x & 15;
    const int rb = moe_fp8_blocks(H), kb = moe_fp8_blocks(I);
    int s = blockIdx.x * MT, e = -1, run = 0;
    while (fp8_block_wide_next_run(tile_experts, s, end, E, e, run)) {
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
        const int64_t w_row = static_cast<int64_t>(e) * H + n0;
        const fp8_bscale_ptr sc[1] = {fp8_bscale_row(bscale + (static_cast<int64_t>(e) * rb + n0 / kFp8BlockSide) * kb)};
        moe_fp8_block_wide_gemm<T, MT, NT, 1>(red, act, a_row, a_on, w + w_row * I, 0, sc, I, run,
                                              [&](int m, const float(*buf)[kMoeWaves][16][16]) {
                                                  // 16 rows x 64 columns: two elements a thread
                                                  const int rr = (threadIdx.x >> 4) & 15, cc = threadIdx.x & 15;
                                                  const int orow = tile_rows[(s0 + m) * 16 + rr];
#pragma unroll
                                                  for (int n = threadIdx.x >> 8; n < NT; n += 2) {
                                                      const float sum = fp8_wave_sum(buf[n], rr, cc);
                                                      if (orow >= 0 && orow < P)
                                                          y[static_cast<int64_t>(orow) * H + n0 + 16 * n + cc] = sum;
                                                  }
                                              });
        s += run;
    }
}

} // namespace swl

extern "C" int swl_moe_up_gate_silu_fp8_block_wide(void *act, const void *x, const void *expert_up_gate,
                                                   const float *up_gate_bscale, int32_t row_blocks, int32_t k_blocks,
                                                   const int32_t *tile_rows, const int32_t *tile_experts, int32_t max_tiles,
                                                   int32_t num_tokens, int32_t top_k, int32_t hidden, int32_t inter,
                                                   int32_t num_experts, int64_t x_row_stride, int32_t row_tiles,
                                                   int32_t dtype, swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0 || x_row_stride < hidden || row_tiles <= 0) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_fp8_block_supported(hidden, inter, num_experts, top_k, dtype) || x_row_stride % 8 != 0)
        return SWL_ERR_UNSUPPORTED;
    if (!swl::moe_fp8_block_wide_tiles_ok(row_tiles)) return SWL_ERR_UNSUPPORTED;
    if (row_blocks != swl::moe_fp8_blocks(inter) || k_blocks != swl::moe_fp8_blocks(hidden)) return SWL_ERR_BAD_ARG;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!act || !x || !expert_up_gate || !up_gate_bscale || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(x) || !swl::aligned16(expert_up_gate)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>((max_tiles + row_tiles - 1) / row_tiles), static_cast<unsigned>(inter / 32));
#define SWL_MOE_FP8_BLOCK_WIDE(MT)                                                                                          \
    SWL_DISPATCH_DTYPE(dtype, T, {                                                                                          \
        hipLaunchKernelGGL((swl::moe_up_gate_silu_fp8_block_wide_kernel<T, MT>), grid, dim3(swl::kFp8BlockWideThreads), 0,  \
                           static_cast<hipStream_t>(stream), static_cast<T *>(act), static_cast<const T *>(x),              \
                           static_cast<const uint8_t *>(expert_up_gate), up_gate_bscale, tile_rows, tile_experts,           \
                           max_tiles, num_tokens * top_k, top_k, hidden, inter, num_experts, x_row_stride);                 \
    })
    SWL_MOE_FP8_BLOCK_WIDE(2);
#undef SWL_MOE_FP8_BLOCK_WIDE
    return swl::check_launch();
}

extern "C" int swl_moe_down_fp8_block_wide(float *y, const void *act, const void *expert_down, const float *down_bscale,
                                           int32_t row_blocks, int32_t k_blocks, const int32_t *tile_rows,
                                           const int32_t *tile_experts, int32_t max_tiles, int32_t num_tokens,
                                           int32_t top_k, int32_t hidden, int32_t inter, int32_t num_experts,
                                           int32_t row_tiles, int32_t dtype, swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0 || row_tiles <= 0) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_fp8_block_supported(hidden, inter, num_experts, top_k, dtype)) return SWL_ERR_UNSUPPORTED;
    if (!swl::moe_fp8_block_wide_tiles_ok(row_tiles)) return SWL_ERR_UNSUPPORTED;
    if (row_blocks != swl::moe_fp8_blocks(hidden) || k_blocks != swl::moe_fp8_blocks(inter)) return SWL_ERR_BAD_ARG;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!y || !act || !expert_down || !down_bscale || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(act) || !swl::aligned16(expert_down)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>((max_tiles + row_tiles - 1) / row_tiles), static_cast<unsigned>(hidden / 64));
#define SWL_MOE_FP8_BLOCK_WIDE(MT)                                                                                          \
    SWL_DISPATCH_DTYPE(dtype, T, {                                                                                          \
        hipLaunchKernelGGL((swl::moe_down_fp8_block_wide_kernel<T, MT>), grid, dim3(swl::kFp8BlockWideThreads), 0,          \
                           static_cast<hipStream_t>(stream), y, static_cast<const T *>(act),                                \
                           static_cast<const uint8_t *>(expert_down), down_bscale, tile_rows, tile_experts, max_tiles,      \
                           num_tokens * top_k, hidden, inter, num_experts);                                                 \
    })
    SWL_MOE_FP8_BLOCK_WIDE(2);
#undef SWL_MOE_FP8_BLOCK_WIDE
    return swl::check_launch();
}
