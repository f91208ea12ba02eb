// gemm_fp8_block_wide.hip — dense projections on block-scaled FP8 (e4m3) weights for steps of 65..256 tokens (the entries take
// 1..256), gfx950. The storage contract and the chain of one output element are gemm_fp8_block.h's, unchanged: with the
// same k_splits a row's bits are the ones gemm_fp8_block.hip writes. DESIGN.md section 4.22.
//
//   swl_gemm_fp8_block_wide            y[M, N] = x[M, K] . W^T
//   swl_gemm_fp8_block_wide_silu_gate  act[M, I] = up *_T silu(gate) over [up ; gate] codes
//   swl_gemm_fp8_block_wide_choose_splits: host arithmetic
//
// The work split. A workgroup is 4 waves, ONE per CU (139 KiB of LDS at 256 rows; a wave has the 512-register file), and
// owns FOUR 16-row weight tiles over one k slice for ALL token tiles: 64 output columns of y, or 32 columns of act (two up
// tiles and the two gate tiles I rows below them — half the columns, not twice the registers). The 4 x 4 TW grid of
// (weight tile, token tile) is cut along the TOKENS: every wave takes all four weight tiles and the TW token tiles
// [wave TW, wave TW + TW), TW = ceil(ceil(M / 16) / 4) = 1..4 by instantiation. A wave so holds 4 x TW running sums and as
// many partials (128 registers at TW = 4), and every fragment it fetches feeds several MFMAs: an A fragment (2 KiB of LDS
// a wave) the four weight tiles (8 MFMAs), a dequantised code pair the TW token tiles (2 TW MFMAs). The price is that every
// wave dequantises every code of the workgroup (4 x the conversions of the other cut, two weight tiles x 2 TW token
// tiles a wave pair); that cut reads twice the x bytes from LDS per MFMA, and the LDS port is what the 16-bit kernel of
// this range (gemm_wide.hip) found itself held by.
//   x        global -> registers -> LDS as full lines, one barrier a chunk, two LDS buffers, as in the 64-row kernel, but
//            asked for TWO chunks ahead through two register sets, so the wait before the LDS write is not a whole
//            memory latency a chunk; a chunk is ONE k block (128 k, two steps) so that two buffers of 256 rows fit: rows 272 bytes apart
//            (17 x 16: the sixteen rows of an A-fragment read fall into sixteen distinct 16-byte bank groups), 2 x 68 KiB.
//   codes    16 bytes a lane, 1 KiB per wave, tile and step, non-temporal, through a ring of EIGHT steps x four tiles in
//            registers (32 KiB a wave in flight; at TW = 4 FOUR steps, 16 KiB, the registers going to the second x set
//            below; a slot is asked for again, a ring ahead, once its codes are dequantised).
//            The four waves ask for the same lines within one chunk of each other (the barrier), so the later asks are
//            expected to meet the line in L1 / L2 and HBM to be read once per code byte and workgroup: NOT measured (no
//            counter run; cached instead of non-temporal loads timed 5 - 12 % faster, so the re-asks may not be free).
//   scales   one scalar load per weight tile and k block.
#include "gemm_fp8_block.h"

namespace swl {

constexpr int kWideMaxM = 256;
constexpr int kWideChunk = kFp8BlockSide;                   // k of x one LDS buffer holds: one k block, two steps
constexpr int kWidePitch = kWideChunk + 8;                  // elements between x rows in LDS: 272 bytes
constexpr int kWideTiles = 4;                               // weight tiles of a workgroup — every wave's
constexpr int kWideThreads = 64 * kGemmFp8Waves;

// TW token tiles a wave (4 TW a workgroup). SILU: weight tiles 0, 1 are up, 2, 3 the gate tiles `nb_stride` rows below them.
template <typename T, int TW, bool SILU>
__global__ __launch_bounds__(kWideThreads, 1) void gemm_fp8_block_wide_kernel(T *__restrict__ out, float *__restrict__ slabs,
                                                                              const T *__restrict__ x,
                                                                              const uint8_t *__restrict__ w,
                                                                              const float *__restrict__ bscale, Fp8Segments seg,
                                                                              int M, int n_out, int K, int nb_stride,
                                                                              int64_t x_row_stride) {
    constexpr int kRows = 16 * TW * kGemmFp8Waves;
    __shared__ __attribute__((aligned(16))) T xs[2][kRows][kWidePitch];
    const int lane = threadIdx.x & 63, wave = fp8_block_wave();
    const int i16 = lane & 15, q = lane >> 4;
    const int kb = moe_fp8_blocks(K), ks = gridDim.y, split = blockIdx.y;
    const int k_begin = fp8_split_first_block(split, ks, kb) * kFp8BlockSide;
    const int k_end = min(fp8_split_first_block(split + 1, ks, kb) * kFp8BlockSide, K);
    const int nchunks = (k_end - k_begin + kWideChunk - 1) / kWideChunk;
    const int row0 = 16 * TW * wave;                        // this wave's first token row

    // ---- the four weight tiles: output column, weight row (uniform over the workgroup) ----
    int col[kWideTiles], wrow[kWideTiles];
    bool on[kWideTiles];                                    // a last workgroup's spare tiles walk tile 0 and store nothing
#pragma unroll
    for (int b = 0; b < kWideTiles; ++b) {
        col[b] = SILU ? (static_cast<int>(blockIdx.x) * 2 + (b & 1)) * 16 : (static_cast<int>(blockIdx.x) * kWideTiles + b) * 16;
        on[b] = col[b] < n_out;
        if (!on[b]) col[b] = 0;
        wrow[b] = col[b] + (SILU && b >= 2 ? nb_stride : 0);
    }

    // ---- x: this thread's 16-byte pieces of a chunk (4 TW of them), rows as full lines (16 lanes a row) ----
    constexpr int kXLoads = kRows * (kWideChunk / 8) / kWideThreads;
    vec8_t<T> xr[2][kXLoads];                               // two sets: chunk c + 2 is asked for while c + 1 still waits
    // Every load of the main loop is UNCONDITIONAL, its address clamped into the slice instead: a load under a branch makes
    // the compiler wait for the vector-memory counter to drain (it must assume the loads issued since were skipped), which
    // turns the rings below into one memory latency a chunk. What a clamped load fetches is never used: rows >= M feed
    // output rows that are not stored, k >= k_end belongs to a step or a chunk that is not computed.
    auto x_fetch = [&](auto set, int c) {
        constexpr int S = decltype(set)::value;
        const int kc = k_begin + c * kWideChunk;
#pragma unroll
        for (int p = 0; p < kXLoads; ++p) {
            const int flat = p * kWideThreads + threadIdx.x;
            xr[S][p] = load8(x + min(flat >> 4, M - 1) * x_row_stride + min(kc + 8 * (flat & 15), k_end - 8));
        }
    };
    auto x_put = [&](auto set, int buf) {
#pragma unroll
        for (int p = 0; p < kXLoads; ++p) {
            const int flat = p * kWideThreads + threadIdx.x;
            store8(&xs[buf][flat >> 4][8 * (flat & 15)], xr[decltype(set)::value][p]);
        }
    };

    // ---- codes: a ring of kRing chunks' steps in registers (TW = 4: the second x set takes two chunks' registers) ----
    constexpr int kRing = TW == 4 ? 2 : 4;
    const uint8_t *wp = w + static_cast<int64_t>(i16) * K + 16 * q;
    int64_t wo[kWideTiles];
    fp8_bscale_ptr sc[kWideTiles];
#pragma unroll
    for (int b = 0; b < kWideTiles; ++b) {
        wo[b] = static_cast<int64_t>(wrow[b]) * K;
        sc[b] = fp8_bscale_row(bscale + static_cast<int64_t>(fp8_segments_scale_row(seg, wrow[b])) * kb);
    }
    u32x4_t wr[kRing][2][kWideTiles];
    auto w_fetch = [&](auto par, auto u, int k) {           // the step at k into slot (par, u); past the slice: its last step
        k = min(k, k_end - kFp8KStep);
#pragma unroll
        for (int b = 0; b < kWideTiles; ++b) wr[par.value][u.value][b] = load16b_nt(wp + wo[b] + k);
    };

    float4_t run[kWideTiles][TW];
#pragma unroll
    for (int b = 0; b < kWideTiles; ++b)
#pragma unroll
        for (int t = 0; t < TW; ++t) run[b][t] = float4_t{0.f, 0.f, 0.f, 0.f};

    x_fetch(IntTag<0>{}, 0);
    x_fetch(IntTag<1>{}, 1);
    w_fetch(IntTag<0>{}, IntTag<0>{}, k_begin), w_fetch(IntTag<0>{}, IntTag<1>{}, k_begin + 64);
    w_fetch(IntTag<1>{}, IntTag<0>{}, k_begin + 128), w_fetch(IntTag<1>{}, IntTag<1>{}, k_begin + 192);
    if constexpr (kRing == 4) {
        w_fetch(IntTag<2>{}, IntTag<0>{}, k_begin + 256), w_fetch(IntTag<2>{}, IntTag<1>{}, k_begin + 320);
        w_fetch(IntTag<3>{}, IntTag<0>{}, k_begin + 384), w_fetch(IntTag<3>{}, IntTag<1>{}, k_begin + 448);
    }
    x_put(IntTag<0>{}, 0);
    __syncthreads();

    // One k block. Its x is in buffer c & 1 and came through register set c & 1, which is free again: chunk c + 2 is asked
    // for into it now and written to LDS at the END OF CHUNK c + 1, a whole chunk's arithmetic after the ask, so the wait
    // before that write (the vector-memory counter retires in order) leaves this chunk's code refills and the next x
    // in flight.
    auto chunk = [&](int c, auto unr) {
        constexpr int kBuf = decltype(unr)::value & 1;
        const IntTag<decltype(unr)::value % kRing> par;     // the ring slot of this chunk's codes
        const int kc = k_begin + c * kWideChunk;
        const bool more = c + 1 < nchunks;                  // (uniform over the workgroup)
        x_fetch(IntTag<kBuf>{}, c + 2);
        float s[kWideTiles];
#pragma unroll
        for (int b = 0; b < kWideTiles; ++b) s[b] = sc[b][kc / kFp8BlockSide];
        float4_t p[kWideTiles][TW];
#pragma unroll
        for (int b = 0; b < kWideTiles; ++b)
#pragma unroll
            for (int t = 0; t < TW; ++t) p[b][t] = float4_t{0.f, 0.f, 0.f, 0.f};
        auto step = [&](auto u) {
            constexpr int U = decltype(u)::value;
            if (U == 0 || kc + kFp8KStep < k_end) {         // (a slice's last k block may be half a block)
            const T *ax = &xs[kBuf][row0 + i16][U * kFp8KStep + 16 * q];
            Fp8AFrag<T> a[TW];
#pragma unroll
            for (int t = 0; t < TW; ++t) a[t].lo = load8(ax + t * 16 * kWidePitch), a[t].hi = load8(ax + t * 16 * kWidePitch + 8);
#pragma unroll
            for (int b = 0; b < kWideTiles; ++b) {
                vec8_t<T> wlo, whi;
                fp8x16_to_t<T>(wr[par.value][U][b], wlo, whi);
#pragma unroll
                for (int t = 0; t < TW; ++t) {
                    p[b][t] = mfma16x32(a[t].lo, wlo, p[b][t]);
                    p[b][t] = mfma16x32(a[t].hi, whi, p[b][t]);
                }
            }
            }
            w_fetch(par, u, kc + U * kFp8KStep + kRing * kWideChunk);               // the slot's next step, kRing chunks ahead
        };
        step(IntTag<0>{});
        step(IntTag<1>{});
#pragma unroll
        for (int b = 0; b < kWideTiles; ++b)
#pragma unroll
            for (int t = 0; t < TW; ++t) mfma_results_tie(p[b][t]);
        mfma_results_ready<4>(p[kWideTiles - 1][TW - 1]);
#pragma unroll
        for (int b = 0; b < kWideTiles; ++b)
#pragma unroll
            for (int t = 0; t < TW; ++t) run[b][t] = fp8_block_fold(p[b][t], s[b], run[b][t]);
        if (more) x_put(IntTag<(kBuf ^ 1)>{}, kBuf ^ 1);
        __syncthreads();                                    // chunk c + 1 is in place; chunk c's buffer is free for c + 2
    };
    for (int c = 0;;) {                                     // (leaving by `break`: only the full path reaches the back edge)
        chunk(c, IntTag<0>{});
        if (++c >= nchunks) break;
        chunk(c, IntTag<1>{});
        if (++c >= nchunks) break;
        chunk(c, IntTag<2>{});
        if (++c >= nchunks) break;
        chunk(c, IntTag<3>{});
        if (++c >= nchunks) break;
    }

    // run[b][t][r] = (row row0 + 16 t + 4 q + r, weight row wrow[b] + i16)
    const int n_w = SILU ? 2 * nb_stride : n_out;           // weight rows: the width of a slab
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 16 * t + 4 * q + r;
            if (row >= M) continue;
            if (ks > 1) {
                float *sl = slabs + (static_cast<int64_t>(split) * M + row) * n_w + i16;
#pragma unroll
                for (int b = 0; b < kWideTiles; ++b)
                    if (on[b]) sl[wrow[b]] = run[b][t][r];
            } else if constexpr (SILU) {
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    if (on[b]) out[static_cast<int64_t>(row) * n_out + col[b] + i16] = fp8_block_up_gate_act<T>(run[b][t][r], run[b + 2][t][r]);
            } else {
#pragma unroll
                for (int b = 0; b < kWideTiles; ++b)
                    if (on[b]) out[static_cast<int64_t>(row) * n_out + col[b] + i16] = to_t<T>(run[b][t][r]);
            }
        }
}

template <typename T, bool SILU>
void launch_fp8_gemm_wide(const GemmArgs &a, const float *bscale, const Fp8Segments &seg, int nb_stride, int ks, hipStream_t stream) {
    const int tiles = a.N / 16, per_wg = SILU ? 2 : kWideTiles;
    const dim3 grid((tiles + per_wg - 1) / per_wg, ks);
    T *out = static_cast<T *>(a.out);
    float *slabs = static_cast<float *>(a.workspace);
    auto go = [&](auto tw) {
        hipLaunchKernelGGL((gemm_fp8_block_wide_kernel<T, decltype(tw)::value, SILU>), grid, dim3(kWideThreads), 0, stream, out,
                           slabs, static_cast<const T *>(a.x), static_cast<const uint8_t *>(a.w), bscale, seg, a.M, a.N, a.K,
                           nb_stride, a.x_row_stride);
    };
    switch ((a.M + 63) / 64) {
    case 1: go(IntTag<1>{}); break;
    case 2: go(IntTag<2>{}); break;
    case 3: go(IntTag<3>{}); break;
    default: go(IntTag<4>{}); break;
    }
    if (ks > 1) {
        const int64_t threads = static_cast<int64_t>(a.M) * (a.N / 4);
        hipLaunchKernelGGL((gemm_fp8_block_finish_kernel<T, SILU>), dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256),
                           0, stream, out, slabs, ks, a.M, a.N, SILU ? 2 * a.N : a.N);
    }
}

} // namespace swl

// One workgroup a CU here, so a slice more is taken only while the grid still fits the card's 256 CUs (the 64-row chooser
// goes one doubling further): every slice writes and the finishing kernel reads 4 M bytes of slab per weight row, which at
// 256 tokens is the weight row's own K code bytes where K = 1024 — slab traffic grows with M, the codes do not. A slice
// keeps at least TWO k blocks (K = 2112: 8 slices of 2 or 3), so a short slice fills only part of the code ring. n: the weight rows of the launch, four tiles (64 rows) a workgroup in both forms.
extern "C" int swl_gemm_fp8_block_wide_choose_splits(int32_t n, int32_t k) {
    if (n <= 0 || n % 16 || !swl::gemm_fp8_geometry_ok(k)) return 0;
    const int wgs = (n / 16 + swl::kWideTiles - 1) / swl::kWideTiles, kb = swl::moe_fp8_blocks(k);
    int ks = 1;
    while (ks < swl::kGemmFp8MaxSplits && 2 * wgs * ks <= 256 && kb / (2 * ks) >= 2) ks *= 2;
    return ks;
}

extern "C" int swl_gemm_fp8_block_wide(void *y, const void *x, const void *codes, const float *bscale, void *workspace,
                                       int64_t workspace_bytes, int32_t num_tokens, int32_t seg0, int32_t seg1, int32_t seg2,
                                       int32_t k, int32_t scale_rows, int32_t k_blocks, int64_t x_row_stride, int32_t k_splits,
                                       int32_t dtype, swl_stream_t stream) {
    const swl::Fp8Segments seg{{seg0, seg1, seg2}};
    const int64_t n64 = static_cast<int64_t>(seg0) + seg1 + seg2;
    if (seg0 < 0 || seg1 < 0 || seg2 < 0 || n64 > INT32_MAX || workspace_bytes < 0 || !swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    const int n = static_cast<int>(n64);
    swl::GemmArgs a{y, x, codes, workspace, static_cast<size_t>(workspace_bytes), num_tokens, n, k, x_row_stride, n, k_splits,
                    swl::kWideMaxM, swl::kFp8KStep};
    int ks = 0, rc = SWL_OK;
    if (swl::fp8_gemm_settled(a, bscale, seg, n, scale_rows, k_blocks, swl_gemm_fp8_block_wide_choose_splits(n, k), ks, rc)) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, { swl::launch_fp8_gemm_wide<T, false>(a, bscale, seg, 0, ks, static_cast<hipStream_t>(stream)); });
    return swl::check_launch();
}

extern "C" int swl_gemm_fp8_block_wide_silu_gate(void *act, const void *x, const void *codes, const float *bscale,
                                                 void *workspace, int64_t workspace_bytes, int32_t num_tokens, int32_t inter,
                                                 int32_t k, int32_t scale_rows, int32_t k_blocks, int64_t x_row_stride,
                                                 int32_t k_splits, int32_t dtype, swl_stream_t stream) {
    if (inter < 0 || inter > INT32_MAX / 2 || workspace_bytes < 0 || !swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    const swl::Fp8Segments seg{{inter, inter, 0}};
    swl::GemmArgs a{act, x, codes, workspace, static_cast<size_t>(workspace_bytes), num_tokens, inter, k, x_row_stride, inter,
                    k_splits, swl::kWideMaxM, swl::kFp8KStep};
    int ks = 0, rc = SWL_OK;
    if (swl::fp8_gemm_settled(a, bscale, seg, 2 * inter, scale_rows, k_blocks, swl_gemm_fp8_block_wide_choose_splits(2 * inter, k), ks, rc)) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, { swl::launch_fp8_gemm_wide<T, true>(a, bscale, seg, inter, ks, static_cast<hipStream_t>(stream)); });
    return swl::check_launch();
}
