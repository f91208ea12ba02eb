// gemm_fp8_block.hip — dense projections on block-scaled FP8 (e4m3, one fp32 scale per 128 x 128 block) weights, gfx950. The
// storage contract, the work split and the chain of one output element: gemm_fp8_block.h.
//
//   swl_gemm_fp8_block            y[M, N] = x[M, K] . W^T for 1 <= M <= 64 tokens: the weight-streaming kernel
//   swl_gemm_fp8_block_silu_gate  act[M, I] = up *_T silu(gate) over [up ; gate] codes: the same walk, two tiles a wave
//   swl_fp8_block_dequant         out[N, K] = T(fp32(code) *_fp32 scale): the 16-bit image hipBLASLt multiplies for steps of more
//                                 than 64 tokens
//   swl_gemm_fp8_block_supported, swl_gemm_fp8_block_choose_splits: host arithmetic
//
// With k_splits > 1 the streaming kernel writes fp32 slabs [k_splits][M][weight rows] into the caller's workspace and
// gemm_fp8_block_finish_kernel, launched behind it on the same stream, adds them in slice order and runs the epilogue.
#include "gemm_fp8_block.h"

namespace swl {

constexpr int kXPitch = kGemmFp8Chunk + 8;                  // elements between x rows in LDS: 528 bytes (gemm_fp8_block.h)
constexpr int kChunkSteps = kGemmFp8Chunk / kFp8KStep;      // 4
constexpr int kThreads = 64 * kGemmFp8Waves;

// MT token tiles, NB weight tiles a wave (1: y; 2: up and gate of the SiLU-gate form, `nb_stride` weight rows apart).
template <typename T, int MT, int NB>
__global__ __launch_bounds__(kThreads) void gemm_fp8_block_kernel(T *__restrict__ out, float *__restrict__ slabs,
                                                                  const T *__restrict__ x, const uint8_t *__restrict__ w,
                                                                  const float *__restrict__ bscale, Fp8Segments seg, int M,
                                                                  int n_out, int K, int nb_stride, int64_t x_row_stride) {
    __shared__ __attribute__((aligned(16))) T xs[2][MT * 16][kXPitch];
    const int lane = threadIdx.x & 63, wave = fp8_block_wave();
    const int i16 = lane & 15, q = lane >> 4;
    const int kb = moe_fp8_blocks(K), ks = gridDim.y, split = blockIdx.y;
    const int k_begin = fp8_split_first_block(split, ks, kb) * kFp8BlockSide;
    const int k_end = min(fp8_split_first_block(split + 1, ks, kb) * kFp8BlockSide, K);
    const int nchunks = (k_end - k_begin + kGemmFp8Chunk - 1) / kGemmFp8Chunk;
    const int n0 = (static_cast<int>(blockIdx.x) * kGemmFp8Waves + wave) * 16;      // (uniform per wave)
    const bool active = n0 < n_out;                         // a last workgroup's spare waves only help to stage x

    // ---- x: this thread's 16-byte pieces of a chunk (2 MT of them), rows as full lines ----
    constexpr int kXLoads = MT * 16 * (kGemmFp8Chunk / 8) / kThreads;               // 2 MT
    vec8_t<T> xr[kXLoads];
    auto x_fetch = [&](int c) {
        const int kc = k_begin + c * kGemmFp8Chunk;
#pragma unroll
        for (int p = 0; p < kXLoads; ++p) {
            const int flat = p * kThreads + threadIdx.x, row = flat >> 5, k = kc + 8 * (flat & 31);
            if (row < M && k < k_end) {
                xr[p] = load8(x + row * x_row_stride + k);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) xr[p][j] = to_t<T>(0.f);
            }
        }
    };
    auto x_put = [&](int buf) {
#pragma unroll
        for (int p = 0; p < kXLoads; ++p) {
            const int flat = p * kThreads + threadIdx.x;
            store8(&xs[buf][flat >> 5][8 * (flat & 31)], xr[p]);
        }
    };

    // ---- codes: a ring of two chunks' steps in registers ----
    const uint8_t *wp = w + static_cast<int64_t>(active ? n0 + i16 : 0) * K + 16 * q;
    const int64_t wb = static_cast<int64_t>(nb_stride) * K;
    u32x4_t wr[2][kChunkSteps][NB];
    auto w_fetch = [&](auto par, auto u, int k) {           // the step at k into slot (par, u); past the slice: nothing
        if (active && k < k_end) {
#pragma unroll
            for (int b = 0; b < NB; ++b) wr[par.value][u.value][b] = load16b_nt(wp + b * wb + k);
        }
    };
    fp8_bscale_ptr sc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
        sc[b] = fp8_bscale_row(bscale + static_cast<int64_t>(fp8_segments_scale_row(seg, (active ? n0 : 0) + b * nb_stride)) * kb);

    float4_t run[NB][MT];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int t = 0; t < MT; ++t) run[b][t] = float4_t{0.f, 0.f, 0.f, 0.f};

    x_fetch(0);
    w_fetch(IntTag<0>{}, IntTag<0>{}, k_begin), w_fetch(IntTag<0>{}, IntTag<1>{}, k_begin + 64);
    w_fetch(IntTag<0>{}, IntTag<2>{}, k_begin + 128), w_fetch(IntTag<0>{}, IntTag<3>{}, k_begin + 192);
    w_fetch(IntTag<1>{}, IntTag<0>{}, k_begin + 256), w_fetch(IntTag<1>{}, IntTag<1>{}, k_begin + 320);
    w_fetch(IntTag<1>{}, IntTag<2>{}, k_begin + 384), w_fetch(IntTag<1>{}, IntTag<3>{}, k_begin + 448);
    x_put(0);
    __syncthreads();

    auto chunk = [&](int c, auto par) {
        const int kc = k_begin + c * kGemmFp8Chunk;
        const bool more = c + 1 < nchunks;                  // (uniform over the workgroup)
        if (more) x_fetch(c + 1);
        if (active) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {                   // the chunk's two k blocks
                const int kk = kc + h * kFp8BlockSide;
                if (kk >= k_end) break;
                float s[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) s[b] = sc[b][kk / kFp8BlockSide];
                float4_t p[NB][MT];
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int t = 0; t < MT; ++t) p[b][t] = float4_t{0.f, 0.f, 0.f, 0.f};
                auto step = [&](auto u) {
                    constexpr int U = decltype(u)::value;
                    const T *ax = &xs[par.value][i16][U * kFp8KStep + 16 * q];
                    Fp8AFrag<T> a[MT];
#pragma unroll
                    for (int t = 0; t < MT; ++t) a[t].lo = load8(ax + t * 16 * kXPitch), a[t].hi = load8(ax + t * 16 * kXPitch + 8);
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        vec8_t<T> wlo, whi;
                        fp8x16_to_t<T>(wr[par.value][U][b], wlo, whi);
#pragma unroll
                        for (int t = 0; t < MT; ++t) {
                            p[b][t] = mfma16x32(a[t].lo, wlo, p[b][t]);
                            p[b][t] = mfma16x32(a[t].hi, whi, p[b][t]);
                        }
                    }
                    w_fetch(par, u, kc + U * kFp8KStep + 2 * kGemmFp8Chunk);        // the slot's next step, 512 k ahead
                };
                if (h == 0) {
                    step(IntTag<0>{});
                    if (kk + kFp8KStep < k_end) step(IntTag<1>{});
                } else {
                    step(IntTag<2>{});
                    if (kk + kFp8KStep < k_end) step(IntTag<3>{});
                }
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int t = 0; t < MT; ++t) mfma_results_tie(p[b][t]);
                mfma_results_ready<4>(p[NB - 1][MT - 1]);
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int t = 0; t < MT; ++t) run[b][t] = fp8_block_fold(p[b][t], s[b], run[b][t]);
            }
        }
        if (more) x_put(par.value ^ 1);
        __syncthreads();                                    // chunk c + 1 is in place; chunk c's buffer is free for c + 2
    };
    for (int c = 0; c < nchunks; c += 2) {
        chunk(c, IntTag<0>{});
        if (c + 1 < nchunks) chunk(c + 1, IntTag<1>{});
    }
    if (!active) return;

    // run[b][t][r] = (row 16 t + 4 q + r, column n0 + i16) of weight tile b
    const int n_w = NB * nb_stride + (NB == 1 ? n_out : 0);     // weight rows: the width of a slab
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + 4 * q + r;
            if (row >= M) continue;
            if (ks > 1) {
                float *sl = slabs + (static_cast<int64_t>(split) * M + row) * n_w + n0 + i16;
#pragma unroll
                for (int b = 0; b < NB; ++b) sl[b * nb_stride] = run[b][t][r];
            } else if constexpr (NB == 2) {
                out[static_cast<int64_t>(row) * n_out + n0 + i16] = fp8_block_up_gate_act<T>(run[0][t][r], run[1][t][r]);
            } else {
                out[static_cast<int64_t>(row) * n_out + n0 + i16] = to_t<T>(run[0][t][r]);
            }
        }
}

// out[N, K] = T(fp32(code) *_fp32 scale): 8 codes a lane, so a wave's store instruction writes 1 KiB of one row's
// contiguous bytes (K % 64 == 0: a wave never straddles rows unevenly, a lane never straddles a k block).
template <typename T>
__global__ __launch_bounds__(256) void fp8_block_dequant_kernel(T *__restrict__ out, const uint8_t *__restrict__ w,
                                                                const float *__restrict__ bscale, Fp8Segments seg, int N, int K) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;      // 8-element group
    const int per_row = K / 8;
    if (i >= static_cast<int64_t>(N) * per_row) return;
    const int row = static_cast<int>(i / per_row), k = 8 * static_cast<int>(i % per_row);
    const float s = bscale[static_cast<int64_t>(fp8_segments_scale_row(seg, row)) * moe_fp8_blocks(K) + k / kFp8BlockSide];
    const uint2 raw = *reinterpret_cast<const uint2 *>(w + static_cast<int64_t>(row) * K + k);
    const vec2_t<T> c[4] = {fp8x2_to_t<T, false>(raw.x), fp8x2_to_t<T, true>(raw.x), fp8x2_to_t<T, false>(raw.y),
                            fp8x2_to_t<T, true>(raw.y)};
    vec8_t<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = to_t<T>(__fmul_rn(to_f(c[j / 2][j % 2]), s));
    store8(out + static_cast<int64_t>(row) * K + k, o);
}

// ---- host ----
template <typename T, int NB>
void launch_fp8_gemm(const GemmArgs &a, const float *bscale, const Fp8Segments &seg, int nb_stride, int ks, hipStream_t stream) {
    const dim3 grid((a.N / 16 + kGemmFp8Waves - 1) / kGemmFp8Waves, ks);
    T *out = static_cast<T *>(a.out);
    float *slabs = static_cast<float *>(a.workspace);
    auto go = [&](auto mt) {
        hipLaunchKernelGGL((gemm_fp8_block_kernel<T, decltype(mt)::value, NB>), grid, dim3(kThreads), 0, stream, out, slabs,
                           static_cast<const T *>(a.x), static_cast<const uint8_t *>(a.w), bscale, seg, a.M, a.N, a.K,
                           nb_stride, a.x_row_stride);
    };
    switch ((a.M + 15) / 16) {
    case 1: go(IntTag<1>{}); break;
    case 2: go(IntTag<2>{}); break;
    case 3: go(IntTag<3>{}); break;
    default: go(IntTag<4>{}); break;
    }
    if (ks > 1) {
        const int64_t threads = static_cast<int64_t>(a.M) * (a.N / 4);
        hipLaunchKernelGGL((gemm_fp8_block_finish_kernel<T, NB == 2>), dim3(static_cast<unsigned>((threads + 255) / 256)),
                           dim3(256), 0, stream, out, slabs, ks, a.M, a.N, NB == 2 ? 2 * a.N : a.N);
    }
}

} // namespace swl

extern "C" int swl_gemm_fp8_block_supported(int32_t n, int32_t k, int32_t dtype) {
    return n > 0 && n % 16 == 0 && swl::gemm_fp8_geometry_ok(k) && swl::moe_dtype_ok(dtype);
}

// Enough workgroups for the card's 256 CUs while a slice keeps at least four k blocks (two chunks of the walk); at most 8
// slices: every slice writes 4 M bytes of slab per column beside its share of the column's K code bytes (at 64 tokens and 8
// slices that is 2 KiB, more than the codes where K <= 2048). 0: the shape is not taken.
extern "C" int swl_gemm_fp8_block_choose_splits(int32_t n, int32_t k) {
    if (n <= 0 || n % 16 || !swl::gemm_fp8_geometry_ok(k)) return 0;
    const int wgs = (n / 16 + swl::kGemmFp8Waves - 1) / swl::kGemmFp8Waves, kb = swl::moe_fp8_blocks(k);
    int ks = 1;
    while (ks < swl::kGemmFp8MaxSplits && wgs * ks < 256 && kb / (2 * ks) >= 2) ks *= 2;
    return ks;
}

extern "C" int swl_gemm_fp8_block(void *y, const void *x, const void *codes, const float *bscale, void *workspace,
                                  int64_t workspace_bytes, int32_t num_tokens, int32_t seg0, int32_t seg1, int32_t seg2,
                                  int32_t k, int32_t scale_rows, int32_t k_blocks, int64_t x_row_stride, int32_t k_splits,
                                  int32_t dtype, swl_stream_t stream) {
    const swl::Fp8Segments seg{{seg0, seg1, seg2}};
    const int64_t n64 = static_cast<int64_t>(seg0) + seg1 + seg2;
    if (seg0 < 0 || seg1 < 0 || seg2 < 0 || n64 > INT32_MAX || workspace_bytes < 0 || !swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    const int n = static_cast<int>(n64);
    swl::GemmArgs a{y, x, codes, workspace, static_cast<size_t>(workspace_bytes), num_tokens, n, k, x_row_stride, n, k_splits,
                    swl::kGemmFp8MaxM, swl::kFp8KStep};
    int ks = 0, rc = SWL_OK;
    if (swl::fp8_gemm_settled(a, bscale, seg, n, scale_rows, k_blocks, swl_gemm_fp8_block_choose_splits(n, k), ks, rc)) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, { swl::launch_fp8_gemm<T, 1>(a, bscale, seg, 0, ks, static_cast<hipStream_t>(stream)); });
    return swl::check_launch();
}

extern "C" int swl_gemm_fp8_block_silu_gate(void *act, const void *x, const void *codes, const float *bscale, void *workspace,
                                            int64_t workspace_bytes, int32_t num_tokens, int32_t inter, int32_t k,
                                            int32_t scale_rows, int32_t k_blocks, int64_t x_row_stride, int32_t k_splits,
                                            int32_t dtype, swl_stream_t stream) {
    if (inter < 0 || inter > INT32_MAX / 2 || workspace_bytes < 0 || !swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    const swl::Fp8Segments seg{{inter, inter, 0}};
    swl::GemmArgs a{act, x, codes, workspace, static_cast<size_t>(workspace_bytes), num_tokens, inter, k, x_row_stride, inter,
                    k_splits, swl::kGemmFp8MaxM, swl::kFp8KStep};
    int ks = 0, rc = SWL_OK;
    if (swl::fp8_gemm_settled(a, bscale, seg, 2 * inter, scale_rows, k_blocks, swl_gemm_fp8_block_choose_splits(inter, k), ks, rc)) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, { swl::launch_fp8_gemm<T, 2>(a, bscale, seg, inter, ks, static_cast<hipStream_t>(stream)); });
    return swl::check_launch();
}

extern "C" int swl_fp8_block_dequant(void *out, const void *codes, const float *bscale, int32_t seg0, int32_t seg1,
                                     int32_t seg2, int32_t k, int32_t scale_rows, int32_t k_blocks, int32_t dtype,
                                     swl_stream_t stream) {
    const swl::Fp8Segments seg{{seg0, seg1, seg2}};
    const int64_t n64 = static_cast<int64_t>(seg0) + seg1 + seg2;
    if (seg0 < 0 || seg1 < 0 || seg2 < 0 || n64 <= 0 || n64 > INT32_MAX || k <= 0 || !swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!out || !codes || !bscale) return SWL_ERR_BAD_ARG;
    if (!swl::gemm_fp8_geometry_ok(k) || !swl::gemm_fp8_segments_ok(seg)) return SWL_ERR_UNSUPPORTED;
    if (!swl::aligned16(out) || !swl::aligned16(codes)) return SWL_ERR_BAD_ARG;
    if (scale_rows != swl::fp8_segments_scale_rows(seg) || k_blocks != swl::moe_fp8_blocks(k)) return SWL_ERR_BAD_ARG;
    const int n = static_cast<int>(n64);
    const int64_t threads = n64 * (k / 8);
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::fp8_block_dequant_kernel<T>), dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<T *>(out), static_cast<const uint8_t *>(codes), bscale,
                           seg, n, k);
    });
    return swl::check_launch();
}
