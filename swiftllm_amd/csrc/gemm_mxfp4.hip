// gemm_mxfp4.hip — dense projections on MXFP4 weights (e2m1 codes, one e8m0 scale per 32 k) in PACKED order, quantised from
// a 16-bit checkpoint at load, gfx950, bfloat16. The numeric contract, the packed orders of codes and scales, the walk and
// the chain of one output element: gemm_mxfp4.h.
//
//   swl_gemm_mxfp4_quantise_pack  16-bit row-major w[N, K] -> packed codes + scale bytes, one pass: a wave per scale group
//                                 (16 rows x up to four k tiles); a lane's 32 elements of a tile are one MX block, so the
//                                 block maximum needs no cross-lane step, and the lane's four scale bytes are one dword store
//   swl_gemm_mxfp4                y[M, N] = x[M, K] . W^T for 1 <= M <= 64 tokens: the weight-streaming kernel
//   swl_gemm_mxfp4_silu_gate      act[M, I] = up * silu(gate) over [up ; gate] codes: the same walk, two row groups a wave
//   swl_mxfp4_dequant             out[N, K] = bf16(e2m1(code) * 2^e), row-major: the unpacking kernel — the executable
//                                 definition of the packed orders, and the image the library GEMM multiplies above 64 tokens
//   swl_gemm_mxfp4_supported, swl_gemm_mxfp4_choose_splits: host arithmetic
//
// With k_splits > 1 the streaming kernel writes fp32 slabs [k_splits][M][weight rows] into the caller's workspace and
// gemm_fp8_row_finish_kernel (gemm_fp8_row.h, SCALED = false), launched behind it on the same stream, adds them in slice
// order and runs the epilogue.
#include "gemm_mxfp4.h"

namespace swl {

constexpr int kMxXPitch = kMxChunk + 8;                     // elements between x rows in LDS: 528 bytes
constexpr int kMxChunkTiles = kMxChunk / kMxKStep;          // 2
constexpr int kMxThreads = 64 * kMxWaves;
constexpr int kMxRingChunks = kMxRing / kMxChunkTiles;      // 4: the chunk loop is unrolled by it, so a ring slot is static
static_assert(kMxRing % kMxChunkTiles == 0 && kMxRingChunks % 2 == 0, "a ring slot and an x buffer per unrolled chunk");

__device__ __forceinline__ int mx_wave() { return __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)); }

// 8 codes (one dword, k order = nibble order) times 2^e -> 8 bfloat16, exact: four v_cvt_scalef32_pk_bf16_fp4
__device__ __forceinline__ vec8_t<bf16> mxfp4x8_to_bf16(unsigned w, float scale) {
    const vec2_t<bf16> a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
    const vec2_t<bf16> b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
    const vec2_t<bf16> c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
    const vec2_t<bf16> d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
    return vec8_t<bf16>{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// 2^e of the scale byte `j` of a lane's scale dword, as the fp32 the convert takes
__device__ __forceinline__ float mx_scale(unsigned dword, int j) {
    return __builtin_bit_cast(float, ((dword >> (8 * j)) & 0xffu) << 23);
}

// A wave per (row group, scale group): up to four k tiles, each lane its own MX block of each.
template <typename T>
__global__ __launch_bounds__(256) void mxfp4_quantise_pack_kernel(uint8_t *__restrict__ codes, uint8_t *__restrict__ scales,
                                                                  const T *__restrict__ w, int N, int K) {
    const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4, KT = K / kMxKStep, KG = mxfp4_scale_groups(KT);
    const int64_t groups = static_cast<int64_t>(N / 16) * KG;
    for (int64_t g = blockIdx.x * 4ll + (threadIdx.x >> 6); g < groups; g += static_cast<int64_t>(gridDim.x) * 4ll) {
        const int nt = static_cast<int>(g / KG), kg = static_cast<int>(g % KG);
        unsigned sdword = 0;
#pragma unroll
        for (int j = 0; j < kMxScaleGroup; ++j) {
            const int kt = kMxScaleGroup * kg + j;
            unsigned byte = 127u;                           // past KT
            if (kt < KT) {
                const T *src = w + static_cast<int64_t>(16 * nt + i16) * K + kMxKStep * kt + kMxBlock * q;
                float v[kMxBlock];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const vec8_t<T> r = load8(src + 8 * p);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[8 * p + i] = to_f(r[i]);
                }
                float amax = 0.f;
#pragma unroll
                for (int i = 0; i < kMxBlock; ++i) amax = fmaxf(amax, fabsf(v[i]));
                const int e = mxfp4_block_exponent(__builtin_bit_cast(unsigned, amax));
                const float inv = __builtin_bit_cast(float, static_cast<unsigned>(127 - e) << 23);    // 2^-e, e <= 126 here
                u32x4_t out;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    unsigned word = 0;
#pragma unroll
                    for (int i = 0; i < 8; ++i) word |= mxfp4_code(__fmul_rn(v[8 * d + i], inv)) << (4 * i);
                    out[d] = word;
                }
                *reinterpret_cast<u32x4_t *>(codes + mxfp4_tile_byte(nt, kt, KT, lane)) = out;
                byte = static_cast<unsigned>(e + 127);
            }
            sdword |= byte << (8 * j);
        }
        *reinterpret_cast<unsigned *>(scales + mxfp4_scale_byte(nt, kg, KG, lane)) = sdword;
    }
}

// The unpacking kernel: a wave per tile reads the tile's 1 KiB and its scale bytes and writes 16 rows x 128 elements of
// the row-major image.
__global__ __launch_bounds__(256) void mxfp4_unpack_kernel(bf16 *__restrict__ out, const uint8_t *__restrict__ codes,
                                                           const uint8_t *__restrict__ scales, int N, int K) {
    const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4, KT = K / kMxKStep, KG = mxfp4_scale_groups(KT);
    const int64_t tiles = static_cast<int64_t>(N / 16) * KT;
    for (int64_t t = blockIdx.x * 4ll + (threadIdx.x >> 6); t < tiles; t += static_cast<int64_t>(gridDim.x) * 4ll) {
        const int nt = static_cast<int>(t / KT), kt = static_cast<int>(t % KT);
        const u32x4_t raw = *reinterpret_cast<const u32x4_t *>(codes + mxfp4_tile_byte(nt, kt, KT, lane));
        const unsigned sd = *reinterpret_cast<const unsigned *>(scales + mxfp4_scale_byte(nt, kt / kMxScaleGroup, KG, lane));
        const float s = mx_scale(sd, kt % kMxScaleGroup);
        bf16 *dst = out + static_cast<int64_t>(16 * nt + i16) * K + kMxKStep * kt + kMxBlock * q;
#pragma unroll
        for (int d = 0; d < 4; ++d) store8(dst + 8 * d, mxfp4x8_to_bf16(raw[d], s));
    }
}

// MT token tiles, NB row groups a wave (1: y; 2: up and gate of the SiLU-gate form, `nb_stride` weight rows apart).
template <int MT, int NB>
__global__ __launch_bounds__(kMxThreads) void gemm_mxfp4_kernel(bf16 *__restrict__ out, float *__restrict__ slabs,
                                                                const bf16 *__restrict__ x, const uint8_t *__restrict__ w,
                                                                const uint8_t *__restrict__ scales, int M, int n_out, int K,
                                                                int nb_stride, int64_t x_row_stride) {
    using T = bf16;
    __shared__ __attribute__((aligned(16))) T xs[2][MT * 16][kMxXPitch];
    const int lane = threadIdx.x & 63, wave = mx_wave();
    const int i16 = lane & 15, q = lane >> 4;
    const int KT = K / kMxKStep, KG = mxfp4_scale_groups(KT), ks = gridDim.y, split = blockIdx.y;
    const int t_begin = fp8_row_split_first(split, ks, KT), t_end = fp8_row_split_first(split + 1, ks, KT);
    const int k_begin = t_begin * kMxKStep, k_end = t_end * kMxKStep;
    const int nchunks = (k_end - k_begin + kMxChunk - 1) / kMxChunk;
    const int n0 = (static_cast<int>(blockIdx.x) * kMxWaves + wave) * 16;           // (uniform per wave)
    const bool active = n0 < n_out;                         // a last workgroup's spare waves only help to stage x

    // ---- x: this thread's 16-byte pieces of a chunk (2 MT of them), rows as full lines ----
    constexpr int kXLoads = MT * 16 * (kMxChunk / 8) / kMxThreads;                  // 2 MT
    vec8_t<T> xr[kXLoads];
    auto x_fetch = [&](int c) {
        const int kc = k_begin + c * kMxChunk;
#pragma unroll
        for (int p = 0; p < kXLoads; ++p) {
            const int flat = p * kMxThreads + threadIdx.x, row = flat >> 5, k = kc + 8 * (flat & 31);
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
            const int flat = p * kMxThreads + threadIdx.x;
            store8(&xs[buf][flat >> 5][8 * (flat & 31)], xr[p]);
        }
    };

    // ---- codes: the row group's contiguous run, tile t is 1 KiB * t in; a ring of kMxRing tiles in registers.
    //      scales: the row group's dwords, scale group g is 256 B * g in; two dwords (groups g and g + 1) ----
    const int nt0 = active ? n0 / 16 : 0;
    const uint8_t *wp = w + mxfp4_tile_byte(nt0, 0, KT, lane);
    const uint8_t *sp = scales + mxfp4_scale_byte(nt0, 0, KG, lane);
    const int64_t wb = mxfp4_tile_byte(nb_stride / 16, 0, KT, 0), sb = mxfp4_scale_byte(nb_stride / 16, 0, KG, 0);
    u32x4_t wr[kMxRing][NB];
    unsigned sc0[NB], sc1[NB];                              // the dwords of the group being walked and of the next one
    auto w_fetch = [&](auto slot, int t) {                  // tile t into the slot; past the slice: nothing
        if (active && t < t_end) {
#pragma unroll
            for (int b = 0; b < NB; ++b) wr[slot.value][b] = load16b_nt(wp + b * wb + static_cast<int64_t>(kMxTileBytes) * t);
        }
    };
    auto s_fetch = [&](unsigned (&dst)[NB], int g) {        // scale group g; past the slice: nothing
        if (active && kMxScaleGroup * g < t_end) {
#pragma unroll
            for (int b = 0; b < NB; ++b) dst[b] = *reinterpret_cast<const unsigned *>(sp + b * sb + 256ll * g);
        }
    };

    float4_t run[NB][MT];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int t = 0; t < MT; ++t) run[b][t] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < NB; ++b) sc0[b] = sc1[b] = 0u;

    x_fetch(0);
    s_fetch(sc0, t_begin / kMxScaleGroup), s_fetch(sc1, t_begin / kMxScaleGroup + 1);
    w_fetch(IntTag<0>{}, t_begin), w_fetch(IntTag<1>{}, t_begin + 1), w_fetch(IntTag<2>{}, t_begin + 2);
    w_fetch(IntTag<3>{}, t_begin + 3), w_fetch(IntTag<4>{}, t_begin + 4), w_fetch(IntTag<5>{}, t_begin + 5);
    w_fetch(IntTag<6>{}, t_begin + 6), w_fetch(IntTag<7>{}, t_begin + 7);
    x_put(0);
    __syncthreads();

    auto chunk = [&](int c, auto ring_chunk) {              // chunk c of the slice; ring_chunk = c % kMxRingChunks
        constexpr int P = decltype(ring_chunk)::value, BUF = P & 1;
        const int tc = t_begin + c * kMxChunkTiles;
        const bool more = c + 1 < nchunks;                  // (uniform over the workgroup)
        if (more) x_fetch(c + 1);
        if (active) {
            auto tile = [&](auto u) {
                constexpr int U = decltype(u)::value;
                const int t = tc + U;                       // (uniform)
                if (t % kMxScaleGroup == 0 && t != t_begin) {   // the walk enters a scale group: ask for the next one's dword
#pragma unroll
                    for (int b = 0; b < NB; ++b) sc0[b] = sc1[b];
                    s_fetch(sc1, t / kMxScaleGroup + 1);
                }
                const T *ax = &xs[BUF][i16][U * kMxKStep + kMxBlock * q];
                float sf[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) sf[b] = mx_scale(sc0[b], t % kMxScaleGroup);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    vec8_t<T> a[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m) a[m] = load8(ax + m * 16 * kMxXPitch + 8 * s);
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const vec8_t<T> wf = mxfp4x8_to_bf16(wr[kMxChunkTiles * P + U][b][s], sf[b]);
#pragma unroll
                        for (int m = 0; m < MT; ++m) run[b][m] = mfma16x32(a[m], wf, run[b][m]);
                    }
                }
                w_fetch(IntTag<kMxChunkTiles * P + U>{}, t + kMxRing);              // the slot's next tile, 1024 k ahead
            };
            tile(IntTag<0>{});                              // (a chunk of the slice holds at least one tile)
            if (tc + 1 < t_end) tile(IntTag<1>{});
        }
        if (more) x_put(BUF ^ 1);
        __syncthreads();                                    // chunk c + 1 is in place; chunk c's buffer is free for c + 2
    };
    for (int c = 0; c < nchunks; c += kMxRingChunks) {
        chunk(c, IntTag<0>{});
        if (c + 1 < nchunks) chunk(c + 1, IntTag<1>{});
        if (c + 2 < nchunks) chunk(c + 2, IntTag<2>{});
        if (c + 3 < nchunks) chunk(c + 3, IntTag<3>{});
    }
    if (!active) return;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int t = 0; t < MT; ++t) mfma_results_tie(run[b][t]);
    mfma_results_ready<4>(run[NB - 1][MT - 1]);

    // run[b][t][r] = (row 16 t + 4 q + r, column n0 + i16) of row group b
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
                out[static_cast<int64_t>(row) * n_out + n0 + i16] = fp8_up_gate_act<T>(run[0][t][r], run[1][t][r], 1.f, 1.f);
            } else {
                out[static_cast<int64_t>(row) * n_out + n0 + i16] = to_t<T>(run[0][t][r]);
            }
        }
}

// ---- host ----
template <int NB>
void launch_mxfp4_gemm(const GemmArgs &a, const uint8_t *scales, int nb_stride, int ks, hipStream_t stream) {
    const dim3 grid((a.N / 16 + kMxWaves - 1) / kMxWaves, ks);
    bf16 *out = static_cast<bf16 *>(a.out);
    float *slabs = static_cast<float *>(a.workspace);
    auto go = [&](auto mt) {
        hipLaunchKernelGGL((gemm_mxfp4_kernel<decltype(mt)::value, NB>), grid, dim3(kMxThreads), 0, stream, out, slabs,
                           static_cast<const bf16 *>(a.x), static_cast<const uint8_t *>(a.w), scales, a.M, a.N, a.K, nb_stride,
                           a.x_row_stride);
    };
    switch ((a.M + 15) / 16) {
    case 1: go(IntTag<1>{}); break;
    case 2: go(IntTag<2>{}); break;
    case 3: go(IntTag<3>{}); break;
    default: go(IntTag<4>{}); break;
    }
    if (ks > 1) {
        const int64_t threads = static_cast<int64_t>(a.M) * (a.N / 4);
        hipLaunchKernelGGL((gemm_fp8_row_finish_kernel<bf16, NB == 2, false>), dim3(static_cast<unsigned>((threads + 255) / 256)),
                           dim3(256), 0, stream, out, slabs, static_cast<const float *>(nullptr), ks, a.M, a.N,
                           NB == 2 ? 2 * a.N : a.N);
    }
}

// a valid dtype code that is not bfloat16 (float16: 2^e leaves its range) is SWL_ERR_UNSUPPORTED, anything else a bad argument
inline int mxfp4_dtype_check(int dtype) {
    return dtype == SWL_BF16 ? SWL_OK : moe_dtype_ok(dtype) ? SWL_ERR_UNSUPPORTED : SWL_ERR_BAD_ARG;
}

// What both GEMM entries check alike, in the order of gemm_fp8_row.hip: counts (M == 0 leaves with SWL_OK), operands, shape,
// strides, alignment (gemm_host.h), then the split and the workspace. `a.N`: output columns, `n_w`: weight rows.
inline bool mxfp4_gemm_settled(const GemmArgs &a, const void *scales, int n_w, int chosen, int &ks, int &rc) {
    if ((rc = check_gemm_counts(a)) != SWL_OK || a.M == 0) return true;
    if ((rc = check_gemm_operands(a)) != SWL_OK) return true;
    if (!scales) return rc = SWL_ERR_BAD_ARG, true;
    if (a.M > a.max_m || !mxfp4_geometry_ok(a.N, a.K)) return rc = SWL_ERR_UNSUPPORTED, true;
    if ((rc = check_gemm_strides(a)) != SWL_OK || (rc = check_gemm_alignment(a)) != SWL_OK) return true;
    if (!aligned16(scales)) return rc = SWL_ERR_BAD_ARG, true;
    ks = a.k_splits ? a.k_splits : chosen;
    if (!mxfp4_splits_ok(ks, a.K)) return rc = SWL_ERR_BAD_ARG, true;
    if (ks > 1 && (!a.workspace || a.workspace_bytes < static_cast<size_t>(ks) * a.M * n_w * sizeof(float)))
        return rc = SWL_ERR_BAD_ARG, true;
    return false;
}

// a conversion entry's checks: operands, dtype, geometry, alignment
inline int mxfp4_convert_check(const void *a, const void *b, const void *c, int n, int k, int dtype, bool any16) {
    if (n <= 0 || k <= 0 || !a || !b || !c) return SWL_ERR_BAD_ARG;
    if (const int rc = any16 ? (moe_dtype_ok(dtype) ? SWL_OK : SWL_ERR_BAD_ARG) : mxfp4_dtype_check(dtype); rc != SWL_OK) return rc;
    if (!mxfp4_geometry_ok(n, k)) return SWL_ERR_UNSUPPORTED;
    return aligned16(a) && aligned16(b) && aligned16(c) ? SWL_OK : SWL_ERR_BAD_ARG;
}

inline unsigned mxfp4_convert_grid(int64_t waves) { return static_cast<unsigned>(std::min<int64_t>((waves + 3) / 4, 1 << 16)); }

} // namespace swl

extern "C" int swl_gemm_mxfp4_supported(int32_t n, int32_t k, int32_t dtype) {
    return swl::mxfp4_geometry_ok(n, k) && dtype == SWL_BF16;
}

// Enough workgroups for the card's 256 CUs while a slice keeps at least a ring of k tiles (1024 k); at most 8 slices.
// 0: the shape is not taken.
extern "C" int swl_gemm_mxfp4_choose_splits(int32_t n, int32_t k) {
    if (!swl::mxfp4_geometry_ok(n, k)) return 0;
    const int wgs = (n / 16 + swl::kMxWaves - 1) / swl::kMxWaves, kt = k / swl::kMxKStep;
    int ks = 1;
    while (ks < swl::kMxMaxSplits && wgs * ks < 256 && kt / (2 * ks) >= swl::kMxRing) ks *= 2;
    return ks;
}

extern "C" int swl_gemm_mxfp4_quantise_pack(void *codes, void *scales, const void *w, int32_t n, int32_t k, int32_t dtype,
                                            swl_stream_t stream) {
    if (const int rc = swl::mxfp4_convert_check(codes, scales, w, n, k, dtype, true); rc != SWL_OK) return rc;
    const int64_t groups = static_cast<int64_t>(n / 16) * swl::mxfp4_scale_groups(k / swl::kMxKStep);
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::mxfp4_quantise_pack_kernel<T>), dim3(swl::mxfp4_convert_grid(groups)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<uint8_t *>(codes), static_cast<uint8_t *>(scales),
                           static_cast<const T *>(w), n, k);
    });
    return swl::check_launch();
}

extern "C" int swl_mxfp4_dequant(void *out, const void *codes, const void *scales, int32_t n, int32_t k, int32_t dtype,
                                 swl_stream_t stream) {
    if (const int rc = swl::mxfp4_convert_check(out, codes, scales, n, k, dtype, false); rc != SWL_OK) return rc;
    const int64_t tiles = static_cast<int64_t>(n / 16) * (k / swl::kMxKStep);
    hipLaunchKernelGGL(swl::mxfp4_unpack_kernel, dim3(swl::mxfp4_convert_grid(tiles)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<swl::bf16 *>(out), static_cast<const uint8_t *>(codes),
                       static_cast<const uint8_t *>(scales), n, k);
    return swl::check_launch();
}

extern "C" int swl_gemm_mxfp4(void *y, const void *x, const void *codes, const void *scales, void *workspace,
                              int64_t workspace_bytes, int32_t num_tokens, int32_t n, int32_t k, int64_t x_row_stride,
                              int32_t k_splits, int32_t dtype, swl_stream_t stream) {
    if (workspace_bytes < 0) return SWL_ERR_BAD_ARG;
    if (const int rc = swl::mxfp4_dtype_check(dtype); rc != SWL_OK) return rc;
    swl::GemmArgs a{y, x, codes, workspace, static_cast<size_t>(workspace_bytes), num_tokens, n, k, x_row_stride, n, k_splits,
                    swl::kMxMaxM, swl::kMxKStep};
    int ks = 0, rc = SWL_OK;
    if (swl::mxfp4_gemm_settled(a, scales, n, swl_gemm_mxfp4_choose_splits(n, k), ks, rc)) return rc;
    swl::launch_mxfp4_gemm<1>(a, static_cast<const uint8_t *>(scales), 0, ks, static_cast<hipStream_t>(stream));
    return swl::check_launch();
}

extern "C" int swl_gemm_mxfp4_silu_gate(void *act, const void *x, const void *codes, const void *scales, void *workspace,
                                        int64_t workspace_bytes, int32_t num_tokens, int32_t inter, int32_t k,
                                        int64_t x_row_stride, int32_t k_splits, int32_t dtype, swl_stream_t stream) {
    if (inter > INT32_MAX / 2 || workspace_bytes < 0) return SWL_ERR_BAD_ARG;
    if (const int rc = swl::mxfp4_dtype_check(dtype); rc != SWL_OK) return rc;
    swl::GemmArgs a{act, x, codes, workspace, static_cast<size_t>(workspace_bytes), num_tokens, inter, k, x_row_stride, inter,
                    k_splits, swl::kMxMaxM, swl::kMxKStep};
    int ks = 0, rc = SWL_OK;
    if (swl::mxfp4_gemm_settled(a, scales, 2 * inter, swl_gemm_mxfp4_choose_splits(inter, k), ks, rc)) return rc;
    swl::launch_mxfp4_gemm<2>(a, static_cast<const uint8_t *>(scales), inter, ks, static_cast<hipStream_t>(stream));
    return swl::check_launch();
}
