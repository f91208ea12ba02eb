// gemm_fp8_row.hip — dense projections on per-row-scaled FP8 (e4m3) weights in PACKED order, quantised from a 16-bit
// checkpoint at load, gfx950. The numeric contract, the packed order, the work split and the chain of one output element:
// gemm_fp8_row.h.
//
//   swl_gemm_fp8_row_quantise_pack  16-bit row-major w[N, K] + fp32 inv[N] -> packed codes, one pass: a wave per 16 x 64 tile,
//                                   a lane turns its 16 elements (two 16-byte loads) into one 16-byte store; the wave's store
//                                   is the tile's contiguous 1 KiB
//   swl_gemm_fp8_row                y[M, N] = x[M, K] . W^T for 1 <= M <= 64 tokens: the weight-streaming kernel
//   swl_gemm_fp8_row_silu_gate      act[M, I] = fp8_up_gate_act over [up ; gate] codes: the same walk, two row groups a wave
//   swl_fp8_row_dequant             out[N, K] = T(fp32(code) *_fp32 scale[row]), row-major: the unpacking kernel — the
//                                   executable definition of the packed order, and the 16-bit image the library GEMM
//                                   multiplies for steps of more than 64 tokens
//   swl_gemm_fp8_row_supported, swl_gemm_fp8_row_choose_splits: host arithmetic
//
// Why this walk (gemm_fp8_row.h has the details). The block-scaled kernel next door pays a fold per 128 k (VALU reads of the
// accumulators between the MFMAs, an s_nop each time) and asks for 16 rows x 64 bytes per load. Here the codes of a row
// group are one contiguous run, so the eight loads a wave keeps in flight are 8 KiB of consecutive bytes, and the scale
// enters once, in the epilogue: between the first and the last MFMA of a slice nothing reads an accumulator. x staging,
// ring depth and waves per workgroup are the block kernel's on purpose: the two forms then differ by the storage form only.
//
// With k_splits > 1 the streaming kernel writes fp32 slabs [k_splits][M][weight rows] into the caller's workspace and
// gemm_fp8_row_finish_kernel, launched behind it on the same stream, adds them in slice order and runs the epilogue.
#include "gemm_fp8_row.h"

namespace swl {

constexpr int kRowXPitch = kFp8RowChunk + 8;                // elements between x rows in LDS: 528 bytes
constexpr int kRowChunkSteps = kFp8RowChunk / kFp8KStep;    // 4
constexpr int kRowThreads = 64 * kFp8RowWaves;
static_assert(kFp8RowRing == 2 * kRowChunkSteps, "the ring is two chunks' tiles");

// the wave's index as a scalar: makes the row group and every code address's base uniform for the compiler
__device__ __forceinline__ int fp8_row_wave() { return __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)); }

template <typename T>
__global__ __launch_bounds__(256) void fp8_row_quantise_pack_kernel(uint8_t *__restrict__ codes, const T *__restrict__ w,
                                                                    const float *__restrict__ inv, int N, int K) {
    const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4, KT = K / kFp8KStep;
    const int64_t tiles = static_cast<int64_t>(N / 16) * KT;
    for (int64_t t = blockIdx.x * 4ll + (threadIdx.x >> 6); t < tiles; t += static_cast<int64_t>(gridDim.x) * 4ll) {
        const int nt = static_cast<int>(t / KT), kt = static_cast<int>(t % KT), row = 16 * nt + i16;
        const T *src = w + static_cast<int64_t>(row) * K + kFp8KStep * kt + 16 * q;
        *reinterpret_cast<u32x4_t *>(codes + fp8_row_tile_byte(nt, kt, KT, lane)) = quantise16<T>(load8(src), load8(src + 8), inv[row]);
    }
}

// The unpacking kernel: a wave per tile reads the tile's 1 KiB and writes 16 rows x 64 elements of the row-major image.
template <typename T>
__global__ __launch_bounds__(256) void fp8_row_unpack_kernel(T *__restrict__ out, const uint8_t *__restrict__ codes,
                                                             const float *__restrict__ scale, int N, int K) {
    const int lane = threadIdx.x & 63, i16 = lane & 15, q = lane >> 4, KT = K / kFp8KStep;
    const int64_t tiles = static_cast<int64_t>(N / 16) * KT;
    for (int64_t t = blockIdx.x * 4ll + (threadIdx.x >> 6); t < tiles; t += static_cast<int64_t>(gridDim.x) * 4ll) {
        const int nt = static_cast<int>(t / KT), kt = static_cast<int>(t % KT), row = 16 * nt + i16;
        const u32x4_t raw = *reinterpret_cast<const u32x4_t *>(codes + fp8_row_tile_byte(nt, kt, KT, lane));
        const float s = scale[row];
        vec8_t<T> lo, hi;
        fp8x16_to_t<T>(raw, lo, hi);
#pragma unroll
        for (int j = 0; j < 8; ++j) lo[j] = to_t<T>(__fmul_rn(to_f(lo[j]), s)), hi[j] = to_t<T>(__fmul_rn(to_f(hi[j]), s));
        T *dst = out + static_cast<int64_t>(row) * K + kFp8KStep * kt + 16 * q;
        store8(dst, lo);
        store8(dst + 8, hi);
    }
}

// MT token tiles, NB row groups a wave (1: y; 2: up and gate of the SiLU-gate form, `nb_stride` weight rows apart).
template <typename T, int MT, int NB>
__global__ __launch_bounds__(kRowThreads) void gemm_fp8_row_kernel(T *__restrict__ out, float *__restrict__ slabs,
                                                                   const T *__restrict__ x, const uint8_t *__restrict__ w,
                                                                   const float *__restrict__ scale, int M, int n_out, int K,
                                                                   int nb_stride, int64_t x_row_stride) {
    __shared__ __attribute__((aligned(16))) T xs[2][MT * 16][kRowXPitch];
    const int lane = threadIdx.x & 63, wave = fp8_row_wave();
    const int i16 = lane & 15, q = lane >> 4;
    const int KT = K / kFp8KStep, ks = gridDim.y, split = blockIdx.y;
    const int k_begin = fp8_row_split_first(split, ks, KT) * kFp8KStep;
    const int k_end = fp8_row_split_first(split + 1, ks, KT) * kFp8KStep;
    const int nchunks = (k_end - k_begin + kFp8RowChunk - 1) / kFp8RowChunk;
    const int n0 = (static_cast<int>(blockIdx.x) * kFp8RowWaves + wave) * 16;       // (uniform per wave)
    const bool active = n0 < n_out;                         // a last workgroup's spare waves only help to stage x

    // ---- x: this thread's 16-byte pieces of a chunk (2 MT of them), rows as full lines ----
    constexpr int kXLoads = MT * 16 * (kFp8RowChunk / 8) / kRowThreads;             // 2 MT
    vec8_t<T> xr[kXLoads];
    auto x_fetch = [&](int c) {
        const int kc = k_begin + c * kFp8RowChunk;
#pragma unroll
        for (int p = 0; p < kXLoads; ++p) {
            const int flat = p * kRowThreads + threadIdx.x, row = flat >> 5, k = kc + 8 * (flat & 31);
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
            const int flat = p * kRowThreads + threadIdx.x;
            store8(&xs[buf][flat >> 5][8 * (flat & 31)], xr[p]);
        }
    };

    // ---- codes: the row group's contiguous run; tile k / 64 is 16 k bytes in. A ring of two chunks' tiles in registers ----
    const uint8_t *wp = w + fp8_row_tile_byte(active ? n0 / 16 : 0, 0, KT, lane);
    const int64_t wb = fp8_row_tile_byte(nb_stride / 16, 0, KT, 0);
    u32x4_t wr[2][kRowChunkSteps][NB];
    auto w_fetch = [&](auto par, auto u, int k) {           // the tile at k into slot (par, u); past the slice: nothing
        if (active && k < k_end) {
#pragma unroll
            for (int b = 0; b < NB; ++b) wr[par.value][u.value][b] = load16b_nt(wp + b * wb + 16 * static_cast<int64_t>(k));
        }
    };

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
        const int kc = k_begin + c * kFp8RowChunk;
        const bool more = c + 1 < nchunks;                  // (uniform over the workgroup)
        if (more) x_fetch(c + 1);
        if (active) {
            auto step = [&](auto u) {
                constexpr int U = decltype(u)::value;
                const T *ax = &xs[par.value][i16][U * kFp8KStep + 16 * q];
                Fp8AFrag<T> a[MT];
#pragma unroll
                for (int t = 0; t < MT; ++t) a[t].lo = load8(ax + t * 16 * kRowXPitch), a[t].hi = load8(ax + t * 16 * kRowXPitch + 8);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    vec8_t<T> wlo, whi;
                    fp8x16_to_t<T>(wr[par.value][U][b], wlo, whi);
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        run[b][t] = mfma16x32(a[t].lo, wlo, run[b][t]);
                        run[b][t] = mfma16x32(a[t].hi, whi, run[b][t]);
                    }
                }
                w_fetch(par, u, kc + U * kFp8KStep + 2 * kFp8RowChunk);             // the slot's next tile, 512 k ahead
            };
            step(IntTag<0>{});                              // (a chunk of the slice holds at least one tile)
            if (kc + 1 * kFp8KStep < k_end) step(IntTag<1>{});
            if (kc + 2 * kFp8KStep < k_end) step(IntTag<2>{});
            if (kc + 3 * kFp8KStep < k_end) step(IntTag<3>{});
        }
        if (more) x_put(par.value ^ 1);
        __syncthreads();                                    // chunk c + 1 is in place; chunk c's buffer is free for c + 2
    };
    for (int c = 0; c < nchunks; c += 2) {
        chunk(c, IntTag<0>{});
        if (c + 1 < nchunks) chunk(c + 1, IntTag<1>{});
    }
    if (!active) return;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int t = 0; t < MT; ++t) mfma_results_tie(run[b][t]);
    mfma_results_ready<4>(run[NB - 1][MT - 1]);

    // run[b][t][r] = (row 16 t + 4 q + r, column n0 + i16) of row group b
    const int n_w = NB * nb_stride + (NB == 1 ? n_out : 0);     // weight rows: the width of a slab
    float s[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) s[b] = scale[n0 + i16 + b * nb_stride];
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
                out[static_cast<int64_t>(row) * n_out + n0 + i16] = fp8_up_gate_act<T>(run[0][t][r], run[1][t][r], s[0], s[1]);
            } else {
                out[static_cast<int64_t>(row) * n_out + n0 + i16] = to_t<T>(__fmul_rn(run[0][t][r], s[0]));
            }
        }
}

// ---- host ----
template <typename T, int NB>
void launch_fp8_row_gemm(const GemmArgs &a, const float *scale, int nb_stride, int ks, hipStream_t stream) {
    const dim3 grid((a.N / 16 + kFp8RowWaves - 1) / kFp8RowWaves, ks);
    T *out = static_cast<T *>(a.out);
    float *slabs = static_cast<float *>(a.workspace);
    auto go = [&](auto mt) {
        hipLaunchKernelGGL((gemm_fp8_row_kernel<T, decltype(mt)::value, NB>), grid, dim3(kRowThreads), 0, stream, out, slabs,
                           static_cast<const T *>(a.x), static_cast<const uint8_t *>(a.w), scale, a.M, a.N, a.K, nb_stride,
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
        hipLaunchKernelGGL((gemm_fp8_row_finish_kernel<T, NB == 2>), dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256),
                           0, stream, out, slabs, scale, ks, a.M, a.N, NB == 2 ? 2 * a.N : a.N);
    }
}

// What both GEMM entries check alike, in this order: counts (M == 0 leaves with SWL_OK), operands, shape, strides,
// alignment (gemm_host.h), then the split and the workspace. `a.N`: output columns, `n_w`: weight rows.
inline bool fp8_row_gemm_settled(const GemmArgs &a, const float *scale, int n_w, int chosen, int &ks, int &rc) {
    if ((rc = check_gemm_counts(a)) != SWL_OK || a.M == 0) return true;
    if ((rc = check_gemm_operands(a)) != SWL_OK) return true;
    if (!scale) return rc = SWL_ERR_BAD_ARG, true;
    if (a.M > a.max_m || !fp8_row_geometry_ok(a.N, a.K)) return rc = SWL_ERR_UNSUPPORTED, true;
    if ((rc = check_gemm_strides(a)) != SWL_OK || (rc = check_gemm_alignment(a)) != SWL_OK) return true;
    if (!aligned16(scale)) return rc = SWL_ERR_BAD_ARG, true;
    ks = a.k_splits ? a.k_splits : chosen;
    if (!fp8_row_splits_ok(ks, a.K)) return rc = SWL_ERR_BAD_ARG, true;
    if (ks > 1 && (!a.workspace || a.workspace_bytes < static_cast<size_t>(ks) * a.M * n_w * sizeof(float)))
        return rc = SWL_ERR_BAD_ARG, true;
    return false;
}

// a conversion entry's checks: operands, dtype, geometry, alignment
inline int fp8_row_convert_check(const void *a, const void *b, const void *c, int n, int k, int dtype) {
    if (n <= 0 || k <= 0 || !moe_dtype_ok(dtype) || !a || !b || !c) return SWL_ERR_BAD_ARG;
    if (!fp8_row_geometry_ok(n, k)) return SWL_ERR_UNSUPPORTED;
    return aligned16(a) && aligned16(b) && !(reinterpret_cast<uintptr_t>(c) & 3u) ? SWL_OK : SWL_ERR_BAD_ARG;
}

inline unsigned fp8_row_convert_grid(int n, int k) {
    const int64_t tiles = static_cast<int64_t>(n / 16) * (k / kFp8KStep);
    return static_cast<unsigned>(std::min<int64_t>((tiles + 3) / 4, 1 << 16));
}

} // namespace swl

extern "C" int swl_gemm_fp8_row_supported(int32_t n, int32_t k, int32_t dtype) {
    return swl::fp8_row_geometry_ok(n, k) && swl::moe_dtype_ok(dtype);
}

// Enough workgroups for the card's 256 CUs while a slice keeps at least a ring of k tiles (512 k); at most 8 slices: every
// slice writes 4 M bytes of slab per column beside its share of the column's K code bytes. 0: the shape is not taken.
extern "C" int swl_gemm_fp8_row_choose_splits(int32_t n, int32_t k) {
    if (!swl::fp8_row_geometry_ok(n, k)) return 0;
    const int wgs = (n / 16 + swl::kFp8RowWaves - 1) / swl::kFp8RowWaves, kt = k / swl::kFp8KStep;
    int ks = 1;
    while (ks < swl::kFp8RowMaxSplits && wgs * ks < 256 && kt / (2 * ks) >= swl::kFp8RowRing) ks *= 2;
    return ks;
}

extern "C" int swl_gemm_fp8_row_quantise_pack(void *codes, const void *w, const float *inv_scale, int32_t n, int32_t k,
                                              int32_t dtype, swl_stream_t stream) {
    if (const int rc = swl::fp8_row_convert_check(codes, w, inv_scale, n, k, dtype); rc != SWL_OK) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::fp8_row_quantise_pack_kernel<T>), dim3(swl::fp8_row_convert_grid(n, k)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<uint8_t *>(codes), static_cast<const T *>(w),
                           inv_scale, n, k);
    });
    return swl::check_launch();
}

extern "C" int swl_fp8_row_dequant(void *out, const void *codes, const float *scale, int32_t n, int32_t k, int32_t dtype,
                                   swl_stream_t stream) {
    if (const int rc = swl::fp8_row_convert_check(out, codes, scale, n, k, dtype); rc != SWL_OK) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::fp8_row_unpack_kernel<T>), dim3(swl::fp8_row_convert_grid(n, k)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<T *>(out), static_cast<const uint8_t *>(codes), scale,
                           n, k);
    });
    return swl::check_launch();
}

extern "C" int swl_gemm_fp8_row(void *y, const void *x, const void *codes, const float *scale, void *workspace,
                                int64_t workspace_bytes, int32_t num_tokens, int32_t n, int32_t k, int64_t x_row_stride,
                                int32_t k_splits, int32_t dtype, swl_stream_t stream) {
    if (workspace_bytes < 0 || !swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    swl::GemmArgs a{y, x, codes, workspace, static_cast<size_t>(workspace_bytes), num_tokens, n, k, x_row_stride, n, k_splits,
                    swl::kFp8RowMaxM, swl::kFp8KStep};
    int ks = 0, rc = SWL_OK;
    if (swl::fp8_row_gemm_settled(a, scale, n, swl_gemm_fp8_row_choose_splits(n, k), ks, rc)) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, { swl::launch_fp8_row_gemm<T, 1>(a, scale, 0, ks, static_cast<hipStream_t>(stream)); });
    return swl::check_launch();
}

extern "C" int swl_gemm_fp8_row_silu_gate(void *act, const void *x, const void *codes, const float *scale, void *workspace,
                                          int64_t workspace_bytes, int32_t num_tokens, int32_t inter, int32_t k,
                                          int64_t x_row_stride, int32_t k_splits, int32_t dtype, swl_stream_t stream) {
    if (inter > INT32_MAX / 2 || workspace_bytes < 0 || !swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    swl::GemmArgs a{act, x, codes, workspace, static_cast<size_t>(workspace_bytes), num_tokens, inter, k, x_row_stride, inter,
                    k_splits, swl::kFp8RowMaxM, swl::kFp8KStep};
    int ks = 0, rc = SWL_OK;
    if (swl::fp8_row_gemm_settled(a, scale, 2 * inter, swl_gemm_fp8_row_choose_splits(inter, k), ks, rc)) return rc;
    SWL_DISPATCH_DTYPE(dtype, T, { swl::launch_fp8_row_gemm<T, 2>(a, scale, inter, ks, static_cast<hipStream_t>(stream)); });
    return swl::check_launch();
}
