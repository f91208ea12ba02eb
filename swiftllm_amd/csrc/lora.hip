// lora.hip — per-row low-rank adapter updates (multi-LoRA serving), gfx950. The reference has no LoRA; this is an addition.
//
// A projection group (one weight tensor of a layer: fused qkv, o, [up ; gate], down) has P column parts of its N outputs,
// each with its own rank-r_max adapter: A_stack [S, R = P * r_max, K] and B_stack [S, N, r_max] in the storage dtype, scale
// fp32 [S], S = adapter slots. Per row (token) with slot s >= 0:
//     t[row, c]  = sum_k x[row, k] * A[s][c, k]                                   (swl_lora_shrink, fp32)
//     y[row, n]  = T(float(y[row, n]) + scale[s] * sum_r t[row, off(n) + r] * B[s][n, r])      (swl_lora_expand)
// Rows are grouped by the host into tiles of <= 16 rows of ONE slot: tile_rows [num_tiles * 16] (row index, -1 = padding)
// and tile_slots [num_tiles]. Rows that are in no tile (slot -1) are neither read nor written.
//
// Both kernels put the tile's rows on the M side of 16 x 16 MFMA tiles, so a row's sums never see another row's data (a
// padding row is a row of zeros) and the order of a row's additions is fixed by (K, R, N) alone:
//   shrink: workgroup = (tile, 16 columns of t, K chunk of kLoraKChunk); wave w of 4 takes the 32-wide k steps w, w + 4, ...
//     of the chunk (v_mfma_f32_16x16x32: A = gathered x rows, B = A_stack rows, both straight from global memory as 16-byte
//     fragments), the four waves are added in wave order through LDS, the chunk's partial goes to slab kc of
//     t [KS, T, R] — no atomics; the consumer adds the KS = ceil(K / kLoraKChunk) slabs in slab order.
//   expand: workgroup = (tile, 4 waves x kLoraTilesPerWave 16-column tiles of y). t is summed over its slabs in fp32 and fed
//     as hi + lo 16-bit halves (two MFMAs, as attend_block_mfma feeds P: t is never rounded to 16 bits; float16 rows are
//     first scaled by an exact power of two that puts the row's largest |t| at 2^14, so that the lo halves stay normal
//     numbers and a large t cannot overflow — undone exactly after the MFMAs). r_max 8 / 16: one v_mfma_f32_16x16x16
//     pair (r_max 8: the upper half of k is zero), 32 / 64: one / two v_mfma_f32_16x16x32 pairs. (r_max 8 / 16 load B as 8 bytes per lane,
//     not the 16 of every other access in csrc/: the 16x16x16 operand is four values per lane and a B row is 16 / 32 bytes.) The tile goes through a
//     wave-private LDS transpose so that y is read, updated in fp32 and stored (ONE rounding) as 16-byte row fragments.
#include "attn_mfma.h"

namespace swl {

constexpr int kLoraKChunk = 1024;       // k columns per shrink workgroup (a multiple of 4 waves x 32)
constexpr int kLoraTilesPerWave = 4;    // 16-column tiles of y per expand wave
constexpr int kLoraMaxParts = 4;

struct LoraParts {
    int32_t n_begin[kLoraMaxParts], n_end[kLoraMaxParts], t_off[kLoraMaxParts];
    int32_t count;
};

template <typename T>
__global__ __launch_bounds__(256) void lora_shrink_kernel(const T *__restrict__ x, const T *__restrict__ a,
                                                          float *__restrict__ t, const int32_t *__restrict__ tile_rows,
                                                          const int32_t *__restrict__ tile_slots, int num_tokens, int K,
                                                          int R, int S, int64_t x_row_stride) {
    __shared__ __attribute__((aligned(16))) float red[4][16][16];
    const int tile = blockIdx.x, ct = blockIdx.y, kc = blockIdx.z;
    const int slot = tile_slots[tile];
    if (slot < 0 || slot >= S) return;      // (uniform)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    int row = tile_rows[tile * 16 + i16];
    if (row >= num_tokens) row = -1;
    const int c = ct * 16 + i16;
    const T *xp = x + static_cast<int64_t>(row < 0 ? 0 : row) * x_row_stride + 8 * q;
    const T *ap = a + (static_cast<int64_t>(slot) * R + (c < R ? c : 0)) * K + 8 * q;
    const bool x_on = row >= 0, a_on = c < R;
    const int k_begin = kc * kLoraKChunk;
    const int k_end = min(K, k_begin + kLoraKChunk);    // (K % 128 == 0: every wave runs the same number of steps)
    vec8_t<T> zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = to_t<T>(0.f);
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = k_begin + 32 * wave; k < k_end; k += 128) {
        const vec8_t<T> xf = x_on ? load8(xp + k) : zero;
        const vec8_t<T> af = a_on ? load8(ap + k) : zero;
        acc = mfma16x32(xf, af, acc);
    }
    mfma_results_ready<4>(acc);
    // acc[r] = partial of t[tile row 4q + r][column ct * 16 + i16]
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][4 * q + r][i16] = acc[r];
    __syncthreads();
    if (wave != 0) return;
    const int rr = lane >> 2, c0 = 4 * (lane & 3);
    float4_t sum = *reinterpret_cast<const float4_t *>(&red[0][rr][c0]);
#pragma unroll
    for (int w = 1; w < 4; ++w) sum += *reinterpret_cast<const float4_t *>(&red[w][rr][c0]);
    const int orow = tile_rows[tile * 16 + rr];
    if (orow < 0 || orow >= num_tokens || ct * 16 + c0 >= R) return;      // (R % 4 == 0: a fragment is inside or outside)
    float *tp = t + (static_cast<int64_t>(kc) * num_tokens + orow) * R + ct * 16 + c0;
    *reinterpret_cast<float4_t *>(tp) = sum;
}

// sum over the KS slabs, in slab order, of 4 consecutive fp32 values of t
__device__ __forceinline__ float4_t lora_t4(const float *p, int ks, int64_t slab_stride) {
    float4_t s = *reinterpret_cast<const float4_t *>(p);
    for (int k = 1; k < ks; ++k) s += *reinterpret_cast<const float4_t *>(p + k * slab_stride);
    return s;
}

template <typename T, int RMAX>
__global__ __launch_bounds__(256) void lora_expand_kernel(T *__restrict__ y, const float *__restrict__ t,
                                                          const T *__restrict__ b, const float *__restrict__ scale,
                                                          const int32_t *__restrict__ tile_rows,
                                                          const int32_t *__restrict__ tile_slots, LoraParts parts,
                                                          int num_tokens, int N, int R, int KS, int S,
                                                          int64_t y_row_stride) {
    constexpr bool WIDE = RMAX >= 32;               // 16x16x32 steps (8 k values per lane), else one 16x16x16 (4 per lane)
    constexpr int STEPS = WIDE ? RMAX / 32 : 1;
    constexpr int PER = WIDE ? 8 : 4;
    __shared__ __attribute__((aligned(16))) float stage[4][16][20];             // per wave: 16 rows x 16 columns, 80-byte pitch (16-byte aligned rows)
    const int tile = blockIdx.x;
    const int slot = tile_slots[tile];
    if (slot < 0 || slot >= S) return;              // (uniform)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    int arow = tile_rows[tile * 16 + i16];          // the row this lane supplies A (= t) fragments of
    if (arow >= num_tokens) arow = -1;
    const bool k_on = RMAX >= 16 || q < 2;          // r_max 8: k = 4q + j < 8
    const float sc = scale[slot];
    const int64_t slab = static_cast<int64_t>(num_tokens) * R;
    const int nt0 = (blockIdx.y * 4 + wave) * kLoraTilesPerWave;

    float tf[STEPS][PER];
    typename Vec8<T>::type ah8[STEPS], al8[STEPS];
    typename Vec4<T>::type ah4, al4;
    float inv = 1.0f;
    int cur = -1;
    for (int i = 0; i < kLoraTilesPerWave; ++i) {
        const int n0 = (nt0 + i) * 16;
        if (n0 >= N) break;                         // (uniform)
        int p = 0;
        while (p + 1 < parts.count && n0 >= parts.n_end[p]) ++p;
        if (p != cur) {                             // (uniform) the t columns of this part, as hi / lo fragments
            cur = p;
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
#pragma unroll
                for (int j = 0; j < PER; ++j) tf[s][j] = 0.f;
                if (arow >= 0 && k_on) {
                    const float *tp = t + static_cast<int64_t>(arow) * R + parts.t_off[p] + 32 * s + PER * q;
                    const float4_t v0 = lora_t4(tp, KS, slab);
#pragma unroll
                    for (int j = 0; j < 4; ++j) tf[s][j] = v0[j];
                    if constexpr (WIDE) {
                        const float4_t v1 = lora_t4(tp + 4, KS, slab);
#pragma unroll
                        for (int j = 0; j < 4; ++j) tf[s][4 + j] = v1[j];
                    }
                }
            }
            float up = 1.0f;
            if constexpr (std::is_same<T, f16>::value) {
                // exact power-of-two scaling of the row: its largest |t| lands in [2^14, 2^15)
                float m = 0.f;
#pragma unroll
                for (int s = 0; s < STEPS; ++s)
#pragma unroll
                    for (int j = 0; j < PER; ++j) m = fmaxf(m, fabsf(tf[s][j]));
                m = rows_allreduce_max(m);          // over the four lanes (q) that hold this row
                int e = static_cast<int>((__float_as_uint(m) >> 23) & 0xffu) - 127;
                e = max(e, -100);
                up = __uint_as_float(static_cast<uint32_t>(127 + 14 - e) << 23);
                inv = __uint_as_float(static_cast<uint32_t>(127 - 14 + e) << 23);
            }
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const float v = tf[s][j] * up;
                    const T hi = to_t<T>(v);
                    const T lo = to_t<T>(v - to_f(hi));
                    if constexpr (WIDE) {
                        ah8[s][j] = hi;
                        al8[s][j] = lo;
                    } else {
                        ah4[j] = hi;
                        al4[j] = lo;
                    }
                }
            }
        }
        // B fragments: B[slot][n0 + i16][k], k = 32 s + 8 q + j (16x16x32) or 4 q + j (16x16x16)
        const T *bp = b + (static_cast<int64_t>(slot) * N + n0 + i16) * RMAX + PER * q;
        float4_t acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (WIDE) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const vec8_t<T> bf = load8(bp + 32 * s);
                acc = mfma16x32(ah8[s], bf, acc);
                acc = mfma16x32(al8[s], bf, acc);
            }
        } else {
            typename Vec4<T>::type bf;
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = to_t<T>(0.f);
            if (k_on) bf = *reinterpret_cast<const typename Vec4<T>::type *>(bp);
            acc = mfma16x16(__builtin_bit_cast(short4_t, ah4), bf, acc);
            acc = mfma16x16(__builtin_bit_cast(short4_t, al4), bf, acc);
        }
        mfma_results_ready<4>(acc);
        // acc[r] = delta of (tile row 4q + r, column n0 + i16), still carrying that row's power-of-two scale
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float d = acc[r];
            if constexpr (std::is_same<T, f16>::value) d *= __shfl(inv, 4 * q + r, 64);   // (lane 4q + r holds row 4q + r)
            stage[wave][4 * q + r][i16] = sc * d;
        }
        // wave-private transpose (in-order LDS pipeline of one wave: no barrier): lane -> (row, 8 columns)
        if (lane < 32) {
            const int rr = lane >> 1, c0 = 8 * (lane & 1);
            const int orow = tile_rows[tile * 16 + rr];
            const float4_t d0 = *reinterpret_cast<const float4_t *>(&stage[wave][rr][c0]);
            const float4_t d1 = *reinterpret_cast<const float4_t *>(&stage[wave][rr][c0 + 4]);
            if (orow >= 0 && orow < num_tokens) {
                T *yp = y + static_cast<int64_t>(orow) * y_row_stride + n0 + c0;
                vec8_t<T> v = load8(yp);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = to_t<T>(to_f(v[j]) + d0[j]);
                    v[4 + j] = to_t<T>(to_f(v[4 + j]) + d1[j]);
                }
                store8(yp, v);
            }
        }
    }
}

inline bool lora_rank_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }

} // namespace swl

extern "C" int swl_lora_k_splits(int32_t k) {
    return k <= 0 ? 0 : (k + swl::kLoraKChunk - 1) / swl::kLoraKChunk;
}

extern "C" int swl_lora_shrink(float *t, const void *x, const void *a_stack, const int32_t *tile_rows,
                               const int32_t *tile_slots, int32_t num_tiles, int32_t num_tokens, int32_t k, int32_t r_total,
                               int32_t num_slots, int64_t x_row_stride, int32_t dtype, swl_stream_t stream) {
    if (num_tiles < 0 || num_tokens < 0 || k <= 0 || r_total <= 0 || num_slots <= 0) return SWL_ERR_BAD_ARG;
    if (x_row_stride < k) return SWL_ERR_BAD_ARG;
    if (dtype != SWL_F16 && dtype != SWL_BF16) return SWL_ERR_BAD_ARG;
    if (k % 128 != 0 || r_total % 8 != 0 || r_total > swl::kLoraMaxParts * 64) return SWL_ERR_UNSUPPORTED;
    if (x_row_stride % 8 != 0) return SWL_ERR_UNSUPPORTED;
    if (num_tiles == 0 || num_tokens == 0) return SWL_OK;
    if (!t || !x || !a_stack || !tile_rows || !tile_slots) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(t) || !swl::aligned16(x) || !swl::aligned16(a_stack)) return SWL_ERR_BAD_ARG;
    const int ks = swl_lora_k_splits(k);
    if (ks > 65535) return SWL_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(num_tiles), static_cast<unsigned>((r_total + 15) / 16), static_cast<unsigned>(ks));
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::lora_shrink_kernel<T>), grid, dim3(256), 0, s, static_cast<const T *>(x),
                           static_cast<const T *>(a_stack), t, tile_rows, tile_slots, num_tokens, k, r_total, num_slots,
                           x_row_stride);
    });
    return swl::check_launch();
}

extern "C" int swl_lora_expand(void *y, const float *t, const void *b_stack, const float *scale, const int32_t *tile_rows,
                               const int32_t *tile_slots, const int32_t *parts, int32_t num_parts, int32_t num_tiles,
                               int32_t num_tokens, int32_t n, int32_t r_max, int32_t r_total, int32_t k_splits,
                               int32_t num_slots, int64_t y_row_stride, int32_t dtype, swl_stream_t stream) {
    if (num_tiles < 0 || num_tokens < 0 || n <= 0 || r_total <= 0 || num_slots <= 0 || k_splits <= 0 || num_parts <= 0)
        return SWL_ERR_BAD_ARG;
    if (y_row_stride < n) return SWL_ERR_BAD_ARG;
    if (dtype != SWL_F16 && dtype != SWL_BF16) return SWL_ERR_BAD_ARG;
    if (!parts) return SWL_ERR_BAD_ARG;             // (a host array, read here)
    if (!swl::lora_rank_ok(r_max) || num_parts > swl::kLoraMaxParts || y_row_stride % 8 != 0) return SWL_ERR_UNSUPPORTED;
    swl::LoraParts lp = {};
    lp.count = num_parts;
    int at = 0;
    for (int p = 0; p < num_parts; ++p) {           // the parts tile [0, n) in order; each reads r_max columns of t
        const int nb = parts[3 * p], ne = parts[3 * p + 1], off = parts[3 * p + 2];
        if (nb != at || ne <= nb || off < 0 || off + r_max > r_total) return SWL_ERR_BAD_ARG;
        if ((ne - nb) % 16 != 0 || off % 8 != 0) return SWL_ERR_UNSUPPORTED;
        lp.n_begin[p] = nb, lp.n_end[p] = ne, lp.t_off[p] = off;
        at = ne;
    }
    if (at != n) return SWL_ERR_BAD_ARG;
    if (r_total % 8 != 0) return SWL_ERR_UNSUPPORTED;
    if (num_tiles == 0 || num_tokens == 0) return SWL_OK;
    if (!y || !t || !b_stack || !scale || !tile_rows || !tile_slots) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(y) || !swl::aligned16(t) || !swl::aligned16(b_stack)) return SWL_ERR_BAD_ARG;
    const int per_wg = 16 * 4 * swl::kLoraTilesPerWave;
    const unsigned gy = static_cast<unsigned>((n + per_wg - 1) / per_wg);
    if (gy > 65535u) return SWL_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(num_tiles), gy);
#define SWL_LORA_EXPAND(RMAX)                                                                                              \
    hipLaunchKernelGGL((swl::lora_expand_kernel<T, RMAX>), grid, dim3(256), 0, s, static_cast<T *>(y), t,                  \
                       static_cast<const T *>(b_stack), scale, tile_rows, tile_slots, lp, num_tokens, n, r_total, k_splits, \
                       num_slots, y_row_stride)
    SWL_DISPATCH_DTYPE(dtype, T, {
        switch (r_max) {
        case 8: SWL_LORA_EXPAND(8); break;
        case 16: SWL_LORA_EXPAND(16); break;
        case 32: SWL_LORA_EXPAND(32); break;
        default: SWL_LORA_EXPAND(64); break;
        }
    });
#undef SWL_LORA_EXPAND
    return swl::check_launch();
}
