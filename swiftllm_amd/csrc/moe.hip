// moe.hip — mixture-of-experts FFN (Qwen3-MoE, Mixtral), gfx950. The reference has no MoE; this is an addition.
//
// A step of T tokens, E experts, k experts per token; "pair" p = t * k + slot is one (token, chosen expert). P = T * k
// pairs, at most kMoeMaxPairs per call (the Python layer walks longer steps in token blocks).
//
//   swl_moe_route         router logits [T, E] (float16 / bfloat16 / fp32) -> topk_ids [T, k] int32, topk_w [T, k] fp32.
//                         One wave per token. The k largest LOGITS are taken (softmax is monotonic), ties to the lowest
//                         expert id, slots in descending order. The softmax is evaluated in fp64 from the fp32 value of
//                         the logits and rounded ONCE to fp32: w = e_j / sum_all(e) or, normalised, e_j / sum_slots(e),
//                         e_i = exp(l_i - max l). A row with a NaN or an infinity gets ids 0..k-1 and weights 0 (the
//                         token's FFN output is then 0); nothing is indexed by a logit, so nothing can leave the buffers.
//   swl_moe_align         topk_ids -> tile_rows [max_tiles * 16] (pair index, -1 = padding) and tile_experts [max_tiles]
//                         (-1 = unused tile). ONE workgroup: a counting sort, stable in the pair index, so the tables are
//                         a function of topk_ids alone. Expert e's pairs fill ceil(count_e / 16) consecutive tiles; the
//                         tiles of the experts follow each other in expert order; max_tiles >= ceil(P / 16) + min(E, P)
//                         always suffices. The only atomics are the LDS counters of pairs per expert (integer sums:
//                         order-free). An id outside [0, E) is in no tile.
//   swl_moe_up_gate_silu  workgroup = (tile, 16 columns of I), 8 waves. The tile's gathered x rows are the M side of
//                         v_mfma_f32_16x16x32; wave w takes the 32-wide k steps w, w + 8, ... of that expert's up row block
//                         and gate row block (both straight from global memory as 16-byte fragments); the eight waves are
//                         added in wave order through LDS. up and gate are rounded to T, then act = up *_T T(silu(gate))
//                         (the arithmetic of silu_mul.hip). act [P, I] in T.
//   swl_moe_down          the same walk over act rows and expert_down [E, H, I]; y [P, H] stays fp32, unrounded.
//   swl_moe_combine       out[t, h] = T(sum over slots j = 0..k-1, in slot order, of topk_w[t, j] * y[t * k + j, h]), each
//                         product and each sum one fp32 operation; ONE rounding to T. No atomics.
//
// A row's sums never see another row's data (a padding row is a row of zeros, rows are the M side of the MFMA) and the order
// of its additions is fixed by (H, I, k) alone: the bits of out[t] are a function of x[t], its experts and its weights. No
// split over K depends on T. Unused tiles leave before any barrier (uniform branch on tile_experts).
#include "attn_mfma.h"

namespace swl {

constexpr int kMoeMaxExperts = 256;
constexpr int kMoeMaxTopK = 16;
constexpr int kMoeMaxPairs = 4096;
constexpr int kMoeWaves = 8;
constexpr int kMoeLogitsF32 = 2;

inline int moe_tile_bound(int pairs, int experts) { return (pairs + 15) / 16 + (experts < pairs ? experts : pairs); }

template <typename L>
__device__ __forceinline__ float moe_logit(const L *p) { return to_f(*p); }
template <>
__device__ __forceinline__ float moe_logit<float>(const float *p) { return *p; }

template <typename L>
__global__ __launch_bounds__(256) void moe_route_kernel(int32_t *__restrict__ topk_ids, float *__restrict__ topk_w,
                                                        const L *__restrict__ logits, int T, int E, int k, int norm,
                                                        int64_t row_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + wave;
    if (t >= T) return;                                     // (uniform per wave; no barrier in this kernel)
    const L *row = logits + static_cast<int64_t>(t) * row_stride;
    float v[4];
    bool bad = false;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        v[j] = -INFINITY;
        if (e < E) {
            v[j] = moe_logit<L>(row + e);
            bad |= !(fabsf(v[j]) < INFINITY);               // NaN or +-inf
            m = fmaxf(m, v[j]);
        }
    }
    int32_t *ids = topk_ids + static_cast<int64_t>(t) * k;
    float *ws = topk_w + static_cast<int64_t>(t) * k;
    if (__ballot(bad) != 0ull) {                            // (uniform)
        if (lane < k) ids[lane] = lane, ws[lane] = 0.f;
        return;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    const double md = static_cast<double>(m);
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (lane + 64 * j < E) sum += exp(static_cast<double>(v[j]) - md);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);   // (butterfly: every lane adds the same pairs)
    unsigned taken = 0u;
    double my_e = 0.0;
    int my_id = 0;
    for (int slot = 0; slot < k; ++slot) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane + 64 * j;
            if (e < E && !(taken >> j & 1u) && (v[j] > bv || bi == 0x7fffffff)) bv = v[j], bi = e;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const float ov = __shfl_xor(bv, s, 64);
            const int oi = __shfl_xor(bi, s, 64);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
        }
        // (k <= E: a candidate is always left)
        if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
        if (lane == slot) my_e = exp(static_cast<double>(bv) - md), my_id = bi;
    }
    double den = sum;
    if (norm) {
        den = lane < k ? my_e : 0.0;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) den += __shfl_xor(den, s, 64);
    }
    if (lane < k) ids[lane] = my_id, ws[lane] = static_cast<float>(my_e / den);
}

__global__ __launch_bounds__(1024) void moe_align_kernel(int32_t *__restrict__ tile_rows, int32_t *__restrict__ tile_experts,
                                                         const int32_t *__restrict__ topk_ids, int P, int E, int max_tiles) {
    __shared__ int counts[kMoeMaxExperts];
    __shared__ int starts[kMoeMaxExperts + 1];              // first tile of expert e; [E] = tiles in use
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kMoeMaxExperts) counts[tid] = 0;
    __syncthreads();
    for (int p = tid; p < P; p += 1024) {
        const int e = topk_ids[p];
        if (e >= 0 && e < E) atomicAdd(&counts[e], 1);
    }
    __syncthreads();
    if (wave == 0) {                                        // exclusive scan of the experts' tile counts: 4 experts a lane
        int n[4], mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * lane + j;
            n[j] = e < E ? (counts[e] + 15) >> 4 : 0;
            mine += n[j];
        }
        int incl = mine;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int o = __shfl_up(incl, s, 64);
            if (lane >= s) incl += o;
        }
        int at = incl - mine;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * lane + j;
            if (e < E) starts[e] = at;
            at += n[j];
        }
        if (lane == 63) starts[E] = incl;
    }
    __syncthreads();
    const int used = min(starts[E], max_tiles);             // (== starts[E] whenever max_tiles is the stated bound)
    for (int i = used + tid; i < max_tiles; i += 1024) tile_experts[i] = -1;
    for (int i = used * 16 + tid; i < max_tiles * 16; i += 1024) tile_rows[i] = -1;
    for (int e = wave; e < E; e += 16) {
        const int cnt = counts[e];
        if (cnt == 0) continue;                             // (uniform per wave)
        const int first = starts[e], nt = (cnt + 15) >> 4;
        if (first + nt > max_tiles) continue;               // (cannot happen under the stated bound; never write past it)
        const int base = first * 16;
        int run = 0;
        for (int c = 0; c < P && run < cnt; c += 64) {
            const int p = c + lane;
            const bool hit = p < P && topk_ids[p] == e;
            const unsigned long long mask = __ballot(hit);
            const int rank = run + __popcll(mask & ((1ull << lane) - 1ull));
            if (hit && rank < cnt) tile_rows[base + rank] = p;
            run += __popcll(mask);
        }
        for (int i = cnt + lane; i < nt * 16; i += 64) tile_rows[base + i] = -1;
        for (int i = lane; i < nt; i += 64) tile_experts[first + i] = e;
    }
}

// One (tile, 16 output columns) block of rows(A)[16, K] x W[e][n0 .. n0 + 16, K]^T for NB weight row blocks that share the
// A rows (NB = 2: up and gate, `nb_stride` elements apart). Leaves the sums, added in wave order, in `sum[b]` of the thread
// that owns (row tid >> 4, column tid & 15), tid < 256.
template <typename T, int NB>
__device__ __forceinline__ void moe_tile_gemm(float (&sum)[NB], float (*red)[kMoeWaves][16][16], const T *__restrict__ a,
                                              int64_t a_row, bool a_on, const T *__restrict__ w, int64_t nb_stride, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const T *ap = a + a_row + 8 * q;
    const T *wp = w + static_cast<int64_t>(i16) * K + 8 * q;
    vec8_t<T> zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = to_t<T>(0.f);
    float4_t acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = float4_t{0.f, 0.f, 0.f, 0.f};
    constexpr int kStep = 32 * kMoeWaves, kDepth = 4;       // kDepth k steps of loads in flight before their MFMAs
    int k = 32 * wave;
    for (; k + (kDepth - 1) * kStep < K; k += kDepth * kStep) {
        vec8_t<T> af[kDepth], wf[NB][kDepth];
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            af[u] = a_on ? load8(ap + k + u * kStep) : zero;
#pragma unroll
            for (int b = 0; b < NB; ++b) wf[b][u] = load8_nt(wp + b * nb_stride + k + u * kStep);
        }
#pragma unroll
        for (int u = 0; u < kDepth; ++u)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = mfma16x32(af[u], wf[b][u], acc[b]);
    }
    for (; k < K; k += kStep) {
        const vec8_t<T> af = a_on ? load8(ap + k) : zero;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = mfma16x32(af, load8_nt(wp + b * nb_stride + k), acc[b]);
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
        const int rr = threadIdx.x >> 4, cc = threadIdx.x & 15;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float s = red[b][0][rr][cc];
#pragma unroll
            for (int wv = 1; wv < kMoeWaves; ++wv) s += red[b][wv][rr][cc];
            sum[b] = s;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kMoeWaves) void moe_up_gate_silu_kernel(
    T *__restrict__ act, const T *__restrict__ x, const T *__restrict__ w, const int32_t *__restrict__ tile_rows,
    const int32_t *__restrict__ tile_experts, int P, int top_k, int H, int I, int E, int64_t x_row_stride) {
    __shared__ __attribute__((aligned(16))) float red[2][kMoeWaves][16][16];
    const int tile = blockIdx.x;
    const int e = tile_experts[tile];
    if (e < 0 || e >= E) return;                            // (uniform; before the barrier)
    const int n0 = blockIdx.y * 16;
    int pair = tile_rows[tile * 16 + (threadIdx.x & 15)];
    if (pair >= P) pair = -1;
    const bool on = pair >= 0;
    const int64_t tok = on ? pair / top_k : 0;
    float sum[2];
    moe_tile_gemm<T, 2>(sum, red, x, tok * x_row_stride, on, w + (static_cast<int64_t>(e) * 2 * I + n0) * H,
                        static_cast<int64_t>(I) * H, H);
    if (threadIdx.x >= 256) return;
    const int orow = tile_rows[tile * 16 + (threadIdx.x >> 4)];
    if (orow < 0 || orow >= P) return;
    const T up = to_t<T>(sum[0]);
    const float g = to_f(to_t<T>(sum[1]));
    const T silu = to_t<T>(g / (1.0f + expf(-g)));
    act[static_cast<int64_t>(orow) * I + n0 + (threadIdx.x & 15)] = mul_t<T>(up, silu);
}

template <typename T>
__global__ __launch_bounds__(64 * kMoeWaves) void moe_down_kernel(float *__restrict__ y, const T *__restrict__ act,
                                                                  const T *__restrict__ w,
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
    float sum[1];
    moe_tile_gemm<T, 1>(sum, red, act, (on ? pair : 0) * static_cast<int64_t>(I), on,
                        w + (static_cast<int64_t>(e) * H + n0) * I, 0, I);
    if (threadIdx.x >= 256) return;
    const int orow = tile_rows[tile * 16 + (threadIdx.x >> 4)];
    if (orow < 0 || orow >= P) return;
    y[static_cast<int64_t>(orow) * H + n0 + (threadIdx.x & 15)] = sum[0];
}

template <typename T>
__global__ __launch_bounds__(256) void moe_combine_kernel(T *__restrict__ out, const float *__restrict__ y,
                                                          const float *__restrict__ topk_w, int64_t items, int top_k, int H,
                                                          int64_t out_row_stride) {
    const int chunks = H / 8;
    for (int64_t item = blockIdx.x * 256ll + threadIdx.x; item < items; item += static_cast<int64_t>(gridDim.x) * 256ll) {
        const int64_t t = item / chunks;
        const int h = static_cast<int>(item - t * chunks) * 8;
        float4_t a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < top_k; ++j) {
            const float wj = topk_w[t * top_k + j];
            const float *yp = y + (t * top_k + j) * H + h;
            a += *reinterpret_cast<const float4_t *>(yp) * wj;
            b += *reinterpret_cast<const float4_t *>(yp + 4) * wj;
        }
        vec8_t<T> v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = to_t<T>(a[j]), v[4 + j] = to_t<T>(b[j]);
        store8(out + t * out_row_stride + h, v);
    }
}

inline bool moe_dtype_ok(int dtype) { return dtype == SWL_F16 || dtype == SWL_BF16; }

// SWL_OK when (T, k, E) is a legal step, else the error code
inline int moe_step_check(int num_tokens, int top_k, int num_experts) {
    if (num_tokens < 0 || top_k <= 0 || num_experts <= 0 || top_k > num_experts) return SWL_ERR_BAD_ARG;
    if (num_experts > kMoeMaxExperts || top_k > kMoeMaxTopK) return SWL_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(num_tokens) * top_k > kMoeMaxPairs) return SWL_ERR_UNSUPPORTED;
    return SWL_OK;
}

} // namespace swl

extern "C" int swl_moe_supported(int32_t hidden, int32_t inter, int32_t num_experts, int32_t top_k, int32_t dtype) {
    if (!swl::moe_dtype_ok(dtype)) return 0;
    if (hidden <= 0 || inter <= 0 || hidden % 64 != 0 || inter % 32 != 0) return 0;
    if (hidden / 16 > 65535 || inter / 16 > 65535) return 0;
    if (num_experts <= 0 || num_experts > swl::kMoeMaxExperts) return 0;
    if (top_k <= 0 || top_k > swl::kMoeMaxTopK || top_k > num_experts) return 0;
    return 1;
}

extern "C" int swl_moe_max_pairs(void) { return swl::kMoeMaxPairs; }

extern "C" int swl_moe_max_tiles(int32_t num_tokens, int32_t top_k, int32_t num_experts) {
    if (swl::moe_step_check(num_tokens, top_k, num_experts) != SWL_OK) return 0;
    return swl::moe_tile_bound(num_tokens * top_k, num_experts);
}

extern "C" int swl_moe_route(int32_t *topk_ids, float *topk_w, const void *logits, int32_t num_tokens, int32_t num_experts,
                             int32_t top_k, int32_t norm_topk_prob, int64_t logits_row_stride, int32_t logits_dtype,
                             swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (logits_row_stride < num_experts) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(logits_dtype) && logits_dtype != swl::kMoeLogitsF32) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0) return SWL_OK;
    if (!topk_ids || !topk_w || !logits) return SWL_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>((num_tokens + 3) / 4));
#define SWL_MOE_ROUTE(L)                                                                                                   \
    hipLaunchKernelGGL((swl::moe_route_kernel<L>), grid, dim3(256), 0, s, topk_ids, topk_w, static_cast<const L *>(logits), \
                       num_tokens, num_experts, top_k, norm_topk_prob != 0, logits_row_stride)
    if (logits_dtype == swl::kMoeLogitsF32) SWL_MOE_ROUTE(float);
    else if (logits_dtype == SWL_F16) SWL_MOE_ROUTE(swl::f16);
    else SWL_MOE_ROUTE(swl::bf16);
#undef SWL_MOE_ROUTE
    return swl::check_launch();
}

extern "C" int swl_moe_align(int32_t *tile_rows, int32_t *tile_experts, const int32_t *topk_ids, int32_t num_tokens,
                             int32_t top_k, int32_t num_experts, int32_t max_tiles, swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (max_tiles < swl::moe_tile_bound(num_tokens * top_k, num_experts)) return SWL_ERR_BAD_ARG;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0) return SWL_OK;
    if (!tile_rows || !tile_experts || !topk_ids) return SWL_ERR_BAD_ARG;
    hipLaunchKernelGGL(swl::moe_align_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), tile_rows,
                       tile_experts, topk_ids, num_tokens * top_k, num_experts, max_tiles);
    return swl::check_launch();
}

extern "C" int swl_moe_up_gate_silu(void *act, const void *x, const void *expert_up_gate, const int32_t *tile_rows,
                                    const int32_t *tile_experts, int32_t max_tiles, int32_t num_tokens, int32_t top_k,
                                    int32_t hidden, int32_t inter, int32_t num_experts, int64_t x_row_stride, int32_t dtype,
                                    swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0 || x_row_stride < hidden) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_supported(hidden, inter, num_experts, top_k, dtype) || x_row_stride % 8 != 0) return SWL_ERR_UNSUPPORTED;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!act || !x || !expert_up_gate || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(x) || !swl::aligned16(expert_up_gate)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>(max_tiles), static_cast<unsigned>(inter / 16));
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::moe_up_gate_silu_kernel<T>), grid, dim3(64 * swl::kMoeWaves), 0,
                           static_cast<hipStream_t>(stream), static_cast<T *>(act), static_cast<const T *>(x),
                           static_cast<const T *>(expert_up_gate), tile_rows, tile_experts, num_tokens * top_k, top_k, hidden,
                           inter, num_experts, x_row_stride);
    });
    return swl::check_launch();
}

extern "C" int swl_moe_down(float *y, const void *act, const void *expert_down, const int32_t *tile_rows,
                            const int32_t *tile_experts, int32_t max_tiles, int32_t num_tokens, int32_t top_k, int32_t hidden,
                            int32_t inter, int32_t num_experts, int32_t dtype, swl_stream_t stream) {
    const int rc = swl::moe_step_check(num_tokens, top_k, num_experts);
    if (rc != SWL_OK) return rc;
    if (hidden <= 0 || inter <= 0 || max_tiles < 0) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (!swl_moe_supported(hidden, inter, num_experts, top_k, dtype)) return SWL_ERR_UNSUPPORTED;
    if (max_tiles > 2 * swl::kMoeMaxPairs) return SWL_ERR_BAD_ARG;
    if (num_tokens == 0 || max_tiles == 0) return SWL_OK;
    if (!y || !act || !expert_down || !tile_rows || !tile_experts) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(act) || !swl::aligned16(expert_down)) return SWL_ERR_BAD_ARG;
    const dim3 grid(static_cast<unsigned>(max_tiles), static_cast<unsigned>(hidden / 16));
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::moe_down_kernel<T>), grid, dim3(64 * swl::kMoeWaves), 0, static_cast<hipStream_t>(stream), y,
                           static_cast<const T *>(act), static_cast<const T *>(expert_down), tile_rows, tile_experts,
                           num_tokens * top_k, hidden, inter, num_experts);
    });
    return swl::check_launch();
}

extern "C" int swl_moe_combine(void *out, const float *y, const float *topk_w, int32_t num_tokens, int32_t top_k,
                               int32_t hidden, int64_t out_row_stride, int32_t dtype, swl_stream_t stream) {
    if (num_tokens < 0 || top_k <= 0 || hidden <= 0 || out_row_stride < hidden) return SWL_ERR_BAD_ARG;
    if (!swl::moe_dtype_ok(dtype)) return SWL_ERR_BAD_ARG;
    if (top_k > swl::kMoeMaxTopK || hidden % 8 != 0 || out_row_stride % 8 != 0) return SWL_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(num_tokens) * top_k > swl::kMoeMaxPairs) return SWL_ERR_UNSUPPORTED;
    if (num_tokens == 0) return SWL_OK;
    if (!out || !y || !topk_w) return SWL_ERR_BAD_ARG;
    if (!swl::aligned16(out) || !swl::aligned16(y)) return SWL_ERR_BAD_ARG;
    const int64_t items = static_cast<int64_t>(num_tokens) * (hidden / 8);
    const int64_t blocks = (items + 255) / 256;
    const unsigned grid = static_cast<unsigned>(blocks < 16384 ? blocks : 16384);
    SWL_DISPATCH_DTYPE(dtype, T, {
        hipLaunchKernelGGL((swl::moe_combine_kernel<T>), dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<T *>(out), y, topk_w, items, top_k, hidden, out_row_stride);
    });
    return swl::check_launch();
}
