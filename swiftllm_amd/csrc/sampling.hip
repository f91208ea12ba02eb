// sampling.hip — seeded temperature / top-k / top-p sampling of the logits, one token per row.
//
// The reference only samples greedily (`torch.argmax(logits, dim=1)`, swiftllm/worker/layers/post_layer.py:40);
// this is an addition next to argmax.hip. Per row r (f_i = float(x_i), n = row width, pos = pos[r]):
//   T == 0 (or not > 0): exactly swl_argmax — lowest index among equal maxima, NaN never selected, 0 when nothing
//     compares. A row whose maximum is +inf also takes that branch (the softmax limit puts all mass there).
//   T > 0: m = max f; s_i = (f_i - m) / T and w_i = exp(s_i) in fp32.
//     top-k (1 <= k < n): keep f_i >= t_k, t_k = the k-th largest f counted with multiplicity (ties kept);
//     top-p (0 < p < 1), on what top-k kept: keep f_i >= t_p, t_p = the largest kept v with
//       sum_{kept, f_j >= v} w_j >= p * sum_{kept} w_j (ties kept).
//     Both thresholds are found by bisection over the order key of the stored 16-bit values (for T > 0 the order of
//     s), so top-k is exact. The token is the Gumbel-max draw argmax_{kept i} s_i + G_i (ties -> lowest i),
//     G_i = -logf(-logf(u_i)), u_i = (word >> 9) * 2^-23 + 2^-24 (exact in fp32, strictly inside (0, 1)), word =
//     word i & 3 of Philox4x32-10 with key (seed_lo, seed_hi) and counter (i >> 2, pos, 0, 0). The stream is a
//     function of (seed, pos, i) only: not of the row, the batch, the graph bucket or the step.
//
// One 1024-thread workgroup per row. The row is loaded once into registers as 16-bit order keys (16 vectors of 8
// per thread = 131072 elements; a wider row re-reads the rest from L2 on every pass). Every reduction that decides
// a token is a fixed-order wave butterfly + a fixed-order sum over the 16 waves: no atomics, so two launches on the
// same input agree bit for bit. Elements with s_i < -kGumbelReach can never win the draw (G lies in
// [-2.82, 16.64]) and draw no noise.
#include "swl_common.h"

namespace swl {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / kWave;
constexpr int kSampleSlots = 16;        // 8-element vectors per thread held in registers
constexpr float kGumbelReach = 19.5f;   // > max G - min G = 16.64 + 2.82

// 8 order keys packed two per dword (element 2d in the low half of dword d): 4 VGPRs per vector held
typedef uint32_t key8_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t key_at(const key8_t &k, int e) { return (k[e >> 1] >> ((e & 1) * 16)) & 0xffffu; }

__device__ __forceinline__ void philox4x32_10(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        // (one 32 x 32 -> 64-bit product per multiplier: v_mad_u64_u32 instead of a mul_lo + mul_hi pair)
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
        const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        c0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
        c1 = static_cast<uint32_t>(p1);
        c2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c3 = static_cast<uint32_t>(p0);
    }
}

// Order key of a 16-bit float: monotone in the value for everything but NaN (key 0, never kept); -0 maps to +0.
template <typename T>
__device__ __forceinline__ uint32_t order_key(uint32_t b) {
    const bool nan = std::is_same<T, f16>::value ? ((b & 0x7c00u) == 0x7c00u && (b & 0x03ffu))
                                                 : ((b & 0x7f80u) == 0x7f80u && (b & 0x007fu));
    if (nan) return 0;
    if (b == 0x8000u) b = 0;
    return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

template <typename T>
__device__ __forceinline__ float key_value(uint32_t k) {
    const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
    if constexpr (std::is_same<T, f16>::value)
        return static_cast<float>(__builtin_bit_cast(f16, static_cast<uint16_t>(b)));
    else
        return __uint_as_float(b << 16);
}

__device__ __forceinline__ void sample_merge(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

// Fixed-order workgroup reductions; `red_*` hold one value per wave. Every thread returns the total.
__device__ __forceinline__ int block_sum(int v, int *red) {
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) v += __shfl_xor(v, mask, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) t += red[w];
    __syncthreads();
    return t;
}

__device__ __forceinline__ float block_sum(float v, float *red) {
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) v += __shfl_xor(v, mask, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) t += red[w];
    __syncthreads();
    return t;
}

__device__ __forceinline__ void block_argmax(float &v, int &i, float *redv, int *redi) {
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) sample_merge(v, i, __shfl_xor(v, mask, 64), __shfl_xor(i, mask, 64));
    if ((threadIdx.x & 63) == 0) {
        redv[threadIdx.x >> 6] = v;
        redi[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    v = redv[0];
    i = redi[0];
#pragma unroll
    for (int w = 1; w < kSampleWaves; ++w) sample_merge(v, i, redv[w], redi[w]);
    __syncthreads();
}

// f(0), f(1), ... f(N - 1) with compile-time arguments (register arrays must never be indexed at run time)
template <int J, int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (J < N) {
        f(std::integral_constant<int, J>{});
        static_for<J + 1, N>(f);
    }
}

// Keys of the 8 elements of vector v (elements 8v .. 8v+7); past the row end: key 0. VEC: 16-byte loads are legal.
template <typename T, bool VEC>
__device__ __forceinline__ key8_t load_keys(const uint16_t *__restrict__ xr, int v, int n) {
    key8_t k;
    const int e0 = v * 8;
    if (VEC && e0 + 8 <= n) {
        const key8_t b = *reinterpret_cast<const key8_t *>(xr + e0);
#pragma unroll
        for (int d = 0; d < 4; ++d) k[d] = order_key<T>(b[d] & 0xffffu) | (order_key<T>(b[d] >> 16) << 16);
    } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t lo = e0 + 2 * d < n ? order_key<T>(xr[e0 + 2 * d]) : 0;
            const uint32_t hi = e0 + 2 * d + 1 < n ? order_key<T>(xr[e0 + 2 * d + 1]) : 0;
            k[d] = lo | (hi << 16);
        }
    }
    return k;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(
    int64_t *__restrict__ out, const uint16_t *__restrict__ x, int n, int64_t row_stride,
    const float *__restrict__ temperature, const int32_t *__restrict__ top_k, const float *__restrict__ top_p,
    const uint32_t *__restrict__ seed, const int32_t *__restrict__ pos) {
    __shared__ float redv[kSampleWaves];
    __shared__ int redi[kSampleWaves];
    const int row = blockIdx.x;
    const int tid = threadIdx.x;
    const uint16_t *xr = x + row * row_stride;
    const int nvec = (n + 7) >> 3;

    // visit(f): f(keys of one vector, its first element index) over this thread's vectors, in ascending index order
    key8_t held[kSampleSlots];
#pragma unroll
    for (int j = 0; j < kSampleSlots; ++j) {
        const int v = j * kSampleThreads + tid;
        held[j] = v < nvec ? load_keys<T, VEC>(xr, v, n) : key8_t(0);
    }
    // (the empty asm makes the held keys opaque on every pass: otherwise the compiler hoists the unpacked 16-bit keys
    // out of the bisection loops — 128 live VGPRs more — and spills)
    auto visit = [&](auto &&f) {
        static_for<0, kSampleSlots>([&](auto j) {
            key8_t k = held[j];
            asm volatile("" : "+v"(k));
            f(k, (j * kSampleThreads + tid) * 8);
        });
        for (int v = kSampleSlots * kSampleThreads + tid; v < nvec; v += kSampleThreads)
            f(load_keys<T, VEC>(xr, v, n), v * 8);
    };

    // pass 1: max / greedy argmax (strict '>' in ascending order keeps the lowest index among equals)
    float m = -INFINITY;
    int am = 0x7fffffff;
    visit([&](const key8_t &k, int e0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = key_value<T>(key_at(k, e));
            if (f > m) {
                m = f;
                am = e0 + e;
            }
        }
    });
    block_argmax(m, am, redv, redi);
    const float temp = temperature[row];
    if (!(temp > 0.0f) || am == 0x7fffffff || m == INFINITY) {
        if (tid == 0) out[row] = am == 0x7fffffff ? 0 : am;
        return;
    }
    const uint32_t kmax = order_key<T>(__builtin_bit_cast(uint16_t, to_t<T>(m)));

    // top-k: the largest key K with count(key >= K) >= k
    uint32_t thr = 1;
    const int k_top = top_k[row];
    if (k_top >= 1 && k_top < n) {
        uint32_t lo = 1, hi = kmax + 1;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            int c = 0;
            visit([&](const key8_t &k, int) {
#pragma unroll
                for (int e = 0; e < 8; ++e) c += key_at(k, e) >= mid;
            });
            if (block_sum(c, redi) >= k_top)
                lo = mid;
            else
                hi = mid;
        }
        thr = lo;
    }

    // top-p: the largest kept key K with mass(key >= K) >= p * mass(kept); the mass above `hi` is carried, so a round
    // only exponentiates the elements inside [mid, hi)
    const float p_top = top_p[row];
    if (p_top > 0.0f && p_top < 1.0f) {
        // (the weights only place t_p, so they are taken as v_exp_f32((f - m) * log2(e) / T): a relative error of
        // ~1e-7 per weight instead of an IEEE division and a full-precision expf per element per round)
        const float l2e_t = 1.4426950408889634f / temp;
        auto mass = [&](uint32_t a, uint32_t b) {
            float s = 0.0f;
            visit([&](const key8_t &k, int) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t ke = key_at(k, e);
                    if (ke >= a && ke < b) s += __builtin_amdgcn_exp2f((key_value<T>(ke) - m) * l2e_t);
                }
            });
            return block_sum(s, redv);
        };
        const float goal = p_top * mass(thr, 0x10000u);
        uint32_t lo = thr, hi = kmax + 1;
        float above = 0.0f;     // mass(key >= hi)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            const float tot = above + mass(mid, hi);
            if (tot >= goal) {
                lo = mid;
            } else {
                hi = mid;
                above = tot;
            }
        }
        thr = lo;
    }

    // Gumbel-max draw over the kept elements
    const uint32_t s_lo = seed[2 * row], s_hi = seed[2 * row + 1];
    const uint32_t p_row = static_cast<uint32_t>(pos[row]);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    visit([&](const key8_t &k, int e0) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float s[4];
            bool live = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t kk = key_at(k, g * 4 + e);
                s[e] = kk >= thr ? (key_value<T>(kk) - m) / temp : -INFINITY;
                live |= s[e] >= -kGumbelReach;
            }
            if (!live) continue;
            uint32_t w[4] = {static_cast<uint32_t>((e0 >> 2) + g), p_row, 0u, 0u};
            philox4x32_10(w[0], w[1], w[2], w[3], s_lo, s_hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!(s[e] >= -kGumbelReach)) continue;
                const float u = static_cast<float>(w[e] >> 9) * 0x1p-23f + 0x1p-24f;
                const float score = s[e] - logf(-logf(u));
                if (score > best) {
                    best = score;
                    bi = e0 + g * 4 + e;
                }
            }
        }
    });
    block_argmax(best, bi, redv, redi);
    if (tid == 0) out[row] = bi == 0x7fffffff ? am : bi;
}

} // namespace swl

extern "C" int swl_sample(int64_t *out, const void *logits, int64_t num_rows, int32_t n, int64_t row_stride,
                          int32_t dtype, const float *temperature, const int32_t *top_k, const float *top_p,
                          const uint32_t *seed, const int32_t *pos, swl_stream_t stream) {
    if (num_rows < 0 || n <= 0 || row_stride < n) return SWL_ERR_BAD_ARG;
    if (dtype != SWL_F16 && dtype != SWL_BF16) return SWL_ERR_BAD_ARG;
    if (num_rows == 0) return SWL_OK;
    if (!out || !logits || !temperature || !top_k || !top_p || !seed || !pos) return SWL_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(logits) & 1u) return SWL_ERR_BAD_ARG;
    if (num_rows > 0x7fffffff) return SWL_ERR_UNSUPPORTED;
    const bool vec = swl::aligned16(logits) && (row_stride & 7) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto *x = static_cast<const uint16_t *>(logits);
    const dim3 grid(static_cast<unsigned>(num_rows)), block(swl::kSampleThreads);
    SWL_DISPATCH_DTYPE(dtype, T, {
        if (vec)
            hipLaunchKernelGGL((swl::sample_kernel<T, true>), grid, block, 0, s, out, x, n, row_stride, temperature,
                               top_k, top_p, seed, pos);
        else
            hipLaunchKernelGGL((swl::sample_kernel<T, false>), grid, block, 0, s, out, x, n, row_stride, temperature,
                               top_k, top_p, seed, pos);
    });
    return swl::check_launch();
}
