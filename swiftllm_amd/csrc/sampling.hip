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
#include "logits_keys.h"

namespace swl {

constexpr float kGumbelReach = 19.5f;   // > max G - min G = 16.64 + 2.82

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
