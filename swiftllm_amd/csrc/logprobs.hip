// logprobs.hip — log-probability and rank of the token a row picked, and the row's exact top-N alternatives.
//
// The reference returns token ids only (swiftllm/worker/layers/post_layer.py:40); this is an addition next to
// argmax.hip and sampling.hip. It reads the logits as they stand when the token is picked: after logits_adjust.hip
// (penalties, bias, min-p, banned stop tokens), before temperature / top-k / top-p. The distribution is the model's
// at temperature 1; a sampled row's filters do not renormalise it. Per asking row r (n = row width):
//   f_i = float(x_i); NaN elements are ignored; m = max f; lse = m + log(sum_i exp(f_i - m)) in fp32;
//   logprob(i) = f_i - lse.
//   Order: (value descending, id ascending), decided on the order keys of the stored 16-bit values (logits_keys.h):
//     -0 == +0, and NaN elements come last (among themselves by id). Ids and ranks are exact, ties included.
//   Chosen token c = chosen[r]: lp[r][0] = logprob(c), ids[r][0] = c, rank[r] = 1 + the number of elements before c in
//     that order (for a c that is not NaN: 1 + #{i : f_i > f_c, or f_i == f_c and i < c}).
//     c outside [0, n): lp[r][0] = NaN, ids[r][0] = -1, rank[r] = 0, and nothing is read outside the row.
//   Top-N, N = min(top_n[r], n_cap), 0 <= N <= 20: columns 1..N of lp / ids hold the first N elements of that order
//     with their logprobs; N = 0 reports the chosen token only. A row narrower than N fills columns n+1..N with
//     id -1 and NaN.
//   A row whose m is not finite (all -inf / NaN, or a +inf): ids and rank as above, every logprob NaN. An element
//     equal to -inf in a healthy row has logprob -inf.
//   top_n[r] < 0: the row does not ask; its workgroup exits at once and writes nothing. An asking row writes exactly
//     columns 0..min(top_n[r], n_cap) and rank[r].
//
// One 1024-thread workgroup per row; the row is loaded once into registers as order keys (16 vectors of 8 per thread =
// 131072 elements; a wider row re-reads the rest from L2 on every pass), as the sampler does. Passes: the maximum key;
// one pass for sum exp and the chosen token's rank; the N-th largest key by bisection over the 16-bit key space (the
// sampler's top-k); the elements above it are placed by a prefix sum over the threads, the lowest ids among those equal
// to it are taken one by one, and the <= 19 elements above are ordered in LDS. Every reduction is fixed-order:
// per-thread in slot order, a wave butterfly, the 16 waves in order. No atomics, so two launches agree bit for bit, and
// a row's outputs depend on nothing but the row, its chosen id and its own N (its first k entries not even on N).
//
// Error of a logprob against exact arithmetic: the sum takes at most n / 1024 rounded up to 8 (128 at n <= 131072)
// serial additions per thread, 6 butterfly and 16 wave additions, over terms from a <= 2-ulp expf: <= ~150 * 2^-24 =
// 9e-6 relative on the sum, which is absolute on its logarithm; m + log(sum) and f - lse round once each (2^-24 |lp|).
#include "logits_keys.h"

namespace swl {

constexpr int kLogprobMaxTop = 20;

// Fixed-order workgroup maximum; every thread returns it.
__device__ __forceinline__ uint32_t block_max(uint32_t v, int *red) {
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), mask, 64)));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = static_cast<int>(v);
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) t = max(t, static_cast<uint32_t>(red[w]));
    __syncthreads();
    return t;
}

// Sum of v over the threads before this one (thread order); `total`: over all of them.
__device__ __forceinline__ int block_exclusive_scan(int v, int *red, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) {
        if (w < wave) base += red[w];
        total += red[w];
    }
    __syncthreads();
    return base + inc - v;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kSampleThreads) void logprobs_kernel(
    float *__restrict__ lp, int32_t *__restrict__ ids, int32_t *__restrict__ rank, const uint16_t *__restrict__ x, int n,
    int64_t row_stride, const int64_t *__restrict__ chosen, const int32_t *__restrict__ top_n, int n_cap) {
    __shared__ float redv[kSampleWaves];
    __shared__ int redi[kSampleWaves];
    __shared__ uint32_t top_key[kLogprobMaxTop];
    __shared__ int top_id[kLogprobMaxTop];
    const int row = blockIdx.x;
    int want = top_n[row];
    if (want < 0) return;
    want = min(want, n_cap);
    const int tid = threadIdx.x;
    const uint16_t *xr = x + row * row_stride;
    float *lpr = lp + static_cast<int64_t>(row) * (n_cap + 1);
    int32_t *idr = ids + static_cast<int64_t>(row) * (n_cap + 1);
    const int nvec = (n + 7) >> 3;

    // visit(f): f(keys of one vector, its first element index) over this thread's vectors, in ascending index order
    key8_t held[kSampleSlots];
#pragma unroll
    for (int j = 0; j < kSampleSlots; ++j) {
        const int v = j * kSampleThreads + tid;
        held[j] = v < nvec ? load_keys<T, VEC>(xr, v, n) : key8_t(0);
    }
    // (the empty asm keeps the held keys packed across the passes, as in sampling.hip; the one on the thread index
    // keeps the 128 element ids of a pass from being computed once, ahead of the loops that run passes, and spilled)
    auto visit = [&](auto &&f) {
        int t = tid;
        asm volatile("" : "+v"(t));
        static_for<0, kSampleSlots>([&](auto j) {
            key8_t k = held[j];
            asm volatile("" : "+v"(k));
            f(k, (j * kSampleThreads + t) * 8);
        });
        for (int v = kSampleSlots * kSampleThreads + tid; v < nvec; v += kSampleThreads)
            f(load_keys<T, VEC>(xr, v, n), v * 8);
    };

    // pass 1: the maximum, from the keys (key 0: every element is NaN)
    uint32_t kmax = 0;
    visit([&](const key8_t &k, int) {
#pragma unroll
        for (int e = 0; e < 8; ++e) kmax = max(kmax, key_at(k, e));
    });
    kmax = block_max(kmax, redi);
    const float m = key_value<T>(kmax);
    const bool healthy = kmax != 0 && fabsf(m) < INFINITY;

    // pass 2: sum exp(f - m) over the elements that are not NaN, and the elements ahead of the chosen one
    const int64_t c64 = chosen[row];
    const bool c_ok = c64 >= 0 && c64 < n;
    const int c = c_ok ? static_cast<int>(c64) : -1;
    const uint32_t kc = c_ok ? order_key<T>(xr[c]) : 0xffffffffu;
    float s = 0.0f;
    int ahead = 0;
    visit([&](const key8_t &k, int e0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t ke = key_at(k, e);
            s += ke ? expf(key_value<T>(ke) - m) : 0.0f;
            ahead += ke > kc || (ke == kc && e0 + e < c);
        }
        // (one vector at a time: left alone, the scheduler starts all 128 exponentials of the unrolled pass at once
        // and spills several hundred registers)
        asm volatile("" : "+v"(s), "+v"(ahead));
    });
    s = block_sum(s, redv);
    ahead = block_sum(ahead, redi);
    const float lse = m + logf(s);
    auto logprob = [&](uint32_t ke) { return healthy ? key_value<T>(ke) - lse : __uint_as_float(0x7fc00000u); };
    if (tid == 0) {
        lpr[0] = c_ok ? logprob(kc) : __uint_as_float(0x7fc00000u);
        idr[0] = c;
        rank[row] = c_ok ? 1 + ahead : 0;
    }
    if (want == 0) return;

    // the N-th largest key: the largest K with count(key >= K) >= N. K = 0 holds by itself (the row has >= `take`
    // elements), and no round asks about it, so the key-0 padding past the row end is never counted.
    const int take = min(want, n);
    uint32_t lo = 0, hi = kmax + 1;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        int cnt = 0;
        visit([&](const key8_t &k, int) {
#pragma unroll
            for (int e = 0; e < 8; ++e) cnt += key_at(k, e) >= mid;
        });
        if (block_sum(cnt, redi) >= take)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t thr = lo;

    // everything above it (fewer than `take` elements): each thread places its own behind those of the threads before it
    int mine = 0;
    visit([&](const key8_t &k, int) {
#pragma unroll
        for (int e = 0; e < 8; ++e) mine += key_at(k, e) > thr;
    });
    int above;
    int at = block_exclusive_scan(mine, redi, above);
    if (mine > 0) {
        visit([&](const key8_t &k, int e0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t ke = key_at(k, e);
                if (ke > thr && at < kLogprobMaxTop) {
                    top_key[at] = ke;
                    top_id[at] = e0 + e;
                    ++at;
                }
            }
        });
    }
    __syncthreads();
    above = min(above, take - 1);
    // ... ordered by counting, in LDS: element t lands behind the elements that precede it
    if (tid < above) {
        const uint32_t kt = top_key[tid];
        const int it = top_id[tid];
        int p = 0;
        for (int j = 0; j < above; ++j) p += top_key[j] > kt || (top_key[j] == kt && top_id[j] < it);
        lpr[1 + p] = logprob(kt);
        idr[1 + p] = it;
    }

    // the rest are equal to it: the lowest ids, one per round (the padding past the row end has key 0 and ids >= n)
    const uint32_t thr2 = thr | (thr << 16);
    int last = -1;
    for (int q = above; q < take; ++q) {
        int best = n;
        visit([&](const key8_t &k, int e0) {
            bool any = false;       // (few vectors hold the key at all: one test per packed pair first)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t diff = k[d] ^ thr2;
                any |= (diff & 0xffffu) == 0 || (diff >> 16) == 0;
            }
            if (!any) return;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int id = e0 + e;
                if (key_at(k, e) == thr && id > last && id < best) best = id;
            }
        });
        best = 0x7fffffff - static_cast<int>(block_max(static_cast<uint32_t>(0x7fffffff - best), redi));
        if (best >= n) break;
        last = best;
        if (tid == 0) {
            lpr[1 + q] = logprob(thr);
            idr[1 + q] = best;
        }
    }
    // a row narrower than N
    if (tid == 0) {
        for (int q = take; q < want; ++q) {
            lpr[1 + q] = __uint_as_float(0x7fc00000u);
            idr[1 + q] = -1;
        }
    }
}

} // namespace swl

extern "C" int swl_logprobs(float *lp, int32_t *ids, int32_t *rank, const void *logits, int64_t num_rows, int32_t n,
                            int64_t row_stride, int32_t dtype, const int64_t *chosen, const int32_t *top_n,
                            int32_t n_cap, swl_stream_t stream) {
    if (num_rows < 0 || n <= 0 || row_stride < n) return SWL_ERR_BAD_ARG;
    if (dtype != SWL_F16 && dtype != SWL_BF16) return SWL_ERR_BAD_ARG;
    if (n_cap < 0 || n_cap > swl::kLogprobMaxTop) return SWL_ERR_BAD_ARG;
    if (num_rows == 0) return SWL_OK;
    if (!lp || !ids || !rank || !logits || !chosen || !top_n) return SWL_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(logits) & 1u) return SWL_ERR_BAD_ARG;
    if (num_rows > 0x7fffffff) return SWL_ERR_UNSUPPORTED;
    const bool vec = swl::aligned16(logits) && (row_stride & 7) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto *x = static_cast<const uint16_t *>(logits);
    const dim3 grid(static_cast<unsigned>(num_rows)), block(swl::kSampleThreads);
    SWL_DISPATCH_DTYPE(dtype, T, {
        if (vec)
            hipLaunchKernelGGL((swl::logprobs_kernel<T, true>), grid, block, 0, s, lp, ids, rank, x, n, row_stride, chosen,
                               top_n, n_cap);
        else
            hipLaunchKernelGGL((swl::logprobs_kernel<T, false>), grid, block, 0, s, lp, ids, rank, x, n, row_stride,
                               chosen, top_n, n_cap);
    });
    return swl::check_launch();
}
