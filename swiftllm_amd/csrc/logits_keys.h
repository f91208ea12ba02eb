// logits_keys.h — what the kernels that walk a whole row of 16-bit logits with one 1024-thread workgroup share
// (sampling.hip, logprobs.hip): the order keys of the stored values, the register-resident row, and the fixed-order
// workgroup reductions.
#pragma once

#include "swl_common.h"

namespace swl {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / kWave;
constexpr int kSampleSlots = 16;        // 8-element vectors per thread held in registers

// 8 order keys packed two per dword (element 2d in the low half of dword d): 4 VGPRs per vector held
typedef uint32_t key8_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t key_at(const key8_t &k, int e) { return (k[e >> 1] >> ((e & 1) * 16)) & 0xffffu; }

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

} // namespace swl
