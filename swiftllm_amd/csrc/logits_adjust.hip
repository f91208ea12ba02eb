// logits_adjust.hip — penalties, logit bias and min-p on the logits, in place, before swl_argmax / swl_sample read them.
//
// The reference only takes the argmax of the raw logits (swiftllm/worker/layers/post_layer.py:40); this is an addition.
// Row r of x[num_rows, n] owns the entries e in [edit_offsets[r], edit_offsets[r + 1]) of three parallel arrays (one
// entry per token id, the host guarantees it) and four fp32 parameters: rep, pres, freq, gap = row_params[r][0..3].
//
// Phase 1, sparse, one lane per entry; id = edit_ids[e], count = edit_meta[e] & 0x7fffffff (occurrences among the
// sequence's output tokens), in_prompt = edit_meta[e] < 0 (bit 31), bias = edit_bias[e]. Every step is ONE IEEE fp32
// operation (the library is built with -ffp-contract=off: the product and the subtraction below stay two roundings):
//     f = float(x[id])
//     if ((count > 0 || in_prompt) && rep != 1)  f = f > 0 ? f / rep : f * rep
//     f = f - freq * float(count)
//     if (count > 0)  f = f - pres
//     f = f + bias
//     x[id] = T(f)        round to nearest even
// NaN stays NaN; an id outside [0, n) is skipped; the store is a 2-byte store (ids 2k and 2k + 1 share a dword and
// belong to different lanes).
//
// Phase 2, dense, only when gap > -inf (min-p; gap = fp32(T * ln(min_p)) is computed by the host in double precision,
// no logarithm here decides what is kept): after a workgroup barrier, m = the row maximum over the non-NaN values, then
// every element with float(x_i) - m < gap becomes -inf. NaN elements compare false and are left alone, so a row without
// a non-NaN element is left as it is. The kept set is {i : p_i >= min_p * p_max} of softmax(x / T).
//
// One 1024-thread workgroup per row; a row with no entries and gap == -inf returns on its first instructions. The
// maximum is a fixed-order wave butterfly + a fixed-order pass over the 16 waves (and a maximum does not depend on
// the order anyway): no atomics, two launches on the same input agree bit for bit. VEC: 16-byte accesses (base 16-byte
// aligned and row_stride % 8 == 0); otherwise 2-byte accesses. The row is read twice in phase 2; the second read comes
// from L2 (256 KB per row at n = 128256).
//
// An element that is -inf when the kernel starts (a token the guide mask of csrc/guided.hip removed) is -inf when it ends:
// every fp32 step above maps -inf to -inf (rep is finite and > 0, freq * count and pres are finite, bias is finite or
// -inf), T(-inf) is -inf, and in phase 2 -inf - m < gap holds for any finite m.
#include "swl_common.h"
#include "logits_bits.h"

namespace swl {

constexpr int kAdjustThreads = 1024;
constexpr int kAdjustWaves = kAdjustThreads / kWave;

template <typename T, bool VEC>
__global__ __launch_bounds__(kAdjustThreads) void logits_adjust_kernel(
    uint16_t *x, int n, int64_t row_stride, const int32_t *__restrict__ edit_offsets,
    const int32_t *__restrict__ edit_ids, const int32_t *__restrict__ edit_meta, const float *__restrict__ edit_bias,
    const float *__restrict__ row_params) {
    __shared__ float red[kAdjustWaves];
    const int row = blockIdx.x;
    const int tid = threadIdx.x;
    const int e_begin = edit_offsets[row], e_end = edit_offsets[row + 1];
    const float gap = row_params[4 * row + 3];
    const bool dense = gap > -INFINITY;
    if (e_end <= e_begin && !dense) return;
    uint16_t *xr = x + row * row_stride;

    // ---- phase 1: one lane per entry ----
    if (e_end > e_begin) {
        const float rep = row_params[4 * row], pres = row_params[4 * row + 1], freq = row_params[4 * row + 2];
        for (int e = e_begin + tid; e < e_end; e += kAdjustThreads) {
            const int id = edit_ids[e];
            if (id < 0 || id >= n) continue;
            const int32_t meta = edit_meta[e];
            const int count = meta & 0x7fffffff;
            float f = bits_to_f<T>(xr[id]);
            if ((count > 0 || meta < 0) && rep != 1.0f) f = f > 0.0f ? f / rep : f * rep;
            f = f - freq * static_cast<float>(count);
            if (count > 0) f = f - pres;
            f = f + edit_bias[e];
            xr[id] = __builtin_bit_cast(uint16_t, to_t<T>(f));
        }
    }
    if (!dense) return;
    __syncthreads();    // (workgroup-scope fence: the 2-byte stores above are visible to every lane's loads below)

    // ---- phase 2: row maximum over the non-NaN values ('>' is false for NaN) ----
    const int nvec = n >> 3;            // whole 8-element vectors; the tail [8 * nvec, n) is scalar on both paths
    float m = -INFINITY;
    if constexpr (VEC) {
        for (int v = tid; v < nvec; v += kAdjustThreads) {
            const bits8_t b = *reinterpret_cast<const bits8_t *>(xr + v * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = bits_to_f<T>(b[e]);
                if (f > m) m = f;
            }
        }
        for (int i = nvec * 8 + tid; i < n; i += kAdjustThreads) {
            const float f = bits_to_f<T>(xr[i]);
            if (f > m) m = f;
        }
    } else {
        for (int i = tid; i < n; i += kAdjustThreads) {
            const float f = bits_to_f<T>(xr[i]);
            if (f > m) m = f;
        }
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
        const float o = __shfl_xor(m, mask, 64);
        if (o > m) m = o;
    }
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < kAdjustWaves; ++w)
        if (red[w] > m) m = red[w];

    // ---- mask: float(x_i) - m < gap -> -inf (NaN, and everything when m == -inf, compares false) ----
    constexpr uint16_t kNegInf = neg_inf_bits<T>();
    if constexpr (VEC) {
        for (int v = tid; v < nvec; v += kAdjustThreads) {
            bits8_t b = *reinterpret_cast<const bits8_t *>(xr + v * 8);
            bool changed = false;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (bits_to_f<T>(b[e]) - m < gap) {
                    b[e] = kNegInf;
                    changed = true;
                }
            }
            if (changed) *reinterpret_cast<bits8_t *>(xr + v * 8) = b;
        }
        for (int i = nvec * 8 + tid; i < n; i += kAdjustThreads)
            if (bits_to_f<T>(xr[i]) - m < gap) xr[i] = kNegInf;
    } else {
        for (int i = tid; i < n; i += kAdjustThreads)
            if (bits_to_f<T>(xr[i]) - m < gap) xr[i] = kNegInf;
    }
}

} // namespace swl

extern "C" int swl_logits_adjust(void *logits, int64_t num_rows, int32_t n, int64_t row_stride, int32_t dtype,
                                 const int32_t *edit_offsets, const int32_t *edit_ids, const int32_t *edit_meta,
                                 const float *edit_bias, const float *row_params, swl_stream_t stream) {
    if (num_rows < 0 || n <= 0 || row_stride < n) return SWL_ERR_BAD_ARG;
    if (dtype != SWL_F16 && dtype != SWL_BF16) return SWL_ERR_BAD_ARG;
    if (num_rows == 0) return SWL_OK;
    if (!logits || !edit_offsets || !edit_ids || !edit_meta || !edit_bias || !row_params) return SWL_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(logits) & 1u) return SWL_ERR_BAD_ARG;
    if (num_rows > 0x7fffffff) return SWL_ERR_UNSUPPORTED;
    const bool vec = swl::aligned16(logits) && (row_stride & 7) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto *x = static_cast<uint16_t *>(logits);
    const dim3 grid(static_cast<unsigned>(num_rows)), block(swl::kAdjustThreads);
    SWL_DISPATCH_DTYPE(dtype, T, {
        if (vec)
            hipLaunchKernelGGL((swl::logits_adjust_kernel<T, true>), grid, block, 0, s, x, n, row_stride, edit_offsets,
                               edit_ids, edit_meta, edit_bias, row_params);
        else
            hipLaunchKernelGGL((swl::logits_adjust_kernel<T, false>), grid, block, 0, s, x, n, row_stride, edit_offsets,
                               edit_ids, edit_meta, edit_bias, row_params);
    });
    return swl::check_launch();
}
