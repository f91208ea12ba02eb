// guided.hip — guided decoding: per-state token bitmasks over the vocabulary, built on the device and applied to the logits.
//
// The reference only takes the argmax of the raw logits (swiftllm/worker/layers/post_layer.py:40); this is an addition.
// A guide is a byte-level DFA (host: swiftllm_amd/guided/regex.py): trans[S, 256] int32, -1 = dead, and accepting[S]. Its
// masks are S rows of one pool masks[rows, W] int32: bit (t & 31) of word (t >> 5) of row row_base + s is set when token t
// may be picked in state s.
//
// swl_guide_build_masks. For every state s < num_states and token t < vocab, with the token's bytes
// tok_bytes[tok_offsets[t] .. tok_offsets[t + 1]):
//     t is an end id                         bit = accepting[s]
//     otherwise, the token has no byte       bit = 0
//     otherwise                              bit = the walk st = s; st = trans[st][byte] over its bytes never meets a dead
//                                                  entry (a value outside [0, num_states) counts as dead: nothing is read
//                                                  outside trans)
// Bits [vocab, 32 * W) are 0. One lane owns one token and keeps its first 8 bytes in registers across the loop over the
// states; the 64 lanes of a wave own 64 consecutive tokens, and the wave's ballot is the row's two mask words, stored by
// lanes 0 and 1 with ordinary 4-byte stores. Every word of rows [row_base, row_base + num_states) is written, whatever the
// pool held; no word outside them is. No atomics: two builds agree bit for bit. Grid: x = groups of 256 tokens, y = up to
// 64 state lanes (state s is served by block y = s mod gridDim.y).
//
// swl_logits_mask. Row r of x[num_rows, n] with k = row_index[r]: k < 0 or k >= num_mask_rows returns on the row's first
// instructions and leaves the row untouched; otherwise every element whose bit in mask row k is clear becomes -inf (0xfc00 /
// 0xff80), whatever it held, NaN included, and every element whose bit is set keeps its bits. One 1024-thread workgroup per
// row. VEC (base 16-byte aligned and row_stride % 8 == 0): one 16-byte vector per 8 bits of the mask; a vector whose 8 bits
// are all set is not even read, and only vectors in which something changed are written back. The tail [8 * (n >> 3), n) and
// the other path use 2-byte accesses. No reduction, no atomics: two launches agree bit for bit.
#include "swl_common.h"
#include "logits_bits.h"

namespace swl {

constexpr int kGuideBuildThreads = 256;
constexpr int kGuideBuildStateLanes = 64;
constexpr int kMaskThreads = 1024;

__global__ __launch_bounds__(kGuideBuildThreads) void guide_build_masks_kernel(
    int32_t *__restrict__ masks, int64_t row_base, int num_states, int words_per_row, const int32_t *__restrict__ trans,
    const uint8_t *__restrict__ accepting, const uint8_t *__restrict__ tok_bytes, const int32_t *__restrict__ tok_offsets,
    int vocab, const int32_t *__restrict__ end_ids, int num_end_ids) {
    const int t = blockIdx.x * kGuideBuildThreads + threadIdx.x;     // (< 32 * words_per_row + 256: the host checked int32)
    const int lane = threadIdx.x & (kWave - 1);
    const int word0 = (t - lane) >> 5;          // the wave's first mask word; uniform over the wave
    if (word0 >= words_per_row) return;         // (a whole wave past the row: uniform exit)

    bool is_end = false;
    int len = 0;
    int64_t off = 0;
    uint64_t head = 0;                          // the token's first 8 bytes, byte i in bits [8i, 8i + 8)
    if (t < vocab) {
        for (int e = 0; e < num_end_ids; ++e) is_end |= end_ids[e] == t;
        off = tok_offsets[t];
        len = tok_offsets[t + 1] - tok_offsets[t];
        if (len < 0) len = 0;
        const int pre = len < 8 ? len : 8;
        for (int i = 0; i < pre; ++i) head |= static_cast<uint64_t>(tok_bytes[off + i]) << (8 * i);
    }
    const uint32_t ns = static_cast<uint32_t>(num_states);
    for (int s = blockIdx.y; s < num_states; s += gridDim.y) {
        bool bit = false;
        if (t < vocab) {
            if (is_end) {
                bit = accepting[s] != 0;
            } else if (len > 0) {
                int st = s;
                int i = 0;
                for (; i < len; ++i) {
                    const uint32_t b = i < 8 ? static_cast<uint32_t>(head >> (8 * i)) & 0xffu : tok_bytes[off + i];
                    st = trans[static_cast<int64_t>(st) * 256 + b];
                    if (static_cast<uint32_t>(st) >= ns) break;
                }
                bit = i == len;
            }
        }
        const uint64_t ballot = __ballot(bit);
        if (lane < 2 && word0 + lane < words_per_row)
            masks[(row_base + s) * words_per_row + word0 + lane] =
                static_cast<int32_t>(static_cast<uint32_t>(lane ? ballot >> 32 : ballot));
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kMaskThreads) void logits_mask_kernel(uint16_t *x, int n, int64_t row_stride,
                                                                   const int32_t *__restrict__ masks, int num_mask_rows,
                                                                   int words_per_row,
                                                                   const int32_t *__restrict__ row_index) {
    const int row = blockIdx.x;
    const int tid = threadIdx.x;
    const int k = row_index[row];
    if (k < 0 || k >= num_mask_rows) return;
    uint16_t *xr = x + row * row_stride;
    const uint32_t *mr = reinterpret_cast<const uint32_t *>(masks) + static_cast<int64_t>(k) * words_per_row;
    constexpr uint16_t kNegInf = neg_inf_bits<T>();
    int tail = 0;
    if constexpr (VEC) {
        const int nvec = n >> 3;        // whole 8-element vectors: vector v is byte (v & 3) of mask word v >> 2
        for (int v = tid; v < nvec; v += kMaskThreads) {
            const uint32_t m8 = (mr[v >> 2] >> ((v & 3) * 8)) & 0xffu;
            if (m8 == 0xffu) continue;
            bits8_t b = *reinterpret_cast<const bits8_t *>(xr + v * 8);
            bool changed = false;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (!((m8 >> e) & 1u) && b[e] != kNegInf) {
                    b[e] = kNegInf;
                    changed = true;
                }
            }
            if (changed) *reinterpret_cast<bits8_t *>(xr + v * 8) = b;
        }
        tail = nvec * 8;
    }
    for (int i = tail + tid; i < n; i += kMaskThreads)
        if (!((mr[i >> 5] >> (i & 31)) & 1u) && xr[i] != kNegInf) xr[i] = kNegInf;
}

} // namespace swl

extern "C" int swl_guide_build_masks(int32_t *masks, int64_t row_base, int64_t num_states, int32_t words_per_row,
                                     const int32_t *trans, const uint8_t *accepting, const uint8_t *tok_bytes,
                                     const int32_t *tok_offsets, int32_t vocab, const int32_t *end_ids,
                                     int32_t num_end_ids, swl_stream_t stream) {
    if (row_base < 0 || num_states < 0 || words_per_row <= 0 || vocab <= 0 || num_end_ids < 0) return SWL_ERR_BAD_ARG;
    if (words_per_row < (static_cast<int64_t>(vocab) + 31) / 32) return SWL_ERR_BAD_ARG;
    if (num_states == 0) return SWL_OK;
    if (!masks || !trans || !accepting || !tok_bytes || !tok_offsets || (num_end_ids > 0 && !end_ids))
        return SWL_ERR_BAD_ARG;
    // int32 inside the kernel: a state's trans row index, a mask row, and a token index of the padded grid
    if (num_states > (0x7fffffff >> 8) || row_base + num_states > 0x7fffffff || words_per_row > (0x7fffffff >> 5) - 8)
        return SWL_ERR_UNSUPPORTED;
    const int64_t bits = static_cast<int64_t>(words_per_row) * 32;
    const unsigned gx = static_cast<unsigned>((bits + swl::kGuideBuildThreads - 1) / swl::kGuideBuildThreads);
    const unsigned gy = static_cast<unsigned>(num_states < swl::kGuideBuildStateLanes ? num_states
                                                                                       : swl::kGuideBuildStateLanes);
    hipLaunchKernelGGL(swl::guide_build_masks_kernel, dim3(gx, gy), dim3(swl::kGuideBuildThreads), 0,
                       static_cast<hipStream_t>(stream), masks, row_base, static_cast<int>(num_states), words_per_row,
                       trans, accepting, tok_bytes, tok_offsets, vocab, end_ids, num_end_ids);
    return swl::check_launch();
}

extern "C" int swl_logits_mask(void *logits, int64_t num_rows, int32_t n, int64_t row_stride, int32_t dtype,
                               const int32_t *masks, int64_t num_mask_rows, int32_t words_per_row,
                               const int32_t *row_index, swl_stream_t stream) {
    if (num_rows < 0 || n <= 0 || row_stride < n) return SWL_ERR_BAD_ARG;
    if (dtype != SWL_F16 && dtype != SWL_BF16) return SWL_ERR_BAD_ARG;
    if (num_mask_rows < 0 || words_per_row <= 0 || static_cast<int64_t>(words_per_row) * 32 < n) return SWL_ERR_BAD_ARG;
    if (num_rows == 0) return SWL_OK;
    if (!logits || !masks || !row_index) return SWL_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(logits) & 1u) return SWL_ERR_BAD_ARG;
    if (num_rows > 0x7fffffff || num_mask_rows > 0x7fffffff) return SWL_ERR_UNSUPPORTED;
    const bool vec = swl::aligned16(logits) && (row_stride & 7) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto *x = static_cast<uint16_t *>(logits);
    const int mask_rows = static_cast<int>(num_mask_rows);
    const dim3 grid(static_cast<unsigned>(num_rows)), block(swl::kMaskThreads);
    SWL_DISPATCH_DTYPE(dtype, T, {
        if (vec)
            hipLaunchKernelGGL((swl::logits_mask_kernel<T, true>), grid, block, 0, s, x, n, row_stride, masks, mask_rows,
                               words_per_row, row_index);
        else
            hipLaunchKernelGGL((swl::logits_mask_kernel<T, false>), grid, block, 0, s, x, n, row_stride, masks, mask_rows,
                               words_per_row, row_index);
    });
    return swl::check_launch();
}
