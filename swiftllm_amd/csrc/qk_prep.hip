// qk_prep.hip — what sits between the q/k/v projections and the KV store for the model families that are not plain Llama:
// the projection bias (Qwen2 / Qwen2.5), the per-head RMSNorm of q and k (Qwen3) and the rotate-half rotary embedding, in
// ONE launch, in place. No reference counterpart (the reference serves Llama only); the arithmetic is the one
// HuggingFace's Qwen2Attention / Qwen3Attention + apply_rotary_pos_emb state, evaluated in fp32.
//
// Contract (swl_qk_prep_rotary), per token t of q[T, H, D], k[T, KVH, D], v[T, KVH, D] (token strides as in swl_rotary):
//   * table row = pos_idx ? pos_idx[t] : t. A negative row is an inert row of a padded hipGraph bucket: q, k and v of that
//     token keep their bits (as swl_rotary, rotary.hip).
//   * per (token, q head or k head), fp32 from the stored 16-bit values, nothing rounded in between:
//       1. f_i = float(x_i) + float(bias[h*D + i])                         (when the head's bias is given)
//       2. r = 1 / sqrt(sum_i f_i^2 / D + eps) ; f_i = f_i * r * float(w_i) (when the norm weights are given; the sum runs
//          in one fixed order: a lane's 16 elements in index order, then an xor butterfly over the head's lanes)
//       3. i < D/2: y_i = f_i*c_i - f_{i+D/2}*s_i ; y_{i+D/2} = f_{i+D/2}*c_i + f_i*s_i  (c, s: the tables' values as floats)
//       4. x_i = round-to-nearest-even(y_i)
//   * v_i = rne(float(v_i) + float(v_bias_i)) when v_bias is given; otherwise v is not touched and may be NULL.
//   * no scratch, no atomics, no allocation, capturable; a row's bits do not depend on the batch.
//   * head_dim in {32, 64, 128, 256}; alignment, stride and count checks are swl_rotary's (kv_store.h). q_norm_w without
//     k_norm_w (or the reverse) is SWL_ERR_BAD_ARG. Zero tokens: SWL_OK, nothing launched.
//
// HBM-bound like swl_rotary: 2*T*(H+KVH)*D*e bytes (+ 2*T*KVH*D*e for a biased v) + the cos/sin rows, biases and norm
// weights (L2 resident). Mapping: rotary_kernel's lane layout — a lane owns 8 consecutive elements of the first half of a
// head and the matching 8 of the second half (two 16-byte loads, two 16-byte stores) — so a head is a GROUP of D/16 = 2 /
// 4 / 8 / 16 adjacent lanes, and the sum of squares is reduced across the group by __shfl_xor. A v head is one more group
// of the same shape that carries the bias only. Groups stay whole: the item count is a multiple of the group size, the
// block and the grid stride are multiples of it, and token, head and the inert-row skip are the same for every lane of a
// group — a shuffle never addresses a lane that left the loop.
#include "kv_store.h"

namespace swl {

template <typename T>
struct QkPrepArgs {
    T *q, *k, *v;
    const T *q_bias, *k_bias, *v_bias;
    const T *q_norm_w, *k_norm_w;
    const T *cos_t, *sin_t;
    const int *pos_idx;
    int64_t num_items;
    int H, KVH, VH, D;          // VH: the v heads that are items (KVH with a v bias, else 0)
    int lg_chunks;              // log2(D / 16)
    int64_t q_tok_stride, k_tok_stride, v_tok_stride;
    float eps, inv_d;
};

// Work item = (token, head in [0, H + KVH + VH), chunk in [0, D/16)).
template <typename T, bool NORM, bool BIAS>
__global__ __launch_bounds__(256) void qk_prep_rotary_kernel(const QkPrepArgs<T> a) {
    const int chunks = 1 << a.lg_chunks;
    const int heads = a.H + a.KVH + a.VH;
    const int half = a.D >> 1;
    for (int64_t item = blockIdx.x * 256ll + threadIdx.x; item < a.num_items;
         item += static_cast<int64_t>(gridDim.x) * 256ll) {
        const int c = static_cast<int>(item & (chunks - 1));
        const int64_t th = item >> a.lg_chunks;
        const int hh = static_cast<int>(th % heads);
        const int64_t tok = th / heads;
        const int64_t row = a.pos_idx ? a.pos_idx[tok] : tok;
        if (row < 0) continue;  // an inert row of a padded decode batch: the whole group leaves together
        T *base;
        const T *bias;
        const T *norm_w = nullptr;
        if (hh < a.H) {
            base = a.q + tok * a.q_tok_stride + static_cast<int64_t>(hh) * a.D;
            bias = a.q_bias ? a.q_bias + static_cast<int64_t>(hh) * a.D : nullptr;
            norm_w = a.q_norm_w;
        } else if (hh < a.H + a.KVH) {
            base = a.k + tok * a.k_tok_stride + static_cast<int64_t>(hh - a.H) * a.D;
            bias = a.k_bias ? a.k_bias + static_cast<int64_t>(hh - a.H) * a.D : nullptr;
            norm_w = a.k_norm_w;
        } else {
            base = a.v + tok * a.v_tok_stride + static_cast<int64_t>(hh - a.H - a.KVH) * a.D;
            bias = a.v_bias + static_cast<int64_t>(hh - a.H - a.KVH) * a.D;
        }
        const bool is_v = hh >= a.H + a.KVH;
        vec8_t<T> x0 = load8(base + c * 8);
        vec8_t<T> x1 = load8(base + half + c * 8);
        if (BIAS && is_v) {     // v carries the bias only: one rounding from the fp32 sum
            const vec8_t<T> b0 = load8(bias + c * 8), b1 = load8(bias + half + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x0[j] = add_t<T>(x0[j], b0[j]);
                x1[j] = add_t<T>(x1[j], b1[j]);
            }
            store8(base + c * 8, x0);
            store8(base + half + c * 8, x1);
            continue;
        }
        const vec8_t<T> cv = load8(a.cos_t + row * half + c * 8);
        const vec8_t<T> sv = load8(a.sin_t + row * half + c * 8);
        float f0[8], f1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f0[j] = to_f(x0[j]), f1[j] = to_f(x1[j]);
        if (BIAS && bias) {
            const vec8_t<T> b0 = load8(bias + c * 8), b1 = load8(bias + half + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) f0[j] += to_f(b0[j]), f1[j] += to_f(b1[j]);
        }
        if (NORM) {
            const vec8_t<T> w0 = load8(norm_w + c * 8), w1 = load8(norm_w + half + c * 8);
            float ssq = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) ssq += f0[j] * f0[j];
#pragma unroll
            for (int j = 0; j < 8; ++j) ssq += f1[j] * f1[j];
            // the head's lanes are adjacent and all here (see the file header); a + b is commutative, so both sides of
            // every exchange hold the same bits and every lane ends with the same sum
            for (int m = 1; m < chunks; m <<= 1) ssq += __shfl_xor(ssq, m);
            const float r = 1.0f / sqrtf(ssq * a.inv_d + a.eps);
#pragma unroll
            for (int j = 0; j < 8; ++j) f0[j] = f0[j] * r * to_f(w0[j]), f1[j] = f1[j] * r * to_f(w1[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float cj = to_f(cv[j]), sj = to_f(sv[j]);
            x0[j] = to_t<T>(f0[j] * cj - f1[j] * sj);
            x1[j] = to_t<T>(f1[j] * cj + f0[j] * sj);
        }
        store8(base + c * 8, x0);
        store8(base + half + c * 8, x1);
    }
}

template <typename T, bool NORM, bool BIAS>
static void launch_qk_prep(const QkPrepArgs<T> &a, swl_stream_t stream) {
    const int64_t blocks = (a.num_items + 255) / 256;
    const unsigned grid = static_cast<unsigned>(blocks < 65536 ? blocks : 65536);
    hipLaunchKernelGGL((qk_prep_rotary_kernel<T, NORM, BIAS>), dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
}

} // namespace swl

using swl::KvStoreArgs;

extern "C" int swl_qk_prep_rotary(void *q, void *k, void *v, const void *q_bias, const void *k_bias, const void *v_bias,
    const void *q_norm_w, const void *k_norm_w, float eps, const void *cos_table, const void *sin_table,
    const int32_t *pos_idx, int64_t num_tokens, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
    int64_t q_tok_stride, int64_t k_tok_stride, int64_t v_tok_stride, int32_t dtype, swl_stream_t stream) {
    KvStoreArgs a;
    a.q = q, a.k = k, a.v = v, a.cos_table = cos_table, a.sin_table = sin_table, a.pos_idx = pos_idx;
    a.num_seqs = num_tokens, a.H = num_q_heads, a.g.KVH = num_kv_heads, a.g.D = head_dim;
    a.q_tok_stride = q_tok_stride, a.k_tok_stride = k_tok_stride, a.v_tok_stride = v_tok_stride;
    SWL_KV_CHECK(swl::check_kv_counts(a));
    if (a.empty()) return SWL_OK;
    SWL_KV_CHECK(swl::check_present({q, k, cos_table, sin_table}));
    SWL_KV_CHECK(swl::check_heads(a));
    SWL_KV_CHECK(swl::check_head_dim_rotary(a, SWL_ERR_BAD_ARG));
    if ((q_norm_w == nullptr) != (k_norm_w == nullptr)) return SWL_ERR_BAD_ARG;     // both or neither
    if (q_norm_w && !(eps >= 0.0f)) return SWL_ERR_BAD_ARG;
    SWL_KV_CHECK(swl::check_tok_stride(a, q_tok_stride, num_q_heads));
    SWL_KV_CHECK(swl::check_tok_stride(a, k_tok_stride, num_kv_heads));
    if (v_bias) {               // only a biased v is touched
        SWL_KV_CHECK(swl::check_present({v}));
        SWL_KV_CHECK(swl::check_tok_stride(a, v_tok_stride, num_kv_heads));
        SWL_KV_CHECK(swl::check_aligned16({v}));
    }
    // (NULL is aligned: the optional operands need no case of their own)
    SWL_KV_CHECK(swl::check_aligned16({q, k, cos_table, sin_table, q_bias, k_bias, v_bias, q_norm_w, k_norm_w}));
    const bool norm = q_norm_w != nullptr, bias = q_bias || k_bias || v_bias;
    const int vh = v_bias ? num_kv_heads : 0;
    SWL_DISPATCH_DTYPE(dtype, T, {
        swl::QkPrepArgs<T> p;
        p.q = static_cast<T *>(q), p.k = static_cast<T *>(k), p.v = static_cast<T *>(v);
        p.q_bias = static_cast<const T *>(q_bias), p.k_bias = static_cast<const T *>(k_bias);
        p.v_bias = static_cast<const T *>(v_bias);
        p.q_norm_w = static_cast<const T *>(q_norm_w), p.k_norm_w = static_cast<const T *>(k_norm_w);
        p.cos_t = static_cast<const T *>(cos_table), p.sin_t = static_cast<const T *>(sin_table), p.pos_idx = pos_idx;
        p.H = num_q_heads, p.KVH = num_kv_heads, p.VH = vh, p.D = head_dim;
        p.lg_chunks = head_dim == 32 ? 1 : head_dim == 64 ? 2 : head_dim == 128 ? 3 : 4;
        p.num_items = num_tokens * (static_cast<int64_t>(num_q_heads) + num_kv_heads + vh) * (head_dim / 16);
        p.q_tok_stride = q_tok_stride, p.k_tok_stride = k_tok_stride, p.v_tok_stride = v_tok_stride;
        p.eps = eps, p.inv_d = 1.0f / static_cast<float>(head_dim);
        if (norm && bias) swl::launch_qk_prep<T, true, true>(p, stream);
        else if (norm) swl::launch_qk_prep<T, true, false>(p, stream);
        else if (bias) swl::launch_qk_prep<T, false, true>(p, stream);
        else swl::launch_qk_prep<T, false, false>(p, stream);
    });
    return swl::check_launch();
}
