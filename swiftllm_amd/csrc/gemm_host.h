// gemm_host.h — what the entry points of the decode GEMMs do alike on the host: gemm_skinny.hip (<= 32 and 33..64 tokens)
// and gemm_wide.hip (65..256). The argument checks, the split-K driver and the launch of the slab reduce. Host code only.
#pragma once

#include "swl_common.h"

namespace swl {

// What a GEMM entry point was handed, with the limits of the kernel behind it.
struct GemmArgs {
    void *out;              // out[M, N] in T — or, `partial`, the fp32 slabs [k_splits][M][N]
    const void *x, *w;
    void *workspace;        // fp32 split-K scratch; may be NULL when K is not split. `partial`: the slabs again
    size_t workspace_bytes;
    int M, N, K;            // N: the output columns (I of a SiLU-gate entry)
    int64_t x_row_stride, out_row_stride;
    int k_splits;
    int max_m;              // 32 / 64 / 256 tokens
    int k_tile;             // K granule of the kernel: 128 / 64
    bool partial = false;   // a slab entry: no output stride, float4 slab stores, k_splits = 0 is not a choice
};

// Callers are promised every refusal code, double faults included, so the checks are steps that return one code each,
// in the order the entries run them; an entry puts the checks of its own before, between or after them.
//   check_gemm_counts    SWL_ERR_BAD_ARG; then M == 0 is SWL_OK with nothing else looked at (the entry returns)
//   check_gemm_operands  SWL_ERR_BAD_ARG
//   check_gemm_shape     SWL_ERR_UNSUPPORTED
//   check_gemm_strides   SWL_ERR_BAD_ARG
//   check_gemm_alignment SWL_ERR_BAD_ARG
//   check_gemm_k_splits  SWL_ERR_BAD_ARG — the last step of an entry that reduces, right behind the operands of a slab entry
#define SWL_GEMM_CHECK(step)                         \
    do {                                             \
        if (const int rc_ = (step); rc_ != SWL_OK) return rc_; \
    } while (0)

inline int check_gemm_counts(const GemmArgs &a) { return a.M < 0 || a.N <= 0 || a.K <= 0 ? SWL_ERR_BAD_ARG : SWL_OK; }

inline int check_gemm_operands(const GemmArgs &a) { return a.out && a.x && a.w ? SWL_OK : SWL_ERR_BAD_ARG; }

// A power of two up to 16; 0 = the library's choice, where there is a reduce to hide it behind.
inline int check_gemm_k_splits(const GemmArgs &a) {
    const int ks = a.k_splits;
    return ks < (a.partial ? 1 : 0) || ks > 16 || (ks & (ks - 1)) ? SWL_ERR_BAD_ARG : SWL_OK;
}

inline int check_gemm_shape(const GemmArgs &a) {
    return a.M > a.max_m || (a.N & 31) || (a.K & (a.k_tile - 1)) ? SWL_ERR_UNSUPPORTED : SWL_OK;
}

// 16-byte loads of x rows, 8-byte stores of out rows.
inline int check_gemm_strides(const GemmArgs &a) {
    if (a.x_row_stride < a.K || (a.x_row_stride & 7)) return SWL_ERR_BAD_ARG;
    if (!a.partial && (a.out_row_stride < a.N || (a.out_row_stride & 3))) return SWL_ERR_BAD_ARG;
    return SWL_OK;
}

inline int check_gemm_alignment(const GemmArgs &a) {
    const bool out_ok = a.partial ? aligned16(a.out) : !(reinterpret_cast<uintptr_t>(a.out) & 7u);
    return aligned16(a.x) && aligned16(a.w) && out_ok && (!a.workspace || aligned16(a.workspace)) ? SWL_OK : SWL_ERR_BAD_ARG;
}

// All the steps, for an entry with no check of its own between them. true: the entry is done and returns rc — the
// refusal, or SWL_OK for M == 0.
inline bool gemm_args_settled(const GemmArgs &a, int &rc) {
    if ((rc = check_gemm_counts(a)) != SWL_OK || a.M == 0) return true;
    if ((rc = check_gemm_operands(a)) != SWL_OK) return true;
    if (a.partial && (rc = check_gemm_k_splits(a)) != SWL_OK) return true;
    if ((rc = check_gemm_shape(a)) != SWL_OK) return true;
    if ((rc = check_gemm_strides(a)) != SWL_OK) return true;
    if ((rc = check_gemm_alignment(a)) != SWL_OK) return true;
    return !a.partial && (rc = check_gemm_k_splits(a)) != SWL_OK;
}

// out[M, N] = round(sum of the ks slabs, in slab order): splitk_reduce_kernel, defined with it in gemm_skinny.hip.
template <typename T>
void launch_splitk_reduce(T *out, const float *slabs, int ks, int M, int N, int64_t out_row_stride, hipStream_t stream);

// The split-K skeleton behind an entry, once `ks` is chosen: direct(out) writes out[M, N] in one launch, partial(slabs)
// the ks slabs into the workspace, which the reduce then adds up. A slab entry (a.partial) stops after the slabs, ks >= 1:
// a fused consumer sums them (swl_splitk_*).
template <typename T, typename Direct, typename Partial>
inline int run_splitk(const GemmArgs &a, int ks, hipStream_t stream, Direct direct, Partial partial) {
    if (ks == 1 && !a.partial) {
        direct(a.out);
        return check_launch();
    }
    float *ws = static_cast<float *>(a.workspace);
    if (!ws || a.workspace_bytes < static_cast<size_t>(ks) * a.M * a.N * sizeof(float)) return SWL_ERR_BAD_ARG;
    partial(ws);
    if (!a.partial) launch_splitk_reduce<T>(static_cast<T *>(a.out), ws, ks, a.M, a.N, a.out_row_stride, stream);
    return check_launch();
}

} // namespace swl
