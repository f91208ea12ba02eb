// moe_common.h — the limits and host-side checks the mixture-of-experts translation units share (moe.hip: routing, alignment,
// the 16-row expert GEMMs, combine; moe_wide.hip: the row-tile form of the expert GEMMs for prompt-sized steps).
#pragma once

#include "swl_common.h"

namespace swl {

constexpr int kMoeMaxExperts = 256;
constexpr int kMoeMaxTopK = 16;
constexpr int kMoeMaxPairs = 4096;
constexpr int kMoeWaves = 8;
constexpr int kMoeLogitsF32 = 2;

inline int moe_tile_bound(int pairs, int experts) { return (pairs + 15) / 16 + (experts < pairs ? experts : pairs); }

inline bool moe_dtype_ok(int dtype) { return dtype == SWL_F16 || dtype == SWL_BF16; }

// SWL_OK when (T, k, E) is a legal step, else the error code
inline int moe_step_check(int num_tokens, int top_k, int num_experts) {
    if (num_tokens < 0 || top_k <= 0 || num_experts <= 0 || top_k > num_experts) return SWL_ERR_BAD_ARG;
    if (num_experts > kMoeMaxExperts || top_k > kMoeMaxTopK) return SWL_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(num_tokens) * top_k > kMoeMaxPairs) return SWL_ERR_UNSUPPORTED;
    return SWL_OK;
}

} // namespace swl
