// logits_bits.h — the 16-bit logits as raw bit patterns: what logits_adjust.hip (min-p) and guided.hip (token masks) share.
// Both rewrite elements to -inf by their bit pattern and move a row in 8-element (16-byte) vectors where they can.
#pragma once
#include "swl_common.h"

namespace swl {

typedef uint16_t bits8_t __attribute__((ext_vector_type(8)));

template <typename T>
__device__ __forceinline__ float bits_to_f(uint16_t b) {
    if constexpr (std::is_same<T, f16>::value)
        return static_cast<float>(__builtin_bit_cast(f16, b));
    else
        return __uint_as_float(static_cast<uint32_t>(b) << 16);
}

template <typename T>
__device__ __forceinline__ constexpr uint16_t neg_inf_bits() {
    return std::is_same<T, f16>::value ? 0xfc00u : 0xff80u;
}

} // namespace swl
