// fixed_point.h — the 2^32 fixed-point addend of the exact integer sums (vector_pairs.hip: c, c * c and e per bin;
// relaxation.hip: sinc(q |dr|) per lag). A sum of such addends is an integer: exact in any order.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr double VP_ONE = 4294967296.0;       // 2^32: the fixed-point unit

// (int64) rint(v * 2^32) of |v| < 2 as a two's-complement word. The product is exact (a power of two) and below 2^33 in
// magnitude; adding 1.5 * 2^52 moves it to where a double's ulp is 1, which rounds it to an integer, half to even, as
// rint does, and leaves that integer in the low bits of the sum: the difference of the two bit patterns is the value.
// One addition and one 64-bit subtraction instead of a rounding and a double-to-int64 conversion sequence.
__device__ __forceinline__ unsigned long long vp_fixed(double v)
{
    constexpr double magic = 6755399441055744.0;  // 1.5 * 2^52
    return (unsigned long long)(__double_as_longlong(v * VP_ONE + magic) - __double_as_longlong(magic));
}

}  // namespace
