// hutk_wordbits.h -- the start-bit arithmetic of k_tiles' word rounds (hutk_kernels.hip, phase 5), shared with the host
// check in tests/cpu/wordbits_check.cpp.  Nothing here needs HIP.
//
// A lane owns 16 positions.  f32 holds the word-start flags of its own positions (bits 0..15) and of the next lane's
// (bits 16..31); both functions answer for all sixteen own positions at once, bit j for position j.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HUTK_WB_HD __host__ __device__ __forceinline__
#else
#define HUTK_WB_HD inline
#endif

namespace hutk {
namespace wb {

// bit j: position j + 1 is a start, i.e. what starts at j is one byte long
HUTK_WB_HD uint32_t one_byte(uint32_t f32) { return (f32 >> 1) & 0xFFFFu; }

// bit j: a start among positions j + 1 .. j + KEY, i.e. what starts at j is at most KEY bytes long (9 <= KEY <= 16, so
// that j + KEY stays inside the 32 flags)
template <int KEY>
HUTK_WB_HD uint32_t within(uint32_t f32) {
    static_assert(KEY >= 9 && KEY <= 16, "two spans of eight cover 1 .. KEY, inside f32");
    uint32_t x = f32 >> 1;
    x |= x >> 1;
    x |= x >> 2;
    x |= x >> 4;          // 1 .. 8
    x |= x >> (KEY - 8);  // and KEY - 7 .. KEY
    return x & 0xFFFFu;
}

}  // namespace wb
}  // namespace hutk
