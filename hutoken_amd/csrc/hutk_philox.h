// hutk_philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the
// counter-based generator behind the masked-LM corruption, the span corruption and the fill-in-the-middle cuts of
// hutk_collate.hip (DESIGN.md sections 8g, 8h, 8k).  Plain C++ for the
// host and the device alike: four 32-bit words out of a 128-bit counter and a 64-bit key, ten rounds of two
// 32 x 32 -> 64 bit multiplies each, no state.  The known-answer vectors of the Random123 distribution are in
// tests/test_targets_cpu.py.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HUTK_PHILOX_HD __host__ __device__
#else
#define HUTK_PHILOX_HD
#endif

namespace hutk {

struct Philox4 {
    uint32_t x, y, z, w;
};

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;  // the round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;  // what the key grows by between rounds

HUTK_PHILOX_HD inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{c0, c1, c2, c3};
}

// What the corruption draws with: every draw is a pure function of (seed, row, unit, purpose).
//   key     = (low32(seed), high32(seed))
//   counter = (low32(row), high32(row), unit, purpose)
// purpose 0: the draw of column `unit` (x: selection in token mode, y: replacement kind, z: random id);
// purpose 1 / 2: the draw of word `unit` of side A / B (x: selection in whole-word mode);
// purpose 3: the span draw of column `unit` (x: whether a noise span starts there, y: its length);
// purpose 4: the fill-in-the-middle draw of DOCUMENT `row`, unit 0 (x: whether it is transformed, y: PSM or SPM, z and w:
//            the two cuts; hutk_fim.h).
constexpr uint32_t DRAW_COLUMN = 0, DRAW_WORD_A = 1, DRAW_WORD_B = 2, DRAW_SPAN = 3, DRAW_FIM = 4;

HUTK_PHILOX_HD inline Philox4 draw(uint64_t seed, int64_t row, uint32_t unit, uint32_t purpose) {
    return philox4x32_10((uint32_t)(uint64_t)row, (uint32_t)((uint64_t)row >> 32), unit, purpose, (uint32_t)seed,
                         (uint32_t)(seed >> 32));
}

// an id in [0, vocab) from one draw, vocab <= 2^31
HUTK_PHILOX_HD inline int32_t draw_id(uint32_t u, uint64_t vocab) { return (int32_t)(((uint64_t)u * vocab) >> 32); }

}  // namespace hutk
