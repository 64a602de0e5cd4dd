// hutk_fim.h -- the rule of the fill-in-the-middle render (include/hutoken_amd.h) as two pure
// functions, plain C++ for the host and the device alike, like hutk_philox.h: which documents are transformed and where
// they are cut (fim_decide), and what stands at position p of a rendered document (fim_locate).  The kernels of
// hutk_collate.hip call them, and besides those only hutk_debug_fim_decide and hutk_debug_fim_locate, through which the
// arithmetic is tested without a GPU (tests/test_fim_cpu.py against tests/fim_ref.py).
#pragma once
#include <cstdint>

#include "hutk_philox.h"

namespace hutk {

constexpr int32_t FIM_PLAIN = 0, FIM_PSM = 1, FIM_SPM = 2;                                      // kinds
constexpr int32_t FIM_PART_PLAIN = 0, FIM_PART_PREFIX = 1, FIM_PART_MIDDLE = 2, FIM_PART_SUFFIX = 3, FIM_PART_SENTINEL = 4;
constexpr int32_t FIM_PRE = 0, FIM_SUF = 1, FIM_MID = 2, FIM_END = 3;                           // the sentinels' numbers

struct FimCut {
    int32_t kind;
    int64_t lo, hi;  // 0 <= lo <= hi <= len; a plain document has lo == hi == len
};

// Document number `doc` of length `len` (ids at token level, bytes at character level) draws (u0, u1, u2, u3) =
// draw(seed, doc, 0, DRAW_FIM).  It is transformed iff u0 < fim_below and 1 <= len < 2^31, SPM iff transformed and
// u1 < spm_below; a = (u2 * (len + 1)) >> 32, b = (u3 * (len + 1)) >> 32, lo = min(a, b), hi = max(a, b).
HUTK_PHILOX_HD inline FimCut fim_decide(uint64_t seed, int64_t doc, int64_t len, uint64_t fim_below, uint64_t spm_below) {
    const Philox4 u = draw(seed, doc, 0, DRAW_FIM);
    if (!(u.x < fim_below) || len < 1 || len >= ((int64_t)1 << 31)) return FimCut{FIM_PLAIN, len, len};
    const uint64_t m = (uint64_t)len + 1;
    const int64_t a = (int64_t)(((uint64_t)u.z * m) >> 32), b = (int64_t)(((uint64_t)u.w * m) >> 32);
    return FimCut{u.y < spm_below ? FIM_SPM : FIM_PSM, a < b ? a : b, a < b ? b : a};
}

// the outputs a document of n ids gives: n when plain, n + 3 + E when transformed (E: 1 with an end sentinel)
HUTK_PHILOX_HD inline int64_t fim_length(int64_t n, int32_t kind, int32_t E) { return kind == FIM_PLAIN ? n : n + 3 + E; }

struct FimPlace {
    int32_t part;  // FIM_PART_*; -1: p is no position of the document
    int64_t v;     // on a token of the document its index inside the document; on a sentinel its number (FIM_PRE ..)
};

// Position p of the rendered document: n ids cut at 0 <= lo <= hi <= n, P = lo, M = hi - lo, S = n - hi.
//   plain   x                                      p: x[p]
//   PSM     pre prefix suf suffix mid middle [end]
//   SPM     pre suf suffix mid prefix middle [end]
HUTK_PHILOX_HD inline FimPlace fim_locate(int64_t n, int64_t lo, int64_t hi, int32_t kind, int32_t E, int64_t p) {
    if (p < 0 || p >= fim_length(n, kind, E)) return FimPlace{-1, -1};
    if (kind == FIM_PLAIN) return FimPlace{FIM_PART_PLAIN, p};
    if (p == 0) return FimPlace{FIM_PART_SENTINEL, FIM_PRE};
    if (p == n + 3) return FimPlace{FIM_PART_SENTINEL, FIM_END};
    const int64_t P = lo, S = n - hi;
    if (kind == FIM_PSM) {
        if (p <= P) return FimPlace{FIM_PART_PREFIX, p - 1};
        if (p == P + 1) return FimPlace{FIM_PART_SENTINEL, FIM_SUF};
        if (p <= P + S + 1) return FimPlace{FIM_PART_SUFFIX, hi + (p - P - 2)};
        if (p == P + S + 2) return FimPlace{FIM_PART_SENTINEL, FIM_MID};
        return FimPlace{FIM_PART_MIDDLE, lo + (p - P - S - 3)};
    }
    if (p == 1) return FimPlace{FIM_PART_SENTINEL, FIM_SUF};
    if (p <= S + 1) return FimPlace{FIM_PART_SUFFIX, hi + (p - 2)};
    if (p == S + 2) return FimPlace{FIM_PART_SENTINEL, FIM_MID};
    const int64_t k = p - S - 3;  // prefix and middle stand in the document's order behind mid
    return FimPlace{k < P ? FIM_PART_PREFIX : FIM_PART_MIDDLE, k};
}

}  // namespace hutk
