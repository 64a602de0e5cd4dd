// hutk_wcache.h -- the learned table of MULTI-TOKEN words ("word cache"): slot layout, key packing
// and hash, shared by the kernels (k_tiles reads, k_finish's d_learn inserts), the host (hutk_api.cpp allocates, clears
// and reports) and the host model in tests/cpu/wcache_check.cpp.  Nothing here needs HIP.
//
// The BPE encoding of a word is a function of its bytes and the context's tables, so the symbols the merge loop found
// for a word are right for every later occurrence of the same bytes.  A BUCKET is one 128-byte line of two 64-byte
// SLOTS; one hash of the key gives the line.  A slot is sixteen dwords:
//   w[0..7]   the word's bytes, little endian, zero padded to 30; byte 30 = nb (the word's length), byte 31 = n (ids)
//   w[8..15]  n 16-bit symbols (the tile kernel's symbols, not ids), the rest zero
// n == 0: the slot is empty.  A reader compares all 30 key bytes AND nb before it trusts a slot: nothing rests on what
// the inserter decided.  Inserters claim a slot through a TAG word kept beside the table (zero: free, else a
// fingerprint of the key) that readers never look at.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HUTK_WC_HD __host__ __device__ __forceinline__
#else
#define HUTK_WC_HD inline
#endif

namespace hutk {
namespace wc {

constexpr int KEY_BYTES = 30;  // longest cached word (the whole-word tables stop at 14 / 28 bytes: hutk_device.h)
constexpr int MIN_BYTES = 2;   // a one-byte word never merges
constexpr int MAX_IDS = 16;    // longest cached result
constexpr int SLOT_DWORDS = 16, KEY_DWORDS = 8;
constexpr int DEFAULT_LOG2 = 19;  // buckets: 2^19 lines = 2^20 slots = 64 MiB (HUTK_WORD_CACHE_LOG2; the size sweep: DESIGN.md section 5.5)
constexpr int MAX_LOG2 = 22;
// Candidates one batch can hand to d_learn (64 bytes each), in LIST_SHARDS sub-lists with a count each on a line of its
// own: a workgroup appends to the sub-list of its block index.  (One count for the whole list made a batch of 130 k
// workgroups queue up 130 k adds to one address: 2 ms became 16.)
constexpr uint32_t LIST_CAP = 1u << 20, LIST_SHARDS = 256, SHARD_CAP = LIST_CAP / LIST_SHARDS;
// Learning closes for good (no eviction: DESIGN.md section 3) once entries * CLOSE_DEN >= slots * CLOSE_NUM, or after
// a batch in which more candidates found their bucket full than found a slot, and at least a 64th of the table's
// slots of them: the table is full for this text, and listing words that will be dropped is pure cost.
constexpr uint32_t CLOSE_NUM = 3, CLOSE_DEN = 4, CLOSE_DROP_DIV = 64;

// the context's control words (device memory): N_CTL of them, then the sub-lists' counts at a stride of CTL_STRIDE
enum : int {
    CTL_ENTRIES = 0,  // slots in use
    CTL_CLOSED,       // 1: no more learning
    CTL_LAST,         // candidates the last learning batch appended (hutk_ctx_word_cache_stats)
    CTL_TICKET,       // d_learn: workgroups that are done with their sub-lists
    CTL_B_LISTED,     // d_learn, this batch: candidates listed, inserted, dropped for a full bucket (zeroed by the last workgroup)
    CTL_B_WON,
    CTL_B_DROPPED,
    N_CTL = 32,
    CTL_STRIDE = 32,
    CTL_DWORDS = N_CTL + CTL_STRIDE * (int)LIST_SHARDS
};
HUTK_WC_HD uint32_t ctl_count(uint32_t shard) { return (uint32_t)N_CTL + (uint32_t)CTL_STRIDE * shard; }

struct Slot { uint32_t w[SLOT_DWORDS]; };

HUTK_WC_HD bool cacheable(int nb, int n) { return nb >= MIN_BYTES && nb <= KEY_BYTES && n >= 1 && n <= MAX_IDS && n <= nb; }

// the bytes of dword j that belong to a word of nb bytes
HUTK_WC_HD uint32_t dword_mask(int nb, int j) {
    const int v = nb - 4 * j;
    return v >= 4 ? 0xFFFFFFFFu : v <= 0 ? 0u : ((1u << (8 * v)) - 1u);
}
// k[0..7]: eight dwords read at the word's first byte -> the key: bytes beyond nb zeroed, nb in byte 30, byte 31 zero
HUTK_WC_HD void make_key(uint32_t (&k)[KEY_DWORDS], int nb) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < KEY_DWORDS; j++) k[j] &= dword_mask(nb, j);
    k[7] = (k[7] & 0xFFFFu) | ((uint32_t)nb << 16);
}
HUTK_WC_HD int slot_nb(uint32_t w7) { return (int)((w7 >> 16) & 0xFFu); }
HUTK_WC_HD int slot_n(uint32_t w7) { return (int)(w7 >> 24); }
HUTK_WC_HD uint32_t with_n(uint32_t k7, int n) { return (k7 & 0x00FFFFFFu) | ((uint32_t)n << 24); }

// the slot's key part s[0..7] holds the key k (whole key and nb; the id count is not part of the key) and an entry
HUTK_WC_HD bool key_hit(const uint32_t (&s)[KEY_DWORDS], const uint32_t (&k)[KEY_DWORDS]) {
    uint32_t d = (s[7] ^ k[7]) & 0x00FFFFFFu;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 7; j++) d |= s[j] ^ k[j];  // (bitwise: one compare, no early exit)
    const int n = slot_n(s[7]);
    return d == 0 && cacheable(slot_nb(s[7]), n);
}

HUTK_WC_HD uint32_t hash_seeded(const uint32_t (&k)[KEY_DWORDS], uint32_t seed, uint32_t mul) {
    uint32_t h = seed;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < KEY_DWORDS; j++) {
        h = (h ^ (j == 7 ? k[j] & 0x00FFFFFFu : k[j])) * mul;
        h = (h << 13) | (h >> 19);
    }
    h ^= h >> 16;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 15);
}
HUTK_WC_HD uint32_t hash(const uint32_t (&k)[KEY_DWORDS]) { return hash_seeded(k, 0x9E3779B9u, 0x85EBCA6Bu); }
HUTK_WC_HD uint32_t bucket_of(uint32_t h, uint32_t log2_buckets) { return log2_buckets ? h >> (32 - log2_buckets) : 0u; }
// The inserters' fingerprint of a key: a second hash, independent of the one that chose the bucket (two words of one
// bucket share that one's top bits); never zero (zero: the slot is free)
HUTK_WC_HD uint32_t tag_of(const uint32_t (&k)[KEY_DWORDS]) { return hash_seeded(k, 0x7F4A7C15u, 0xCC9E2D51u) | 1u; }

// ---- host side: bytes <-> slot (the kernels build theirs from registers) ----
// false: the word or its result is not cacheable (nothing is written)
inline bool pack(Slot& s, const uint8_t* bytes, int nb, const uint16_t* syms, int n) {
    if (!cacheable(nb, n)) return false;
    for (int j = 0; j < SLOT_DWORDS; j++) s.w[j] = 0;
    for (int i = 0; i < nb; i++) s.w[i >> 2] |= (uint32_t)bytes[i] << (8 * (i & 3));
    s.w[7] = with_n(s.w[7] | ((uint32_t)nb << 16), n);
    for (int i = 0; i < n; i++) s.w[8 + (i >> 1)] |= (uint32_t)syms[i] << (16 * (i & 1));
    return true;
}
inline bool unpack(const Slot& s, uint8_t* bytes, int* nb, uint16_t* syms, int* n) {
    *nb = slot_nb(s.w[7]);
    *n = slot_n(s.w[7]);
    if (!cacheable(*nb, *n)) return false;
    for (int i = 0; i < *nb; i++) bytes[i] = (uint8_t)(s.w[i >> 2] >> (8 * (i & 3)));
    for (int i = 0; i < *n; i++) syms[i] = (uint16_t)(s.w[8 + (i >> 1)] >> (16 * (i & 1)));
    return true;
}

}  // namespace wc
}  // namespace hutk
