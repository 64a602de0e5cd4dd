// hutk_train.hip -- BPE training on the GPU (hutk_trainer_*, include/hutoken_amd.h).
//
// Replaces the reference's trainers (src/lib.c:76-126, src/bpe.c, src/bbpe.c) with the semantics of
// tools/train_vocab.cpp in "bytes" or "chars" mode, bit for bit:
//   words    the reference's splitter (hutk_classify.h, exact form), never across documents, no length cap
//   symbols  bytes: byte values 0..255, A = 256.  chars: unique words holding a byte < 0x20 or 0x7F are dropped, ' '
//            becomes E2 96 81, each word is cut left to right into characters (length from the lead byte: < 0x80 1,
//            110xxxxx 2, 1110xxxx 3, any other 4; cut short at the word's end), and the distinct characters, sorted
//            as byte strings, are 0..A-1.  Merge k creates A + k
//   count    pair (a, b): sum over unique words of count x adjacent (a, b) positions (overlaps count)
//   select   highest count, ties to the smaller (uint64)a << 32 | b, stop when no count >= 1
//   apply    left to right, non-overlapping (aaaa -> n n, aaa -> n a)
//
// Phases
//   add   k_docmark + k_split: word-start bits (classify16_exact per 16 bytes) and the NUL check;
//         k_insert / k_insert_pending: each word into a device hash table of unique words (key = 64-bit hash,
//         equality = full byte compare against the arena copy).  A slot is claimed by CAS on its key, then its
//         bytes are copied into the arena and it is published with a release store; a word that meets a claimed
//         but unpublished slot with its own hash is deferred to the next round (no spinning).
//   symbolise (hutk_trainer_alphabet, or the start of run; once)  k_words_from_table lists the unique words; bytes
//         mode copies the arena to the symbol CSR (k_bytes_to_sym).  Chars mode: k_chars_xform applies the skip and
//         space rules, k_chars_walk<false> cuts characters and inserts them into a device hash set, the host sorts
//         the compacted keys, k_cset_number numbers them, and k_chars_walk<true> writes the ids into the CSR; all
//         three a wavefront per word, 64 bytes per trip.
//   run   the CSR holds the unique words' symbols; k_init_* count the pairs into an open-addressing
//         table (u64 key, i64 count, integer atomics only); then per merge two kernels, no host round trip:
//         k_select (grid reduction, the last block decides) and k_apply_short (a lane per word) /
//         k_apply_long (a wavefront per word finds the first occurrence, one lane rewrites from there).
//         Pair counts are updated by the exact delta of each occurrence (old neighbours out, new ones in).
//         The host synchronises every few merges to drop finished words and rebuild the pair table; a step
//         that might not find room for its new keys pauses the loop instead (the host grows the table and
//         resumes), so the table can never fill.
//
// Test-only knobs, read by every symbolisation and run (unset: the constants below, the same code path)
//   HUTK_TRAIN_SYNC_EVERY=n     merges enqueued between host synchronisations (n >= 1; default SYNC_EVERY = 64).
//                               1 re-partitions the word lists and checks the table after every merge; a very large
//                               value leaves the device-side pause as the only guard against a full pair table.
//   HUTK_TRAIN_PAIR_CAP_LOG2=n  the pair table's floor, 2^n slots (default 16): the lower bound of the initial size
//                               (4 * min(symbols, 65536) stays the other bound) and of every rebuild, and 2^(n-2) in
//                               the shrink test.  A small floor makes pauses and shrinks frequent; 21 or more gives
//                               k_select its full 1024 blocks with 8+ grid-stride trips per thread.
//   HUTK_TRAIN_CHARSET_CAP_LOG2=n  chars mode: the character set's first size, 2^n slots (default: 2 * min(symbols,
//                               2^20), at least 2^12).  A small size makes the set pass half load, grow eightfold and
//                               repeat its pass.
// hutk_trainer_debug_counters reports which of these paths a run took (host values only, no added synchronisation).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hutk_host.h"
#include "hutk_classify.h"

namespace {

constexpr int TB = 256;              // threads per block
constexpr int LONG_WORD = 64;        // words with more symbols take the wavefront-per-word kernels
constexpr uint64_t PK_EMPTY = ~0ull; // pair table: empty key (a = b = -1 is no pair)
constexpr int SYNC_EVERY = 64;       // merges enqueued between host synchronisations
constexpr int PAIR_CAP_LOG2 = 16;    // the pair table's floor: 2^16 slots

__host__ __device__ inline uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__device__ inline uint64_t word_hash(const uint8_t* p, int64_t len) {
    uint64_t h = 0xCBF29CE484222325ull ^ (uint64_t)len;
    for (int64_t i = 0; i < len; i++) h = (h ^ p[i]) * 0x100000001B3ull;
    h = mix64(h);
    return h ? h : 1;  // 0 marks an empty slot
}

__device__ inline uint64_t pkey(int32_t a, int32_t b) { return ((uint64_t)(uint32_t)a << 32) | (uint32_t)b; }

// ---- unique-word table ------------------------------------------------------------------------------------
struct WordTab {
    unsigned long long* key;  // hash, 0 = empty
    uint32_t* state;          // 1 = published (off, len, bytes visible)
    int64_t* off;             // into the arena
    int64_t* len;
    unsigned long long* cnt;
    uint64_t mask;
};

struct AddCtl {                     // device-side counters of one add() call
    unsigned long long n_words;     // word occurrences in the batch
    unsigned long long arena_used;  // bytes of the arena in use
    unsigned long long n_unique;
    unsigned int nul;               // a 0x00 byte was seen
    unsigned int full;              // a probe found no slot (never expected: the table is sized first)
    unsigned int pend_n[2];         // deferred words per round (double buffered)
};

struct Pending {
    int64_t pos, len;
    uint64_t h;
};

__device__ bool bytes_equal(const uint8_t* x, const uint8_t* y, int64_t n) {
    for (int64_t i = 0; i < n; i++)
        if (x[i] != y[i]) return false;
    return true;
}

// 0: counted; 1: deferred (a slot with this hash is claimed but not yet published); 2: table full
__device__ int insert_word(WordTab T, uint8_t* arena, AddCtl* ctl, const uint8_t* src, int64_t len, uint64_t h) {
    uint64_t s = h & T.mask;
    for (uint64_t probe = 0; probe <= T.mask; probe++, s = (s + 1) & T.mask) {
        unsigned long long k = __hip_atomic_load(&T.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            k = atomicCAS(&T.key[s], 0ull, (unsigned long long)h);
            if (k == 0) {  // claimed: copy the bytes, then publish
                const int64_t o = (int64_t)atomicAdd(&ctl->arena_used, (unsigned long long)len);
                for (int64_t i = 0; i < len; i++) arena[o + i] = src[i];
                T.off[s] = o;
                T.len[s] = len;
                __hip_atomic_store(&T.state[s], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                atomicAdd(&T.cnt[s], 1ull);
                atomicAdd(&ctl->n_unique, 1ull);
                return 0;
            }
        }
        if (k != h) continue;
        if (__hip_atomic_load(&T.state[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 0) return 1;
        if (T.len[s] == len && bytes_equal(arena + T.off[s], src, len)) {
            atomicAdd(&T.cnt[s], 1ull);
            return 0;
        }
    }
    return 2;
}

__global__ void k_docmark(const int64_t* offs, int64_t n_docs, int64_t base, int64_t n, uint32_t* dbm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_docs) return;
    const int64_t p = offs[i] - base;
    if (p < n) atomicOr(&dbm[p >> 5], 1u << (p & 31));
}

__device__ inline uint32_t bits32(const uint32_t* bm, int64_t pos, int64_t n_words) {  // bits pos..pos+31
    uint32_t r = 0;
    for (int j = 0; j < 32; j++) {
        const int64_t p = pos + j;
        if (p < 0 || (p >> 5) >= n_words) continue;
        r |= ((bm[p >> 5] >> (p & 31)) & 1u) << j;
    }
    return r;
}

// one thread per 16 input bytes: word-start bits (wsb), word count, NUL check.  `bytes` is zero padded by 32+.
__global__ void k_split(const uint8_t* bytes, int64_t n, const uint32_t* dbm, uint32_t* wsb, AddCtl* ctl) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_groups = (n + 15) >> 4;
    uint32_t nw = 0;
    if (g < n_groups) {
        const int64_t p0 = g << 4;
        uint32_t d[8];
        for (int q = 0; q < 8; q++) {
            const int64_t p = p0 - 8 + 4 * q;
            d[q] = p < 0 ? 0u : *reinterpret_cast<const uint32_t*>(bytes + p);  // 4-aligned (p0 % 16 == 0)
        }
        // bytes past n are zero (padding); bytes of the window before 0 are zero
        const uint32_t dbits = bits32(dbm, p0 - 8, (n + 31) >> 5);
        uint32_t f = hutk::classify16_exact(d, dbits);
        const int64_t valid = n - p0 < 16 ? n - p0 : 16;
        if (valid < 16) f &= (1u << valid) - 1u;
        wsb[g] = f;
        nw = __popc(f);
        bool nul = false;
        for (int j = 0; j < valid; j++) nul |= ((d[2 + (j >> 2)] >> (8 * (j & 3))) & 0xFFu) == 0;
        if (nul) atomicOr(&ctl->nul, 1u);
    }
    for (int o = 32; o > 0; o >>= 1) nw += __shfl_xor(nw, o);
    if ((threadIdx.x & 63) == 0 && nw) atomicAdd(&ctl->n_words, (unsigned long long)nw);
}

__global__ void k_insert(const uint8_t* bytes, int64_t n, const uint32_t* wsb, WordTab T, uint8_t* arena, AddCtl* ctl,
                         Pending* pend) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_groups = (n + 15) >> 4;
    if (g >= n_groups) return;
    uint32_t f = wsb[g];
    while (f) {
        const int j = __ffs(f) - 1;
        f &= f - 1;
        const int64_t p = (g << 4) + j;
        int64_t e;
        if (f) {
            e = (g << 4) + __ffs(f) - 1;
        } else {
            int64_t h = g + 1;
            while (h < n_groups && wsb[h] == 0) h++;
            e = h < n_groups ? (h << 4) + __ffs(wsb[h]) - 1 : n;
        }
        const uint64_t hh = word_hash(bytes + p, e - p);
        const int r = insert_word(T, arena, ctl, bytes + p, e - p, hh);
        if (r == 1) {
            const unsigned i = atomicAdd(&ctl->pend_n[0], 1u);
            pend[i] = Pending{p, e - p, hh};
        } else if (r == 2) {
            atomicOr(&ctl->full, 1u);
        }
    }
}

__global__ void k_insert_pending(const uint8_t* bytes, WordTab T, uint8_t* arena, AddCtl* ctl, const Pending* pin,
                                 int which_in, Pending* pout) {
    const unsigned n_in = ctl->pend_n[which_in];
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
        const Pending w = pin[i];
        const int r = insert_word(T, arena, ctl, bytes + w.pos, w.len, w.h);
        if (r == 1) {
            const unsigned o = atomicAdd(&ctl->pend_n[which_in ^ 1], 1u);
            pout[o] = w;
        } else if (r == 2) {
            atomicOr(&ctl->full, 1u);
        }
    }
}

// rehash the published entries of `src` into the empty table `dst` (distinct words: no byte compare)
__global__ void k_word_rehash(WordTab src, uint64_t src_cap, WordTab dst, AddCtl* ctl) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= src_cap || src.key[i] == 0) return;
    const unsigned long long h = src.key[i];
    uint64_t s = h & dst.mask;
    for (uint64_t probe = 0; probe <= dst.mask; probe++, s = (s + 1) & dst.mask) {
        if (atomicCAS(&dst.key[s], 0ull, h) == 0) {
            dst.off[s] = src.off[i];
            dst.len[s] = src.len[i];
            dst.cnt[s] = src.cnt[i];
            dst.state[s] = 1;
            return;
        }
    }
    atomicOr(&ctl->full, 1u);
}

// ---- merge loop -------------------------------------------------------------------------------------------
struct PairTab {
    unsigned long long* key;
    long long* cnt;
    uint64_t mask;
    unsigned long long* used;  // slots holding a key
    unsigned int* full;
};

struct LoopCtl {
    long long best_cnt;
    unsigned long long best_key;
    int stop;        // no pair with count >= 1 is left
    int pause;       // the table might not hold the next step's new keys: the host grows it and resumes
    int n_done;      // merges done
    unsigned int blocks_done;
};

__device__ inline uint64_t pslot(uint64_t k, uint64_t mask) { return mix64(k) & mask; }

__device__ void pair_add(PairTab T, uint64_t k, long long d) {
    uint64_t s = pslot(k, T.mask);
    for (uint64_t probe = 0; probe <= T.mask; probe++, s = (s + 1) & T.mask) {
        unsigned long long cur = __hip_atomic_load(&T.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == PK_EMPTY) {
            cur = atomicCAS(&T.key[s], PK_EMPTY, (unsigned long long)k);
            if (cur == PK_EMPTY) {
                atomicAdd(T.used, 1ull);
                cur = k;
            }
        }
        if (cur == k) {
            atomicAdd((unsigned long long*)&T.cnt[s], (unsigned long long)d);
            return;
        }
    }
    atomicOr(T.full, 1u);
}

// published word-table slots -> word arrays (id order is irrelevant: every count is a sum)
__global__ void k_words_from_table(WordTab T, uint64_t cap, int64_t* w_off, int32_t* w_len, int64_t* w_cnt,
                                   unsigned int* n_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || T.key[i] == 0) return;
    const unsigned w = atomicAdd(n_out, 1u);
    w_off[w] = T.off[i];
    w_len[w] = (int32_t)T.len[i];
    w_cnt[w] = (int64_t)T.cnt[i];
}

__global__ void k_bytes_to_sym(const uint8_t* arena, int64_t n, int32_t* sym) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        sym[i] = arena[i];
}

// ---- chars mode: UTF-8 characters as the initial symbols ----------------------------------------------------
// A wavefront per unique word (grid-stride over words), 64 bytes per trip, so a long word is never walked by one
// lane.  The transformed word (' ' -> E2 96 81) of the word at arena offset o lives at tbuf + 3 * o: it is never more
// than three times as long, so no offsets need to be computed.  Every word has at most as many characters as bytes (a
// space's expansion starts at most one character), so the sym CSR keeps the arena's offsets.
struct CharSet {                // distinct character keys: big-endian bytes, zero padded (0 = empty slot)
    unsigned int* key;
    int32_t* id;                // the key's symbol id, after numbering
    uint64_t mask;
    unsigned long long* used;
    unsigned int* full;         // more than half of the slots used: the host grows the set and repeats
};

__device__ inline int char_len(uint32_t lead) {  // from the lead byte; stray continuations and F0..FF take 4
    return lead < 0x80 ? 1 : (lead & 0xE0) == 0xC0 ? 2 : (lead & 0xF0) == 0xE0 ? 3 : 4;
}

__device__ void cset_insert(CharSet C, uint32_t k) {
    uint64_t s = mix64(k) & C.mask;
    for (uint64_t probe = 0; probe <= C.mask; probe++, s = (s + 1) & C.mask) {
        unsigned int cur = __hip_atomic_load(&C.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&C.key[s], 0u, k);
            if (cur == 0) {
                if (2 * (atomicAdd(C.used, 1ull) + 1) > C.mask + 1) atomicOr(C.full, 1u);
                return;
            }
        }
        if (cur == k) return;
    }
    atomicOr(C.full, 1u);
}

__device__ int32_t cset_find(CharSet C, uint32_t k) {  // k is present (inserted by k_chars_walk<false>)
    uint64_t s = mix64(k) & C.mask;
    while (C.key[s] != k) s = (s + 1) & C.mask;
    return C.id[s];
}

// rules 2 and 3: a word holding a byte < 0x20 or 0x7F is dropped (t_len = -1); ' ' becomes E2 96 81
__global__ void __launch_bounds__(TB) k_chars_xform(const uint8_t* arena, const int64_t* w_off, const int32_t* w_len,
                                                    int64_t n_words, uint8_t* tbuf, int64_t* t_len,
                                                    unsigned long long* n_dropped) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < n_words; w += n_waves) {
        const int64_t off = w_off[w];
        const int32_t len = w_len[w];
        const uint8_t* src = arena + off;
        uint8_t* dst = tbuf + 3 * off;
        int64_t tpos = 0;  // (a word of 2^31 - 1 spaces is 3 * (2^31 - 1) bytes long)
        bool bad = false;
        for (int64_t base = 0; base < len; base += 64) {
            const int64_t j = base + lane;
            const bool in = j < len;
            const uint32_t c = in ? src[j] : 0x61u;
            const unsigned long long sp = __ballot(in && c == 0x20);
            if (__ballot(in && (c < 0x20 || c == 0x7F))) {
                bad = true;
                break;
            }
            const int64_t p = tpos + lane + 2 * __popcll(sp & below);
            if (in && c == 0x20) {
                dst[p] = 0xE2;
                dst[p + 1] = 0x96;
                dst[p + 2] = 0x81;
            } else if (in) {
                dst[p] = (uint8_t)c;
            }
            tpos += std::min<int64_t>(64, len - base) + 2 * __popcll(sp);
        }
        if (lane == 0) {
            t_len[w] = bad ? -1 : tpos;
            if (bad) atomicAdd(n_dropped, 1ull);
        }
    }
}

// rules 4 and 5: cut the transformed word into characters, left to right.  NUMBER = false: insert every character
// into the set and write the word's character count to w_len (0 for a dropped word); NUMBER = true: write the
// characters' ids into the sym CSR.
template <bool NUMBER>
__global__ void __launch_bounds__(TB) k_chars_walk(const uint8_t* tbuf, const int64_t* w_off, const int64_t* t_len,
                                                   int64_t n_words, CharSet C, int32_t* w_len, int32_t* sym) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < n_words; w += n_waves) {
        if (!NUMBER && __builtin_amdgcn_readfirstlane(__hip_atomic_load(C.full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
            return;  // the set is being outgrown: the host repeats this pass
        const int64_t tl = t_len[w];
        const int64_t off = w_off[w];
        const uint8_t* s = tbuf + 3 * off;
        int32_t carry = 0, n_ch = 0;  // carry: the first character start of the next 64 bytes, past their start
        for (int64_t base = 0; base < tl; base += 64) {
            const int64_t j = base + lane;
            const uint32_t c = j < tl ? s[j] : 0u;
            const int L = char_len(c);
            const unsigned long long m2 = __ballot(L == 2), m3 = __ballot(L == 3), m4 = __ballot(L == 4);
            const int lim = (int)std::min<int64_t>(64, tl - base);
            unsigned long long starts;
            int p;
            if ((m2 | m3 | m4) == 0) {  // all single bytes
                starts = (lim == 64 ? ~0ull : (1ull << lim) - 1) & (~0ull << carry);
                p = lim;
            } else {
                starts = 0;
                for (p = carry; p < lim;) {
                    starts |= 1ull << p;
                    p += 1 + (int)((m2 >> p) & 1) + 2 * (int)((m3 >> p) & 1) + 3 * (int)((m4 >> p) & 1);
                }
            }
            carry = p - 64;
            if ((starts >> lane) & 1) {
                uint32_t k = c << 24;
                for (int q = 1; q < L && j + q < tl; q++) k |= (uint32_t)s[j + q] << (24 - 8 * q);
                if (NUMBER)
                    sym[off + n_ch + __popcll(starts & below)] = cset_find(C, k);
                else
                    cset_insert(C, k);
            }
            n_ch += __popcll(starts);
        }
        if (!NUMBER && lane == 0) w_len[w] = tl > 0 ? n_ch : 0;
    }
}

__global__ void k_cset_compact(CharSet C, uint64_t cap, uint32_t* out, unsigned int* n_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || C.key[i] == 0) return;
    out[atomicAdd(n_out, 1u)] = C.key[i];
}

// sorted[i] gets id i
__global__ void k_cset_number(CharSet C, const uint32_t* sorted, unsigned n) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t s = mix64(sorted[i]) & C.mask;
    while (C.key[s] != sorted[i]) s = (s + 1) & C.mask;
    C.id[s] = (int32_t)i;
}

__global__ void k_sum_len(const int32_t* w_len, int64_t n, unsigned long long* tot) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long v = i < n ? (unsigned long long)w_len[i] : 0ull;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(tot, v);
}

// active lists: words with >= 2 symbols, split by length.  One atomic per wavefront and list (a per-lane atomic on
// the two counters serialises 800k lanes: 9 ms a call on VG)
__global__ void k_partition(const int32_t* ids_in, unsigned n_in, const int32_t* w_len, int32_t* short_out,
                            int32_t* long_out, unsigned int* n_out2) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t w = -1, l = 0;
    if (i < n_in) {
        w = ids_in ? ids_in[i] : (int32_t)i;
        l = w_len[w];
    }
    const unsigned long long ms = __ballot(l >= 2 && l <= LONG_WORD), ml = __ballot(l > LONG_WORD);
    unsigned bs = 0, bl = 0;
    if (lane == 0) {
        if (ms) bs = atomicAdd(&n_out2[0], (unsigned)__popcll(ms));
        if (ml) bl = atomicAdd(&n_out2[1], (unsigned)__popcll(ml));
    }
    bs = __shfl(bs, 0);
    bl = __shfl(bl, 0);
    const unsigned long long below = (1ull << lane) - 1;
    if (l >= 2 && l <= LONG_WORD) short_out[bs + __popcll(ms & below)] = w;
    else if (l > LONG_WORD) long_out[bl + __popcll(ml & below)] = w;
}

__global__ void k_init_short(const int32_t* sym, const int32_t* act, unsigned n_act, const int64_t* w_off,
                             const int32_t* w_len, const int64_t* w_cnt, PairTab T) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_act) return;
    const int32_t w = act[i];
    const int32_t* s = sym + w_off[w];
    const int32_t l = w_len[w];
    const long long c = w_cnt[w];
    for (int32_t j = 0; j + 1 < l; j++) pair_add(T, pkey(s[j], s[j + 1]), c);
}

__global__ void k_init_long(const int32_t* sym, const int32_t* act, unsigned n_act, const int64_t* w_off,
                            const int32_t* w_len, const int64_t* w_cnt, PairTab T) {
    const unsigned wv = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wv >= n_act) return;
    const int32_t w = act[wv];
    const int32_t* s = sym + w_off[w];
    const int32_t l = w_len[w];
    const long long c = w_cnt[w];
    for (int32_t j = lane; j + 1 < l; j += 64) pair_add(T, pkey(s[j], s[j + 1]), c);
}

struct Best {
    long long c;
    unsigned long long k;
};
__device__ inline bool better(const Best& x, const Best& y) { return x.c > y.c || (x.c == y.c && x.k < y.k); }

__device__ Best block_best(Best b, Best* sh) {
    for (int o = 32; o > 0; o >>= 1) {
        Best t{__shfl_xor(b.c, o), __shfl_xor(b.k, o)};
        if (better(t, b)) b = t;
    }
    const int wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wv] = b;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < nw; i++)
            if (better(sh[i], sh[0])) sh[0] = sh[i];
    __syncthreads();
    return sh[0];
}

// merge `step`: the best pair over the table (count desc, key asc, count >= 1), decided by the last block
__global__ void __launch_bounds__(TB) k_select(PairTab T, uint64_t cap, Best* partial, LoopCtl* L, int base, int step,
                                               long long new_key_room, int32_t* out_pairs, int64_t* out_counts) {
    __shared__ Best sh[TB / 64];
    __shared__ bool last;
    if (L->stop || L->pause || *T.full) return;  // (full: the run fails at the next synchronisation; skip the rest)
    Best b{0, ~0ull};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = T.key[i];
        const long long c = T.cnt[i];
        if (k != PK_EMPTY && c > 0) {
            Best t{c, k};
            if (better(t, b)) b = t;
        }
    }
    b = block_best(b, sh);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = b;
        __threadfence();
        last = atomicAdd(&L->blocks_done, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    Best r{0, ~0ull};
    for (unsigned i = threadIdx.x; i < gridDim.x; i += blockDim.x) {
        const Best t{__hip_atomic_load(&partial[i].c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                     __hip_atomic_load(&partial[i].k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
        if (better(t, r)) r = t;
    }
    r = block_best(r, sh);
    if (threadIdx.x == 0) {
        L->blocks_done = 0;
        if (r.c < 1) {
            L->stop = 1;
        } else {
            // every new key holds the new symbol next to an occurrence: at most 2 per occurrence, and at most
            // 2 * (symbols so far) + 1 distinct ones
            const long long sym_bound = 2LL * (base + step) + 1;
            const long long bound = 2 * r.c < sym_bound ? 2 * r.c : sym_bound;
            if ((long long)*T.used + bound > new_key_room) {
                L->pause = 1;
            } else {
                L->best_cnt = r.c;
                L->best_key = r.k;
                out_pairs[2 * step] = (int32_t)(r.k >> 32);
                out_pairs[2 * step + 1] = (int32_t)(r.k & 0xFFFFFFFFu);
                out_counts[step] = r.c;
                L->n_done = step + 1;
            }
        }
    }
}

// rewrite one word from its first occurrence i0 of (a, b), updating the pair counts by the exact delta
__device__ int32_t rewrite_word(int32_t* s, int32_t len, int32_t i0, int32_t a, int32_t b, int32_t n, long long c,
                                PairTab T) {
    int32_t i = i0, w = i0, last_m = -4;
    while (i < len) {
        const int32_t x = s[i];
        if (i + 1 < len && x == a && s[i + 1] == b) {
            pair_add(T, pkey(a, b), -c);
            if (i > 0) {
                if (last_m == i - 2) {  // the left neighbour is the previous new symbol: (b, a) went out there
                    pair_add(T, pkey(n, n), c);
                } else {
                    const int32_t p = s[i - 1];  // (writes so far stop at index w - 1 <= i - 2)
                    pair_add(T, pkey(p, a), -c);
                    pair_add(T, pkey(p, n), c);
                }
            }
            if (i + 2 < len) {
                const int32_t r = s[i + 2];
                pair_add(T, pkey(b, r), -c);
                const bool next_m = i + 3 < len && r == a && s[i + 3] == b;
                if (!next_m) pair_add(T, pkey(n, r), c);
            }
            s[w++] = n;
            last_m = i;
            i += 2;
        } else {
            s[w++] = x;
            i++;
        }
    }
    return w;
}

__global__ void __launch_bounds__(TB) k_apply_short(int32_t* sym, const int32_t* act, unsigned n_act,
                                                    const int64_t* w_off, int32_t* w_len, const int64_t* w_cnt,
                                                    PairTab T, const LoopCtl* L, int base, int step) {
    if (L->stop || L->pause || L->n_done != step + 1) return;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_act) return;
    const int32_t a = (int32_t)(L->best_key >> 32), b = (int32_t)(L->best_key & 0xFFFFFFFFu);
    const int32_t w = act[i];
    const int32_t l = w_len[w];
    if (l < 2) return;
    int32_t* s = sym + w_off[w];
    int32_t i0 = -1;
    int32_t x = s[0];
    for (int32_t j = 0; j + 1 < l; j++) {
        const int32_t y = s[j + 1];
        if (x == a && y == b) {
            i0 = j;
            break;
        }
        x = y;
    }
    if (i0 < 0) return;
    w_len[w] = rewrite_word(s, l, i0, a, b, base + step, w_cnt[w], T);
}

__global__ void __launch_bounds__(TB) k_apply_long(int32_t* sym, const int32_t* act, unsigned n_act,
                                                   const int64_t* w_off, int32_t* w_len, const int64_t* w_cnt,
                                                   PairTab T, const LoopCtl* L, int base, int step) {
    if (L->stop || L->pause || L->n_done != step + 1) return;
    const unsigned wv = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wv >= n_act) return;
    const int32_t a = (int32_t)(L->best_key >> 32), b = (int32_t)(L->best_key & 0xFFFFFFFFu);
    const int32_t w = act[wv];
    const int32_t l = w_len[w];
    if (l < 2) return;
    int32_t* s = sym + w_off[w];
    int32_t i0 = -1;
    for (int32_t base = 0; base + 1 < l; base += 64) {
        const int32_t j = base + lane;
        const bool hit = j + 1 < l && s[j] == a && s[j + 1] == b;
        const unsigned long long m = __ballot(hit);
        if (m) {
            i0 = base + __ffsll((long long)m) - 1;
            break;
        }
    }
    if (i0 < 0 || lane != 0) return;
    w_len[w] = rewrite_word(s, l, i0, a, b, base + step, w_cnt[w], T);
}

// live keys of `src` into the empty table `dst`
__global__ void k_pair_rehash(PairTab src, uint64_t src_cap, PairTab dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= src_cap) return;
    const unsigned long long k = src.key[i];
    const long long c = src.cnt[i];
    if (k == PK_EMPTY || c == 0) return;
    pair_add(dst, k, c);
}

inline unsigned nblocks(uint64_t n, int per = TB) { return (unsigned)std::max<uint64_t>(1, (n + per - 1) / per); }
inline uint64_t pow2_at_least(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace

struct hutk_trainer {
    int device = 0;
    int mode = HUTK_TRAIN_BYTES;
    hipStream_t st = nullptr;
    bool ran = false;
    bool symbolised = false;  // the adding phase is over: sym / w_* below hold the words' initial symbols
    int sym_rc = HUTK_OK;
    // statistics
    int64_t n_docs = 0, n_bytes = 0, n_occ = 0, n_unique = 0, n_sym = 0, n_pairs0 = 0, peak = 0, cur = 0;
    int64_t loop_us = 0;
    // path counters (hutk_trainer_debug_counters), all from values the host reads anyway
    int64_t c_pauses = 0, c_grows = 0, c_shrinks = 0, c_rebuilds = 0, c_syncs = 0, c_pcap_max = 0, c_sel_blocks_max = 0,
            c_word_rehash = 0, c_deferred = 0, c_insert_rounds_max = 0, c_long_to_short = 0, c_dropped = 0,
            c_cset_grows = 0;
    // after symbolisation: the alphabet (symbol id order; chars mode: big-endian keys, bytes mode: empty) and the
    // words' symbols (CSR at the arena offsets; w_len in symbols)
    std::vector<uint32_t> alpha;
    int32_t n_alpha = 0;
    int32_t* sym = nullptr;
    int32_t* w_len = nullptr;
    int64_t *w_off = nullptr, *w_cnt = nullptr;
    // word table + arena (persist across add calls)
    WordTab wt{};
    uint64_t wt_cap = 0;
    uint8_t* arena = nullptr;
    int64_t arena_cap = 0, arena_used = 0;
    AddCtl* ctl = nullptr;
    // per-batch staging
    uint8_t* d_bytes = nullptr;
    int64_t d_bytes_cap = 0;
    int64_t* d_offs = nullptr;
    int64_t d_offs_cap = 0;
    uint32_t* d_dbm = nullptr;
    uint32_t* d_wsb = nullptr;
    int64_t d_bm_cap = 0;
    Pending* pend[2] = {nullptr, nullptr};
    int64_t pend_cap = 0;
    std::vector<std::pair<void*, int64_t>> allocs;

    hipError_t alloc(void** p, int64_t n) {
        hipError_t e = hipMalloc(p, (size_t)std::max<int64_t>(n, 16));
        if (e != hipSuccess) return e;
        allocs.push_back({*p, n});
        cur += n;
        peak = std::max(peak, cur);
        return hipSuccess;
    }
    void release(void* p) {
        if (!p) return;
        for (size_t i = 0; i < allocs.size(); i++)
            if (allocs[i].first == p) {
                cur -= allocs[i].second;
                allocs.erase(allocs.begin() + i);
                break;
            }
        (void)hipFree(p);
    }
    template <class T>
    hipError_t grow(T** p, int64_t* cap, int64_t n) {  // staging buffers: contents not kept
        if (n <= *cap) return hipSuccess;
        release(*p);
        *p = nullptr;
        hipError_t e = alloc((void**)p, n * (int64_t)sizeof(T));
        *cap = e == hipSuccess ? n : 0;
        return e;
    }
};

namespace {

hipError_t wordtab_alloc(hutk_trainer* t, WordTab* w, uint64_t cap) {
    hipError_t e;
    if ((e = t->alloc((void**)&w->key, cap * 8)) != hipSuccess) return e;
    if ((e = t->alloc((void**)&w->state, cap * 4)) != hipSuccess) return e;
    if ((e = t->alloc((void**)&w->off, cap * 8)) != hipSuccess) return e;
    if ((e = t->alloc((void**)&w->len, cap * 8)) != hipSuccess) return e;
    if ((e = t->alloc((void**)&w->cnt, cap * 8)) != hipSuccess) return e;
    w->mask = cap - 1;
    if ((e = hipMemsetAsync(w->key, 0, cap * 8, t->st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w->state, 0, cap * 4, t->st)) != hipSuccess) return e;
    return hipMemsetAsync(w->cnt, 0, cap * 8, t->st);
}

void wordtab_free(hutk_trainer* t, WordTab* w) {
    t->release(w->key);
    t->release(w->state);
    t->release(w->off);
    t->release(w->len);
    t->release(w->cnt);
    *w = WordTab{};
}

// chars mode, between k_words_from_table and the first k_partition: rules 2-5 of the header, then sym / w_len in
// characters.  The distinct characters go into a device hash set (grown and refilled if it passes half load), are
// sorted on the host (a few thousand keys, once) and numbered back into the set.
int symbolise_chars(hutk_trainer* t, int64_t n_words) {
    hipStream_t st = t->st;
    const int64_t n_sym = t->arena_used;
    const unsigned grid = (unsigned)std::min<uint64_t>(nblocks((uint64_t)n_words * 64), 8192);
    uint8_t* tbuf = nullptr;
    int64_t* t_len = nullptr;
    unsigned long long* d_n = nullptr;  // [0] dropped words, [1] set slots used
    unsigned int* d_u = nullptr;        // [0] set full, [1] compacted keys
    HUTK_HIP_TRY(t->alloc((void**)&tbuf, std::max<int64_t>(3 * n_sym, 1)));
    HUTK_HIP_TRY(t->alloc((void**)&t_len, std::max<int64_t>(n_words, 1) * 8));
    HUTK_HIP_TRY(t->alloc((void**)&d_n, 16));
    HUTK_HIP_TRY(t->alloc((void**)&d_u, 8));
    HUTK_HIP_TRY(hipMemsetAsync(d_n, 0, 16, st));
    if (n_words)
        hipLaunchKernelGGL(k_chars_xform, dim3(grid), dim3(TB), 0, st, t->arena, t->w_off, t->w_len, n_words, tbuf,
                           t_len, d_n);
    HUTK_HIP_TRY(hipGetLastError());
    CharSet cs{};
    // (HUTK_TRAIN_CHARSET_CAP_LOG2, test only: the set's first size, so that a test can make it grow)
    const char* e_cs = getenv("HUTK_TRAIN_CHARSET_CAP_LOG2");
    uint64_t cap = e_cs ? 1ull << std::min(std::max(atoi(e_cs), 2), 30)
                        : pow2_at_least(std::max<uint64_t>(2 * std::min<int64_t>(n_sym, 1 << 20), 1 << 12));
    for (;;) {
        HUTK_HIP_TRY(t->alloc((void**)&cs.key, cap * 4));
        HUTK_HIP_TRY(t->alloc((void**)&cs.id, cap * 4));
        HUTK_HIP_TRY(hipMemsetAsync(cs.key, 0, cap * 4, st));
        HUTK_HIP_TRY(hipMemsetAsync(d_n + 1, 0, 8, st));
        HUTK_HIP_TRY(hipMemsetAsync(d_u, 0, 8, st));
        cs.mask = cap - 1;
        cs.used = d_n + 1;
        cs.full = d_u;
        if (n_words)
            hipLaunchKernelGGL(k_chars_walk<false>, dim3(grid), dim3(TB), 0, st, tbuf, t->w_off, t_len, n_words, cs,
                               t->w_len, t->sym);
        HUTK_HIP_TRY(hipGetLastError());
        unsigned full = 0;
        HUTK_HIP_TRY(hipMemcpyAsync(&full, d_u, 4, hipMemcpyDeviceToHost, st));
        HUTK_HIP_TRY(hipStreamSynchronize(st));
        if (!full) break;
        t->release(cs.key);
        t->release(cs.id);
        cap *= 8;  // (a set of 2 * n_sym slots never passes half load: every character is a byte of the arena)
        t->c_cset_grows++;
    }
    uint32_t* keys = nullptr;
    HUTK_HIP_TRY(t->alloc((void**)&keys, cap / 2 * 4 + 4));
    hipLaunchKernelGGL(k_cset_compact, dim3(nblocks(cap)), dim3(TB), 0, st, cs, cap, keys, d_u + 1);
    HUTK_HIP_TRY(hipGetLastError());
    unsigned n_keys = 0;
    unsigned long long dropped = 0;
    HUTK_HIP_TRY(hipMemcpyAsync(&n_keys, d_u + 1, 4, hipMemcpyDeviceToHost, st));
    HUTK_HIP_TRY(hipMemcpyAsync(&dropped, d_n, 8, hipMemcpyDeviceToHost, st));
    HUTK_HIP_TRY(hipStreamSynchronize(st));
    t->alpha.resize(n_keys);
    if (n_keys) HUTK_HIP_TRY(hipMemcpy(t->alpha.data(), keys, (size_t)n_keys * 4, hipMemcpyDeviceToHost));
    std::sort(t->alpha.begin(), t->alpha.end());  // memcmp order of the characters: no byte is 0x00
    if (n_keys) {
        HUTK_HIP_TRY(hipMemcpyAsync(keys, t->alpha.data(), (size_t)n_keys * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cset_number, dim3(nblocks(n_keys)), dim3(TB), 0, st, cs, keys, n_keys);
        hipLaunchKernelGGL(k_chars_walk<true>, dim3(grid), dim3(TB), 0, st, tbuf, t->w_off, t_len, n_words, cs,
                           t->w_len, t->sym);
        HUTK_HIP_TRY(hipGetLastError());
    }
    // characters in all words (the symbol count of the run)
    unsigned long long* d_tot = d_n + 1;
    HUTK_HIP_TRY(hipMemsetAsync(d_tot, 0, 8, st));
    if (n_words) hipLaunchKernelGGL(k_sum_len, dim3(nblocks(n_words)), dim3(TB), 0, st, t->w_len, n_words, d_tot);
    HUTK_HIP_TRY(hipGetLastError());
    unsigned long long tot = 0;
    HUTK_HIP_TRY(hipMemcpyAsync(&tot, d_tot, 8, hipMemcpyDeviceToHost, st));
    HUTK_HIP_TRY(hipStreamSynchronize(st));
    for (void* p : {(void*)tbuf, (void*)t_len, (void*)d_n, (void*)d_u, (void*)cs.key, (void*)cs.id, (void*)keys})
        t->release(p);
    t->n_alpha = (int32_t)n_keys;
    t->c_dropped = (int64_t)dropped;
    t->n_sym = (int64_t)tot;
    return HUTK_OK;
}

int symbolise_once(hutk_trainer* t) {
    HUTK_HIP_TRY(hipSetDevice(t->device));
    hipStream_t st = t->st;
    const int64_t n_words = t->n_unique, n_sym = t->arena_used;
    t->n_sym = n_sym;
    t->n_alpha = t->mode == HUTK_TRAIN_CHARS ? 0 : 256;
    if (n_sym > INT32_MAX || n_words > INT32_MAX)
        return hutk::api_set_error(HUTK_E_UNSUPPORTED, "hutk_trainer_run: more than 2^31 symbols or words");
    // free the staging buffers of add()
    t->release(t->d_bytes), t->d_bytes = nullptr, t->d_bytes_cap = 0;
    t->release(t->d_dbm), t->d_dbm = nullptr;
    t->release(t->d_wsb), t->d_wsb = nullptr, t->d_bm_cap = 0;
    t->release(t->pend[0]), t->release(t->pend[1]), t->pend[0] = t->pend[1] = nullptr, t->pend_cap = 0;
    t->release(t->d_offs), t->d_offs = nullptr, t->d_offs_cap = 0;

    const int64_t nw1 = std::max<int64_t>(n_words, 1);
    unsigned int* n_out = nullptr;
    HUTK_HIP_TRY(t->alloc((void**)&t->sym, std::max<int64_t>(n_sym, 1) * 4));
    HUTK_HIP_TRY(t->alloc((void**)&t->w_len, nw1 * 4));
    HUTK_HIP_TRY(t->alloc((void**)&t->w_off, nw1 * 8));
    HUTK_HIP_TRY(t->alloc((void**)&t->w_cnt, nw1 * 8));
    HUTK_HIP_TRY(t->alloc((void**)&n_out, 4));
    HUTK_HIP_TRY(hipMemsetAsync(n_out, 0, 4, st));
    if (t->wt_cap)
        hipLaunchKernelGGL(k_words_from_table, dim3(nblocks(t->wt_cap)), dim3(TB), 0, st, t->wt, t->wt_cap, t->w_off,
                           t->w_len, t->w_cnt, n_out);
    if (t->mode == HUTK_TRAIN_BYTES && n_sym)
        hipLaunchKernelGGL(k_bytes_to_sym, dim3(1024), dim3(TB), 0, st, t->arena, n_sym, t->sym);
    HUTK_HIP_TRY(hipGetLastError());
    if (t->mode == HUTK_TRAIN_CHARS)
        if (int rc = symbolise_chars(t, n_words)) return rc;
    HUTK_HIP_TRY(hipStreamSynchronize(st));
    t->release(n_out);
    wordtab_free(t, &t->wt);
    t->wt_cap = 0;
    t->release(t->arena), t->arena = nullptr, t->arena_cap = 0;
    return HUTK_OK;
}

// ends the adding phase: the unique words' initial symbols, the alphabet and its size (once; later calls give the same
// answer)
int symbolise(hutk_trainer* t) {
    if (t->symbolised)
        return t->sym_rc == HUTK_OK ? HUTK_OK : hutk::api_set_error(t->sym_rc, "hutk_trainer: symbolisation failed");
    t->symbolised = true;
    t->sym_rc = symbolise_once(t);
    return t->sym_rc;
}

}  // namespace

extern "C" {

int hutk_trainer_create(hutk_trainer** out, int device) { return hutk_trainer_create_mode(out, device, HUTK_TRAIN_BYTES); }

int hutk_trainer_create_mode(hutk_trainer** out, int device, int mode) {
    if (!out) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_create: out is NULL");
    *out = nullptr;
    if (mode != HUTK_TRAIN_BYTES && mode != HUTK_TRAIN_CHARS)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_create_mode: unknown mode");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return hutk::api_set_error(HUTK_E_DEVICE, "hutk_trainer_create: no HIP device");
    if (device < 0) HUTK_HIP_TRY(hipGetDevice(&device));
    if (device >= n) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_trainer_create: no such device");
    HUTK_HIP_TRY(hipSetDevice(device));
    hutk_trainer* t = new hutk_trainer();
    t->device = device;
    t->mode = mode;
    hipError_t e = hipStreamCreateWithFlags(&t->st, hipStreamNonBlocking);
    if (e == hipSuccess) e = t->alloc((void**)&t->ctl, sizeof(AddCtl));
    if (e == hipSuccess) e = hipMemsetAsync(t->ctl, 0, sizeof(AddCtl), t->st);
    if (e == hipSuccess) e = hipStreamSynchronize(t->st);
    if (e != hipSuccess) {
        hutk_trainer_destroy(t);
        return hutk::api_set_error(HUTK_E_DEVICE, std::string("hutk_trainer_create: ") + hipGetErrorString(e));
    }
    *out = t;
    return HUTK_OK;
}

int hutk_trainer_add(hutk_trainer* t, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs) {
    if (!t || n_docs < 0 || (n_docs > 0 && !offsets)) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_add: bad arguments");
    if (t->ran) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_add: the trainer has already run");
    if (t->symbolised) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_add: the alphabet has been read");
    if (n_docs == 0) return HUTK_OK;
    // (a negative offset is reported as a decreasing one: behind a first offset of 0 or more, none can be negative)
    if (offsets[0] < 0) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_add: offsets must not decrease");
    if (int rc = hutk::check_offsets(offsets, n_docs, false, "hutk_trainer_add: offsets")) return rc;
    const int64_t base = offsets[0], n = offsets[n_docs] - base;
    if (n > 0 && !bytes) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_add: bytes is NULL");
    if (n == 0) {
        t->n_docs += n_docs;
        return HUTK_OK;
    }
    HUTK_HIP_TRY(hipSetDevice(t->device));
    hipStream_t st = t->st;
    const int64_t n_groups = (n + 15) / 16, n_bm = (n + 31) / 32;
    HUTK_HIP_TRY(t->grow(&t->d_bytes, &t->d_bytes_cap, n + 64));
    HUTK_HIP_TRY(t->grow(&t->d_offs, &t->d_offs_cap, n_docs + 1));
    HUTK_HIP_TRY(t->grow(&t->d_wsb, &t->d_bm_cap, std::max(n_groups, n_bm) + 1));
    {
        int64_t c2 = 0;
        t->release(t->d_dbm);
        t->d_dbm = nullptr;
        HUTK_HIP_TRY(t->grow(&t->d_dbm, &c2, n_bm + 1));
    }
    HUTK_HIP_TRY(hipMemcpyAsync(t->d_bytes, bytes + base, n, hipMemcpyHostToDevice, st));
    HUTK_HIP_TRY(hipMemsetAsync(t->d_bytes + n, 0, 64, st));
    HUTK_HIP_TRY(hipMemcpyAsync(t->d_offs, offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, st));
    HUTK_HIP_TRY(hipMemsetAsync(t->d_dbm, 0, (n_bm + 1) * 4, st));
    HUTK_HIP_TRY(hipMemsetAsync(t->ctl, 0, sizeof(AddCtl), st));
    hipLaunchKernelGGL(k_docmark, dim3(nblocks(n_docs)), dim3(TB), 0, st, t->d_offs, n_docs, base, n, t->d_dbm);
    hipLaunchKernelGGL(k_split, dim3(nblocks(n_groups)), dim3(TB), 0, st, t->d_bytes, n, t->d_dbm, t->d_wsb, t->ctl);
    HUTK_HIP_TRY(hipGetLastError());
    AddCtl h;
    HUTK_HIP_TRY(hipMemcpyAsync(&h, t->ctl, sizeof h, hipMemcpyDeviceToHost, st));
    HUTK_HIP_TRY(hipStreamSynchronize(st));
    if (h.nul) return hutk::api_set_error(HUTK_E_NUL_BYTE, "hutk_trainer_add: a document holds a 0x00 byte");
    const int64_t nw = (int64_t)h.n_words;

    // room: arena for every byte of the batch, word table at load <= 1/2, a pending list per round
    if (t->arena_used + n > t->arena_cap) {
        const int64_t cap = std::max<int64_t>(t->arena_used + n, 2 * t->arena_cap);
        uint8_t* p = nullptr;
        HUTK_HIP_TRY(t->alloc((void**)&p, cap));
        if (t->arena_used) HUTK_HIP_TRY(hipMemcpyAsync(p, t->arena, t->arena_used, hipMemcpyDeviceToDevice, st));
        HUTK_HIP_TRY(hipStreamSynchronize(st));
        t->release(t->arena);
        t->arena = p;
        t->arena_cap = cap;
    }
    const uint64_t need = pow2_at_least((uint64_t)std::max<int64_t>(2 * (t->n_unique + nw), 1024));
    if (need > t->wt_cap) {
        WordTab nt{};
        HUTK_HIP_TRY(wordtab_alloc(t, &nt, need));
        if (t->wt_cap) {
            hipLaunchKernelGGL(k_word_rehash, dim3(nblocks(t->wt_cap)), dim3(TB), 0, st, t->wt, t->wt_cap, nt, t->ctl);
            t->c_word_rehash++;
        }
        HUTK_HIP_TRY(hipStreamSynchronize(st));
        wordtab_free(t, &t->wt);
        t->wt = nt;
        t->wt_cap = need;
    }
    HUTK_HIP_TRY(t->grow(&t->pend[0], &t->pend_cap, nw));
    {
        int64_t c1 = 0;
        t->release(t->pend[1]);
        t->pend[1] = nullptr;
        HUTK_HIP_TRY(t->grow(&t->pend[1], &c1, t->pend_cap));
    }
    // arena_used / n_unique continue from the earlier batches
    h = AddCtl{};
    h.arena_used = (unsigned long long)t->arena_used;
    h.n_unique = (unsigned long long)t->n_unique;
    HUTK_HIP_TRY(hipMemcpy(t->ctl, &h, sizeof h, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_insert, dim3(nblocks(n_groups)), dim3(TB), 0, st, t->d_bytes, n, t->d_wsb, t->wt, t->arena,
                       t->ctl, t->pend[0]);
    HUTK_HIP_TRY(hipGetLastError());
    int which = 0;
    for (int round = 0;; round++) {
        HUTK_HIP_TRY(hipMemcpyAsync(&h, t->ctl, sizeof h, hipMemcpyDeviceToHost, st));
        HUTK_HIP_TRY(hipStreamSynchronize(st));
        if (h.full) return hutk::api_set_error(HUTK_E_CAPACITY, "hutk_trainer_add: word table full");
        if (h.pend_n[which] == 0) break;
        if (round > 64) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_trainer_add: word insertion does not settle");
        t->c_deferred += h.pend_n[which];
        t->c_insert_rounds_max = std::max<int64_t>(t->c_insert_rounds_max, round + 1);
        HUTK_HIP_TRY(hipMemsetAsync(&t->ctl->pend_n[which ^ 1], 0, 4, st));
        hipLaunchKernelGGL(k_insert_pending, dim3(nblocks(h.pend_n[which])), dim3(TB), 0, st, t->d_bytes, t->wt,
                           t->arena, t->ctl, t->pend[which], which, t->pend[which ^ 1]);
        HUTK_HIP_TRY(hipGetLastError());
        HUTK_HIP_TRY(hipMemsetAsync(&t->ctl->pend_n[which], 0, 4, st));
        which ^= 1;
    }
    t->arena_used = (int64_t)h.arena_used;
    t->n_unique = (int64_t)h.n_unique;
    t->n_docs += n_docs;
    t->n_bytes += n;
    t->n_occ += nw;
    return HUTK_OK;
}

int hutk_trainer_run(hutk_trainer* t, int32_t n_merges, int32_t* pairs_out, int64_t* counts_out, int32_t* n_done) {
    if (!t || n_merges < 0 || (n_merges > 0 && !pairs_out) || !n_done)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_run: bad arguments");
    if (t->ran) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_run: run may be called once per trainer");
    t->ran = true;
    *n_done = 0;
    // test-only knobs (header comment); unset, they are SYNC_EVERY and PAIR_CAP_LOG2
    const char* e_sync = getenv("HUTK_TRAIN_SYNC_EVERY");
    const int64_t sync_every = e_sync && atoll(e_sync) >= 1 ? std::min<int64_t>(atoll(e_sync), INT32_MAX) : SYNC_EVERY;
    const char* e_cap = getenv("HUTK_TRAIN_PAIR_CAP_LOG2");
    const int cap_log2 = e_cap ? std::min(std::max(atoi(e_cap), 2), 30) : PAIR_CAP_LOG2;
    const uint64_t pair_floor = 1ull << cap_log2;
    if (int rc = symbolise(t)) return rc;
    HUTK_HIP_TRY(hipSetDevice(t->device));
    // every merge removes at least one symbol, so no more than n_sym merges can happen; symbol ids stay below 2^31
    n_merges = (int32_t)std::min<int64_t>({(int64_t)n_merges, t->n_sym, (int64_t)INT32_MAX - t->n_alpha});
    hipStream_t st = t->st;
    const int64_t n_words = t->n_unique, n_sym = t->n_sym;
    const int base = t->n_alpha;
    int32_t *sym = t->sym, *w_len = t->w_len, *act[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    int64_t *w_off = t->w_off, *w_cnt = t->w_cnt;
    unsigned int* cnt2 = nullptr;  // [0..1] active short / long, [3] short before the long list
    const int64_t nw1 = std::max<int64_t>(n_words, 1);
    for (int p = 0; p < 2; p++)
        for (int q = 0; q < 2; q++) HUTK_HIP_TRY(t->alloc((void**)&act[p][q], nw1 * 4));
    HUTK_HIP_TRY(t->alloc((void**)&cnt2, 16));
    HUTK_HIP_TRY(hipMemsetAsync(cnt2, 0, 16, st));

    // active lists (cur = 0): words with >= 2 symbols
    unsigned n_act[2] = {0, 0};
    int cur_list = 0;
    auto partition = [&](const int32_t* in, unsigned n_in, int dst) -> int {
        HUTK_HIP_TRY(hipMemsetAsync(cnt2, 0, 8, st));
        if (n_in)
            hipLaunchKernelGGL(k_partition, dim3(nblocks(n_in)), dim3(TB), 0, st, in, n_in, w_len, act[dst][0],
                               act[dst][1], cnt2);
        HUTK_HIP_TRY(hipGetLastError());
        HUTK_HIP_TRY(hipMemcpyAsync(n_act, cnt2, 8, hipMemcpyDeviceToHost, st));
        HUTK_HIP_TRY(hipStreamSynchronize(st));
        return HUTK_OK;
    };
    if (int rc = partition(nullptr, (unsigned)n_words, 0)) return rc;

    // pair table
    PairTab pt{};
    uint64_t pcap = 0;
    unsigned long long* d_used = nullptr;
    unsigned int* d_full = nullptr;
    HUTK_HIP_TRY(t->alloc((void**)&d_used, 8));
    HUTK_HIP_TRY(t->alloc((void**)&d_full, 4));
    HUTK_HIP_TRY(hipMemsetAsync(d_full, 0, 4, st));
    auto pair_alloc = [&](PairTab* p, uint64_t cap) -> hipError_t {
        hipError_t e;
        if ((e = t->alloc((void**)&p->key, cap * 8)) != hipSuccess) return e;
        if ((e = t->alloc((void**)&p->cnt, cap * 8)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(p->key, 0xFF, cap * 8, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(p->cnt, 0, cap * 8, st)) != hipSuccess) return e;
        p->mask = cap - 1;
        p->used = d_used;
        p->full = d_full;
        return hipMemsetAsync(d_used, 0, 8, st);
    };
    // initial keys: at most min(symbols, A^2) distinct pairs (65536 in bytes mode)
    pcap = pow2_at_least(std::max<uint64_t>(4 * std::min<int64_t>(n_sym, (int64_t)base * base), pair_floor));
    HUTK_HIP_TRY(pair_alloc(&pt, pcap));
    t->c_pcap_max = (int64_t)pcap;
    if (n_act[0])
        hipLaunchKernelGGL(k_init_short, dim3(nblocks(n_act[0])), dim3(TB), 0, st, sym, act[0][0], n_act[0], w_off, w_len,
                           w_cnt, pt);
    if (n_act[1])
        hipLaunchKernelGGL(k_init_long, dim3(nblocks((uint64_t)n_act[1] * 64)), dim3(TB), 0, st, sym, act[0][1], n_act[1],
                           w_off, w_len, w_cnt, pt);
    HUTK_HIP_TRY(hipGetLastError());
    unsigned long long used = 0;
    HUTK_HIP_TRY(hipMemcpyAsync(&used, d_used, 8, hipMemcpyDeviceToHost, st));
    HUTK_HIP_TRY(hipStreamSynchronize(st));
    t->n_pairs0 = (int64_t)used;

    int32_t* d_pairs = nullptr;
    int64_t* d_counts = nullptr;
    LoopCtl* lc = nullptr;
    Best* partial = nullptr;
    constexpr unsigned SEL_BLOCKS_MAX = 1024;
    HUTK_HIP_TRY(t->alloc((void**)&d_pairs, std::max<int64_t>(2LL * n_merges, 2) * 4));
    HUTK_HIP_TRY(t->alloc((void**)&d_counts, std::max<int64_t>(n_merges, 1) * 8));
    HUTK_HIP_TRY(t->alloc((void**)&lc, sizeof(LoopCtl)));
    HUTK_HIP_TRY(t->alloc((void**)&partial, SEL_BLOCKS_MAX * sizeof(Best)));
    HUTK_HIP_TRY(hipMemsetAsync(lc, 0, sizeof(LoopCtl), st));

    auto rebuild = [&](uint64_t live_hint, uint64_t room_hint) -> int {
        uint64_t cap = pow2_at_least(std::max<uint64_t>(4 * (live_hint + room_hint), pair_floor));
        PairTab nt{};
        PairTab old = pt;
        const uint64_t old_cap = pcap;
        // the new table's `used` counter is the same device word: reset after the old table is no longer read
        unsigned long long* used_new = nullptr;
        HUTK_HIP_TRY(t->alloc((void**)&used_new, 8));
        hipError_t e;
        if ((e = t->alloc((void**)&nt.key, cap * 8)) != hipSuccess) HUTK_HIP_TRY(e);
        if ((e = t->alloc((void**)&nt.cnt, cap * 8)) != hipSuccess) HUTK_HIP_TRY(e);
        HUTK_HIP_TRY(hipMemsetAsync(nt.key, 0xFF, cap * 8, st));
        HUTK_HIP_TRY(hipMemsetAsync(nt.cnt, 0, cap * 8, st));
        HUTK_HIP_TRY(hipMemsetAsync(used_new, 0, 8, st));
        nt.mask = cap - 1;
        nt.used = used_new;
        nt.full = d_full;
        hipLaunchKernelGGL(k_pair_rehash, dim3(nblocks(old_cap)), dim3(TB), 0, st, old, old_cap, nt);
        HUTK_HIP_TRY(hipGetLastError());
        HUTK_HIP_TRY(hipStreamSynchronize(st));
        t->release(old.key);
        t->release(old.cnt);
        t->release(d_used);
        d_used = used_new;
        pt = nt;
        t->c_rebuilds++;
        t->c_grows += cap > old_cap;
        t->c_shrinks += cap < old_cap;
        t->c_pcap_max = std::max<int64_t>(t->c_pcap_max, (int64_t)cap);
        pcap = cap;
        return HUTK_OK;
    };

    hipEvent_t ev0, ev1;
    HUTK_HIP_TRY(hipEventCreate(&ev0));
    HUTK_HIP_TRY(hipEventCreate(&ev1));
    HUTK_HIP_TRY(hipEventRecord(ev0, st));
    int k = 0;
    LoopCtl hl{};
    int rc = HUTK_OK;
    while (k < n_merges) {
        const unsigned sel_blocks = (unsigned)std::min<uint64_t>(SEL_BLOCKS_MAX, nblocks(pcap, TB * 4));
        const long long room = (long long)(pcap / 2);
        const int end = (int)std::min<int64_t>(n_merges, k + sync_every);
        t->c_sel_blocks_max = std::max<int64_t>(t->c_sel_blocks_max, sel_blocks);
        for (int j = k; j < end; j++) {
            hipLaunchKernelGGL(k_select, dim3(sel_blocks), dim3(TB), 0, st, pt, pcap, partial, lc, base, j, room,
                               d_pairs, d_counts);
            if (n_act[0])
                hipLaunchKernelGGL(k_apply_short, dim3(nblocks(n_act[0])), dim3(TB), 0, st, sym, act[cur_list][0],
                                   n_act[0], w_off, w_len, w_cnt, pt, lc, base, j);
            if (n_act[1])
                hipLaunchKernelGGL(k_apply_long, dim3(nblocks((uint64_t)n_act[1] * 64)), dim3(TB), 0, st, sym,
                                   act[cur_list][1], n_act[1], w_off, w_len, w_cnt, pt, lc, base, j);
        }
        HUTK_HIP_TRY(hipGetLastError());
        HUTK_HIP_TRY(hipMemcpyAsync(&hl, lc, sizeof hl, hipMemcpyDeviceToHost, st));
        unsigned full = 0;
        HUTK_HIP_TRY(hipMemcpyAsync(&full, d_full, 4, hipMemcpyDeviceToHost, st));
        HUTK_HIP_TRY(hipMemcpyAsync(&used, d_used, 8, hipMemcpyDeviceToHost, st));
        HUTK_HIP_TRY(hipStreamSynchronize(st));
        t->c_syncs++;
        t->c_pauses += hl.pause != 0;
        if (full) {
            rc = hutk::api_set_error(HUTK_E_CAPACITY, "hutk_trainer_run: pair table full");
            break;
        }
        k = hl.n_done;
        if (hl.stop) break;
        // drop finished words; swap the active lists
        const unsigned na0 = n_act[0], na1 = n_act[1];
        const int nxt = cur_list ^ 1;
        {
            HUTK_HIP_TRY(hipMemsetAsync(cnt2, 0, 8, st));
            if (na0)
                hipLaunchKernelGGL(k_partition, dim3(nblocks(na0)), dim3(TB), 0, st, act[cur_list][0], na0, w_len,
                                   act[nxt][0], act[nxt][1], cnt2);
            // (the short count before the long list goes in: cnt2[3], so that the host learns how many long words
            // became short from the same copy; short words never become long)
            if (na1) HUTK_HIP_TRY(hipMemcpyAsync(cnt2 + 3, cnt2, 4, hipMemcpyDeviceToDevice, st));
            if (na1)
                hipLaunchKernelGGL(k_partition, dim3(nblocks(na1)), dim3(TB), 0, st, act[cur_list][1], na1, w_len,
                                   act[nxt][0], act[nxt][1], cnt2);
            HUTK_HIP_TRY(hipGetLastError());
            unsigned n4[4] = {0, 0, 0, 0};
            HUTK_HIP_TRY(hipMemcpyAsync(n4, cnt2, na1 ? 16 : 8, hipMemcpyDeviceToHost, st));
            HUTK_HIP_TRY(hipStreamSynchronize(st));
            n_act[0] = n4[0], n_act[1] = n4[1];
            if (na1) t->c_long_to_short += n4[0] - n4[3];
            cur_list = nxt;
        }
        // the table: grow when a step paused, rebuild (dropping dead keys) when it is half used
        const long long sym_room = 2LL * (base + k) + 1;  // (the select kernel's bound; counts never grow)
        const uint64_t step_room = (uint64_t)(hl.n_done ? std::min<long long>(2 * hl.best_cnt, sym_room) : sym_room);
        // (k_select scans the whole table every merge: room for one worst-case step is enough, a step that does not
        // fit pauses and comes back here)
        if (hl.pause || used + 2 * step_room > pcap / 2 ||
            pcap > 16 * std::max<uint64_t>(used + step_room, pair_floor >> 2)) {
            if ((rc = rebuild(used, step_room))) break;
            HUTK_HIP_TRY(hipMemsetAsync(&lc->pause, 0, 4, st));
        }
    }
    HUTK_HIP_TRY(hipEventRecord(ev1, st));
    HUTK_HIP_TRY(hipEventSynchronize(ev1));
    float ms = 0;
    HUTK_HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    t->loop_us = (int64_t)(ms * 1000.0f);
    if (rc) return rc;
    HUTK_HIP_TRY(hipMemcpyAsync(&hl, lc, sizeof hl, hipMemcpyDeviceToHost, st));
    HUTK_HIP_TRY(hipStreamSynchronize(st));
    const int done = hl.n_done;
    if (done) {
        HUTK_HIP_TRY(hipMemcpy(pairs_out, d_pairs, (size_t)done * 8, hipMemcpyDeviceToHost));
        if (counts_out) HUTK_HIP_TRY(hipMemcpy(counts_out, d_counts, (size_t)done * 8, hipMemcpyDeviceToHost));
    }
    *n_done = done;
    // the workspace is returned now; stats stay readable
    for (auto& a : std::vector<std::pair<void*, int64_t>>(t->allocs))
        if (a.first != t->ctl) t->release(a.first);
    t->sym = t->w_len = nullptr;
    t->w_off = t->w_cnt = nullptr;
    return HUTK_OK;
}

int hutk_trainer_stats(const hutk_trainer* t, int64_t* out8) {
    if (!t || !out8) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_stats: bad arguments");
    const int64_t v[8] = {t->n_docs, t->n_bytes, t->n_occ, t->n_unique, t->symbolised ? t->n_sym : t->arena_used,
                          t->n_pairs0, t->peak, t->loop_us};
    memcpy(out8, v, sizeof v);
    return HUTK_OK;
}

int hutk_trainer_debug_counters(const hutk_trainer* t, int64_t* out, int n) {
    if (!t || n < 0 || (n > 0 && !out)) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_debug_counters: bad arguments");
    const int64_t v[] = {t->c_pauses,        t->c_grows,         t->c_shrinks,      t->c_rebuilds,
                         t->c_syncs,         t->c_pcap_max,      t->c_sel_blocks_max, t->c_word_rehash,
                         t->c_deferred,      t->c_insert_rounds_max, t->c_long_to_short, t->c_dropped,
                         t->c_cset_grows};
    const int nv = (int)(sizeof v / sizeof v[0]);
    if (n > 0) memcpy(out, v, sizeof(int64_t) * std::min(n, nv));
    return HUTK_OK;
}

int hutk_trainer_alphabet(hutk_trainer* t, uint8_t* bytes_out, int64_t bytes_cap, int64_t* offsets_out,
                          int64_t offsets_cap, int64_t* n_symbols, int64_t* n_bytes) {
    if (!t) return hutk::api_set_error(HUTK_E_ARG, "hutk_trainer_alphabet: bad arguments");
    if (int rc = symbolise(t)) return rc;
    std::vector<uint8_t> b;
    std::vector<int64_t> o{0};
    for (int32_t i = 0; i < t->n_alpha; i++) {
        if (t->mode == HUTK_TRAIN_BYTES) {
            b.push_back((uint8_t)i);
        } else {
            for (int q = 3; q >= 0; q--)
                if (const uint8_t c = (uint8_t)(t->alpha[i] >> (8 * q))) b.push_back(c);
        }
        o.push_back((int64_t)b.size());
    }
    if (n_symbols) *n_symbols = t->n_alpha;
    if (n_bytes) *n_bytes = (int64_t)b.size();
    if (!bytes_out || !offsets_out) return HUTK_OK;
    if (bytes_cap < (int64_t)b.size() || offsets_cap < (int64_t)o.size())
        return hutk::api_set_error(HUTK_E_CAPACITY, "hutk_trainer_alphabet: the buffers are too small");
    if (!b.empty()) memcpy(bytes_out, b.data(), b.size());
    memcpy(offsets_out, o.data(), o.size() * sizeof(int64_t));
    return HUTK_OK;
}

void hutk_trainer_destroy(hutk_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->st) (void)hipStreamSynchronize(t->st);
    for (auto& a : std::vector<std::pair<void*, int64_t>>(t->allocs)) t->release(a.first);
    if (t->st) (void)hipStreamDestroy(t->st);
    delete t;
}

}  // extern "C"
