// hutk_unigram_seed.h -- making the seed of a Unigram training on the GPU (include/hutoken_amd.h states the rule; DESIGN.md
// section 8n.3): the unique words of a corpus, their characters, and every substring of 2 .. 16 characters that has two
// distinct followers, with frequency x characters as its score.  hutk_unigram.hip includes it behind hutk_unigram_train.h:
// the check, the flags, the fold, the chunks and the word queue are that file's; a seeder owns a hutk_unigram handle with a
// one-line vocabulary for them, so nothing the encoder's kernels compile to changes.
//
//   k_ugs_insert   a workgroup a chunk of the folded text.  A lane takes a word of the chunk's queue: up to SHORT_WORD bytes
//                  it hashes, probes and compares alone; a longer one goes to a queue in LDS, and the wavefronts take those
//                  behind a barrier, 64 bytes a trip (length, hash, compare).  A word has no length limit.
//   k_ugs_settle   a wavefront a word that is new in this round: its index, its place in the arena, its bytes behind a 0x00
//   k_ugs_pending  a wavefront a word that found the table at its limit, after the host has grown it
//   k_ugs_rehash   a lane a unique word, into the grown table
//   k_ugs_chars    a wavefront a unique word: count[character] += n_w
//   k_ugs_words    the words' starts, lengths and counts, for the caller
//   k_ugs_count    THE HOT KERNEL: a workgroup a tile of the arena, staged in LDS with the halo; a lane a character start;
//                  all lanes step through the lengths 2 .. L together, a table probe each
//   k_ugs_compact  a lane a table slot: the candidates as (score, position, byte length)
//   k_ugs_gather   a lane a chosen string, into the packed blob
//
// THE UNIQUE-WORD TABLE.  hutk_train.hip's protocol (claim a slot by compare-and-swap on the hash, copy the bytes, publish,
// defer whoever meets a claimed slot that is not published yet to a next round, each round a host round trip) is not shared:
// a slot here is ONE 64-bit claim word -- a tag of the hash, and either the index of a word of an earlier round or, with
// NEW_BIT, the position of the claiming occurrence IN THE FOLDED TEXT OF THIS BATCH.  That text is read-only while the
// kernel runs, so whoever meets such a slot compares against it at once: nothing is deferred and nothing spins.
// k_ugs_settle then moves the new words into the arena and turns their claim words into index + 1 (never 0, which is
// empty).  Growth: the slots in use are checked before a claim and counted behind one that won; at the table's limit (half
// its slots; the lanes in flight may pass it by their number) an occurrence goes to a pending list instead.  The host reads
// the counters once per call, grows table and records when something is pending, rehashes and runs the pending list: no
// occurrence of the batch is lost.  The call waits for that read, and once more for every reallocation (table, records,
// arena).  The table stops at 2^32 slots: the list of a round's new slots is 32 bits wide.  hutk_train.hip is left as it stands.
//
// THE SUBSTRING TABLE.  claim[slot] (64 bits) = tag:14 | characters - 1:4 | bytes - 1:6 | arena position:40 of the first
// occurrence to arrive; the key's bytes are the arena's at that position, so there is no key store, and the arena is
// read-only in this pass.  A lane compares the arena's bytes with its own in LDS.  freq[slot] and fol[slot] are 32 bits
// each: fol is 0 (empty), follower + 1, or MANY, which is final.  Keys already present are found by loads; only an empty
// slot sees a compare-and-swap, behind the same check of the slots in use: at the limit the pass sets `full` and ends,
// and the host runs it again from the arena with twice the slots.  freq is counted by plain global atomics: the E-step's
// accumulator in LDS, keyed by the slot's index, measured the same (1 029.5 ms against 1 025.9 ms) and was dropped.
#pragma once

namespace {

constexpr int SHORT_WORD = 64;                 // bytes a lane takes alone
constexpr uint64_t W_NEW_BIT = 1ull << 40, W_VAL_MASK = W_NEW_BIT - 1;  // the word table's claim word: tag:23 | new:1 | value:40
constexpr int64_t UGS_MIN_SLOTS = 1 << 12;
constexpr int SEED_TILE = 2048, SEED_HALO = 64, SEED_BACK = 4, SEED_MAX_CHARS = 16;
constexpr int SEED_STAGE = SEED_BACK + SEED_TILE + SEED_HALO + 8;  // the halo, the follower's 4 bytes, 4 more for its decode
constexpr uint32_t FOL_MANY = 0xFFFFFFFFu;
constexpr int64_t SEED_COUNTS = 0x110000 + 256;  // the code points, then the bytes that are no UTF-8

struct SeedRec {  // a unique word
    int64_t off, len;  // in the arena; arena[off - 1] == 0
    unsigned long long cnt, hash;
};

struct SeedCtl {
    unsigned long long n_words;     // occurrences so far
    unsigned long long n_unique;
    unsigned long long arena_used;  // the arena holds every word behind a 0x00, and nothing but 0x00 beyond its use
    unsigned long long used;        // slots of the word table in use
    unsigned int n_new, n_pend[2];
    unsigned int bad;               // an index past a list's capacity: never expected
};

struct SeedTab {
    unsigned long long* claim;     // 0: empty
    unsigned long long* slot_cnt;  // occurrences of a word that is new in this round
    uint64_t mask, limit;
};

struct InsArgs {
    U::Text f;  // f.n: the folded text's size
    SeedTab T;
    SeedRec* rec;
    const uint8_t* arena;
    SeedCtl* ctl;
    uint32_t* fresh;  // slots claimed in this round
    int64_t* pend;    // positions that found the table at its limit
    int which;        // the pending list's counter
    int64_t list_cap;
};

__device__ __forceinline__ uint64_t ugs_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ x >> 31;
}
// a word's hash: up to SHORT_WORD bytes one chain, a longer word 64 interleaved chains (lane l: bytes l, l + 64, ..)
// combined in lane order; which form a word takes follows from its length alone
__device__ __forceinline__ uint64_t ugs_hash_short(const uint8_t* w, int len) {
    uint64_t h = 0xCBF29CE484222325ull ^ (uint64_t)len;
    for (int i = 0; i < len; i++) h = (h ^ w[i]) * 0x100000001B3ull;
    return ugs_mix(h);
}
__device__ __forceinline__ uint64_t ugs_hash_long(const uint8_t* w, int64_t len, int lane) {
    uint64_t h = 0xCBF29CE484222325ull ^ (uint64_t)len ^ ((uint64_t)lane << 56);
    for (int64_t i = lane; i < len; i += 64) h = (h ^ w[i]) * 0x100000001B3ull;
    h = ugs_mix(h);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) h += __shfl_xor(h, d);  // (a sum: every lane ends with the same value)
    return ugs_mix(h);
}
__device__ __forceinline__ uint64_t ugs_tag(uint64_t h) { return (h >> 41) << 41; }

// the word of the folded text at p is the len bytes at w
__device__ __forceinline__ bool ugs_same_text(const U::Text& f, int64_t p, const uint8_t* w, int64_t len) {
    if (p + len > f.n || !U::word_ends(f, p + len)) return false;
    for (int64_t i = 0; i < len; i++)
        if (f.bytes[p + i] != w[i] || (i > 0 && U::word_ends(f, p + i))) return false;
    return true;
}

__device__ __forceinline__ void ugs_to_pending(const InsArgs& a, int64_t q) {
    const unsigned i = atomicAdd(&a.ctl->n_pend[a.which], 1u);
    if ((int64_t)i < a.list_cap) a.pend[i] = q;
    else atomicOr(&a.ctl->bad, 1u);
}

// One occurrence, by one lane (words of up to SHORT_WORD bytes) or, with WAVE, by a wavefront whose lanes all call this with
// the same arguments.  The slot's word is read by loads; only an empty slot sees a compare-and-swap.
template <bool WAVE>
__device__ __forceinline__ void ugs_insert(const InsArgs& a, int64_t q, int64_t len, uint64_t h, int lane) {
    const uint8_t* w = a.f.bytes + q;
    const uint64_t tag = ugs_tag(h);
    uint64_t s = h & a.T.mask;
    for (uint64_t probe = 0; probe <= a.T.mask; probe++, s = (s + 1) & a.T.mask) {
        unsigned long long c = 0;
        if (!WAVE || lane == 0) {
            c = __hip_atomic_load(&a.T.claim[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c == 0) {  // the word is not in the table.  The slots in use are checked before the claim and counted behind a
                           // claim that won, so a race for one word counts once; what the lanes in flight add past the limit
                           // is bounded by their number, and a table they fill sends the rest to the pending list as well
                if (__hip_atomic_load(&a.ctl->used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.T.limit) {
                    c = ~0ull;
                } else {
                    const unsigned long long mine = tag | W_NEW_BIT | (unsigned long long)q;
                    c = atomicCAS(&a.T.claim[s], 0ull, mine);
                    if (c == 0) {
                        atomicAdd(&a.ctl->used, 1ull);
                        const unsigned i = atomicAdd(&a.ctl->n_new, 1u);
                        if ((int64_t)i < a.list_cap) a.fresh[i] = (uint32_t)s;
                        else atomicOr(&a.ctl->bad, 1u);
                        c = mine;
                    }
                }
            }
        }
        if (WAVE) c = __shfl(c, 0);
        if (c == ~0ull) {  // the table is at its limit: the host grows it and this occurrence comes again
            if (!WAVE || lane == 0) ugs_to_pending(a, q);
            return;
        }
        if (ugs_tag(c) != tag) continue;
        const int64_t v = (int64_t)(c & W_VAL_MASK) - ((c & W_NEW_BIT) ? 0 : 1);  // (a settled claim holds the index + 1: never 0)
        bool same;
        if (c & W_NEW_BIT) {
            if (v == q) {
                same = true;
            } else if (!WAVE) {
                same = ugs_same_text(a.f, v, w, len);
            } else {
                bool diff = v + len > a.f.n || !U::word_ends(a.f, v + len);
                for (int64_t i = lane; i < len && !diff; i += 64) diff = a.f.bytes[v + i] != w[i] || (i > 0 && U::word_ends(a.f, v + i));
                same = !__any(diff);
            }
            if (same && (!WAVE || lane == 0)) atomicAdd(&a.T.slot_cnt[s], 1ull);
        } else {
            const SeedRec r = a.rec[v];
            same = r.len == len && r.hash == h;
            if (same) {
                const uint8_t* k = a.arena + r.off;
                bool diff = false;
                for (int64_t i = WAVE ? lane : 0; i < len && !diff; i += WAVE ? 64 : 1) diff = k[i] != w[i];
                same = WAVE ? !__any(diff) : !diff;
            }
            if (same && (!WAVE || lane == 0)) atomicAdd(&a.rec[v].cnt, 1ull);
        }
        if (same) return;
    }
    if (!WAVE || lane == 0) ugs_to_pending(a, q);  // every slot is taken
}

// the bytes of the word that starts at q, by a wavefront
__device__ __forceinline__ int64_t ugs_word_len_wave(const U::Text& f, int64_t q, int lane) {
    for (int64_t base = 1;; base += 64) {
        const uint64_t em = __ballot(U::word_ends(f, q + base + lane));
        if (em) return base + __ffsll((unsigned long long)em) - 1;
    }
}

__device__ __forceinline__ void ugs_insert_wave(const InsArgs& a, int64_t q, int lane) {
    const int64_t len = ugs_word_len_wave(a.f, q, lane);
    if (len <= SHORT_WORD) {
        if (lane == 0) ugs_insert<false>(a, q, len, ugs_hash_short(a.f.bytes + q, (int)len), 0);
    } else {
        ugs_insert<true>(a, q, len, ugs_hash_long(a.f.bytes + q, len, lane), lane);
    }
}

__global__ __launch_bounds__(TB) void k_ugs_insert(InsArgs a, const int64_t* n_dev, const int32_t* ok) {
    __shared__ int s_part[TB / 64];
    __shared__ int s_n_long;
    __shared__ uint16_t s_ws[U::CHUNK_BYTES];
    __shared__ uint16_t s_long[U::CHUNK_BYTES];
    if (!*ok) return;
    a.f.n = *n_dev;
    const int64_t c0 = (int64_t)blockIdx.x * U::CHUNK_BYTES;
    if (c0 >= a.f.n) return;
    const int tid = threadIdx.x;
    if (tid == 0) s_n_long = 0;
    const int n_words = list_words(a.f, c0, s_part, s_ws);  // (its barriers stand behind s_n_long = 0)
    __syncthreads();  // the queue is whole
    for (int i = tid; i < n_words; i += TB) {
        const int64_t q = c0 + s_ws[i];
        int len = 1;
        while (len <= SHORT_WORD && !U::word_ends(a.f, q + len)) len++;
        if (len > SHORT_WORD) s_long[atomicAdd(&s_n_long, 1)] = s_ws[i];
        else ugs_insert<false>(a, q, len, ugs_hash_short(a.f.bytes + q, len), 0);
    }
    if (tid == 0 && n_words) atomicAdd(&a.ctl->n_words, (unsigned long long)n_words);
    __syncthreads();
    const int n_long = s_n_long, lane = tid & 63;
    for (int i = tid >> 6; i < n_long; i += TB / 64) ugs_insert_wave(a, c0 + s_long[i], lane);
}

__global__ __launch_bounds__(TB) void k_ugs_pending(InsArgs a, const int64_t* n_dev, const int64_t* pin, int which_in) {
    a.f.n = *n_dev;
    const unsigned n_in = a.ctl->n_pend[which_in];
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6); i < (int64_t)n_in && i < a.list_cap; i += (int64_t)gridDim.x * (TB / 64))
        ugs_insert_wave(a, pin[i], lane);
}

// The words that are new in this round: a wavefront each.  (The round's inserts have ended: every count is whole.)
__global__ __launch_bounds__(TB) void k_ugs_settle(InsArgs a, const int64_t* n_dev, uint8_t* arena, int64_t arena_cap, int64_t rec_cap) {
    a.f.n = *n_dev;
    const int64_t n_new = a.ctl->n_new < (unsigned)a.list_cap ? a.ctl->n_new : a.list_cap;
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6); i < n_new; i += (int64_t)gridDim.x * (TB / 64)) {
        const uint64_t s = a.fresh[i];
        const unsigned long long c = a.T.claim[s];
        const int64_t q = (int64_t)(c & W_VAL_MASK);
        const int64_t len = ugs_word_len_wave(a.f, q, lane);
        const uint8_t* w = a.f.bytes + q;
        uint64_t h = len <= SHORT_WORD ? ugs_hash_short(w, (int)len) : ugs_hash_long(w, len, lane);
        long long idx = 0, o = 0;
        if (lane == 0) {
            idx = (long long)atomicAdd(&a.ctl->n_unique, 1ull);
            o = (long long)atomicAdd(&a.ctl->arena_used, (unsigned long long)len + 1);
        }
        idx = __shfl(idx, 0), o = __shfl(o, 0);
        if (idx >= rec_cap || o + len + 1 > arena_cap) {  // (the host sizes both for the round: never expected)
            if (lane == 0) atomicOr(&a.ctl->bad, 4u);
            continue;
        }
        for (int64_t j = lane; j < len; j += 64) arena[o + 1 + j] = w[j];  // (arena[o] is 0: the arena is zeroed beyond its use)
        if (lane == 0) {
            a.rec[idx] = SeedRec{o + 1, len, a.T.slot_cnt[s], h};
            a.T.slot_cnt[s] = 0;
            a.T.claim[s] = ugs_tag(h) | (unsigned long long)(idx + 1);
        }
    }
}

__global__ __launch_bounds__(TB) void k_ugs_rehash(const SeedRec* rec, int64_t n, SeedTab T, SeedCtl* ctl) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = rec[i].hash;
    uint64_t s = h & T.mask;
    for (uint64_t probe = 0; probe <= T.mask; probe++, s = (s + 1) & T.mask)
        if (atomicCAS(&T.claim[s], 0ull, ugs_tag(h) | (unsigned long long)(i + 1)) == 0) return;
    atomicOr(&ctl->bad, 8u);
}

// the controls between two rounds: the new words are settled; a rehashed table holds the unique words and nothing else
__global__ void k_ugs_round(SeedCtl* ctl, int keep_pending, int rehashed) {
    ctl->n_new = 0;
    ctl->n_pend[keep_pending ^ 1] = 0;
    if (rehashed) ctl->used = ctl->n_unique;
}

// ---- characters ----
__global__ __launch_bounds__(TB) void k_ugs_chars(const SeedRec* rec, int64_t n, const uint8_t* arena, unsigned long long* count) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * (TB / 64)) {
        const SeedRec r = rec[i];
        const uint8_t* w = arena + r.off;
        for (int64_t p = lane; p < r.len; p += 64) {
            const uint32_t b = w[p];
            if (b == 0 || !char_starts(w, p, r.len)) continue;
            uint32_t cp = 0;
            const int cl = hutk::norm::decode(w, p, r.len, &cp);
            atomicAdd(&count[cl ? cp : 0x110000u + b], r.cnt);
        }
    }
}

__global__ __launch_bounds__(TB) void k_ugs_words(const SeedRec* rec, int64_t n, int64_t* start, int64_t* len, int64_t* cnt) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    start[i] = rec[i].off, len[i] = rec[i].len, cnt[i] = (int64_t)rec[i].cnt;
}

// ---- substrings ----
struct SubTab {
    unsigned long long* claim;
    uint32_t* freq;
    uint32_t* fol;
    uint64_t mask, limit;
    unsigned long long* info;  // [0] full, [1] slots in use, [2] the candidates (k_ugs_compact)
};

__device__ __forceinline__ void ugs_follow(uint32_t* at, uint32_t f) {
    uint32_t o = __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o == FOL_MANY || o == f) return;
    if (o == 0) {
        o = atomicCAS(at, 0u, f);
        if (o == 0 || o == f) return;
    }
    __hip_atomic_store(at, FOL_MANY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the substring own[0 .. len) of n_chars characters, first seen at arena position pos, with the follower word f
__device__ __forceinline__ void ugs_sub_add(const SubTab& T, const uint8_t* arena, const uint8_t* own, int64_t pos, int len, int n_chars,
                                            uint32_t h, uint32_t f) {
    const unsigned long long head = ((unsigned long long)(h >> 18) << 50) | ((unsigned long long)(n_chars - 1) << 46) |
                                    ((unsigned long long)(len - 1) << 40);
    const unsigned long long mine = head | (unsigned long long)pos;
    uint64_t s = (ugs_mix(h) >> 7) & T.mask;
    for (uint64_t probe = 0; probe <= T.mask; probe++, s = (s + 1) & T.mask) {
        unsigned long long c = __hip_atomic_load(&T.claim[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0) {  // (the slots in use: checked before the claim, counted behind one that won, as the word table's)
            if (__hip_atomic_load(&T.info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= T.limit) {
                T.info[0] = 1;
                return;
            }
            c = atomicCAS(&T.claim[s], 0ull, mine);
            if (c == 0) {
                atomicAdd(&T.info[1], 1ull);
                c = mine;
            }
        }
        if ((c >> 40) != (head >> 40)) continue;
        if (c != mine) {
            const uint8_t* k = arena + (int64_t)(c & W_VAL_MASK);
            int i = 0;
            while (i < len && k[i] == own[i]) i++;
            if (i < len) continue;
        }
        atomicAdd(&T.freq[s], 1u);
        ugs_follow(&T.fol[s], f);
        return;
    }
    T.info[0] = 1;
}

__global__ __launch_bounds__(TB) void k_ugs_count(const uint8_t* arena, int64_t n_arena, int max_chars, const SubTab T) {
    __shared__ uint8_t s_b[SEED_STAGE];
    __shared__ uint8_t s_len[SEED_STAGE];  // the length of the character that starts here; 0: none does, or a 0x00
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * SEED_TILE, g0 = t0 - SEED_BACK;
    for (int i = tid; i < SEED_STAGE; i += TB) {
        const int64_t g = g0 + i;
        s_b[i] = g >= 0 && g < n_arena ? arena[g] : 0;
    }
    __syncthreads();
    constexpr int LEN_END = SEED_BACK + SEED_TILE + SEED_HALO + 1;  // the last follower starts at SEED_TILE - 1 + SEED_HALO
    for (int i = SEED_BACK + tid; i < LEN_END; i += TB) {
        const uint32_t b = s_b[i];
        int len = 0;
        if (b != 0) {
            bool starts = (b & 0xC0u) != 0x80u;
            if (!starts) {
                starts = true;
                for (int j = 1; j <= 3; j++)
                    if ((s_b[i - j] & 0xC0u) != 0x80u) {
                        uint32_t cp;
                        const int cl = hutk::norm::decode(s_b, i - j, SEED_STAGE, &cp);
                        starts = (cl ? cl : 1) <= j;
                        break;
                    }
            }
            if (starts) {
                uint32_t cp;
                len = hutk::norm::decode(s_b, i, SEED_STAGE, &cp);
                if (!len) len = 1;
            }
        }
        s_len[i] = (uint8_t)len;
    }
    __syncthreads();
    for (int i = SEED_BACK + tid; i < SEED_BACK + SEED_TILE; i += TB) {
        if (!s_len[i] || g0 + i >= n_arena) continue;
        if (__hip_atomic_load(&T.info[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;  // the table is full: the pass is run again
        uint32_t h = U::HASH_INIT;
        int cur = i;
        for (int k = 1; k <= max_chars; k++) {  // every lane of the wavefront is at its k-th character: 64 probes in flight
            const int cl = s_len[cur];
            if (!cl) break;
            for (int j = 0; j < cl; j++) h = U::hash_step(h, s_b[cur + j]);
            cur += cl;
            if (k < 2) continue;
            uint32_t f = 0;
            for (int j = 0, fl = s_len[cur]; j < fl; j++) f = f << 8 | s_b[cur + j];
            ugs_sub_add(T, arena, s_b + i, g0 + i, cur - i, k, U::hash_end(h), f + 1);
        }
    }
}

__global__ __launch_bounds__(TB) void k_ugs_compact(const SubTab T, int64_t n_slots, int64_t cap, int64_t* score, int64_t* pos, int32_t* len) {
    const int64_t s = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= n_slots) return;
    const unsigned long long c = T.claim[s];
    if (c == 0 || T.fol[s] != FOL_MANY) return;
    const int64_t i = (int64_t)atomicAdd(&T.info[2], 1ull);
    if (i >= cap) return;
    score[i] = (int64_t)T.freq[s] * (int64_t)(((c >> 46) & 15u) + 1);
    pos[i] = (int64_t)(c & W_VAL_MASK);
    len[i] = (int32_t)((c >> 40) & 63u) + 1;
}

__global__ __launch_bounds__(TB) void k_ugs_gather(const uint8_t* arena, int64_t n_arena, const int64_t* pos, const int32_t* len,
                                                   const int64_t* dst, int64_t n, uint8_t* blob, int64_t blob_cap) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i], d = dst[i];
    const int l = len[i];
    if (p < 0 || l < 0 || p + l > n_arena || d < 0 || d + l > blob_cap) return;
    for (int j = 0; j < l; j++) blob[d + j] = arena[p + j];
}

template <class T>
hipError_t ugs_grow(T** p, int64_t* cap, int64_t want, int64_t keep, hipStream_t st) {  // zeroed beyond what is kept
    if (want <= *cap) return hipSuccess;
    want += want / 4 + 256;
    T* q = nullptr;
    hipError_t e = hipMalloc((void**)&q, (size_t)want * sizeof(T));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(q, 0, (size_t)want * sizeof(T), st);
    if (e == hipSuccess && keep && *p) e = hipMemcpyAsync(q, *p, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (*p) (void)hipFree(*p);
    *p = q, *cap = want;
    return e;
}

}  // namespace

struct hutk_ugseed {
    hutk_unigram* front = nullptr;  // the fold and the word queue: a handle with a one-line vocabulary
    int device = 0;
    uint8_t* arena = nullptr;
    SeedRec* rec = nullptr;
    unsigned long long *claim = nullptr, *slot_cnt = nullptr;
    int64_t arena_cap = 0, rec_cap = 0, n_slots = 0;
    SeedCtl* ctl = nullptr;
    SeedCtl* h_ctl = nullptr;  // page-locked
    int64_t n_unique = 0, n_words = 0, arena_used = 0, grows = 0;
    DevBuf<int64_t> pend1;
    // the substring table of the last hutk_ugseed_count_device
    DevBuf<unsigned long long> s_claim, s_info;
    DevBuf<uint32_t> s_freq, s_fol;
    int64_t s_slots = 0;
    std::mutex mu;
};

namespace {

int ugs_table(hutk_ugseed* h, int64_t slots, hipStream_t st) {  // a new, empty word table
    HUTK_HIP_TRY(hipStreamSynchronize(st));
    if (h->claim) (void)hipFree(h->claim);
    if (h->slot_cnt) (void)hipFree(h->slot_cnt);
    h->claim = h->slot_cnt = nullptr;
    HUTK_HIP_TRY(hipMalloc((void**)&h->claim, (size_t)slots * 8));
    HUTK_HIP_TRY(hipMalloc((void**)&h->slot_cnt, (size_t)slots * 8));
    HUTK_HIP_TRY(hipMemsetAsync(h->claim, 0, (size_t)slots * 8, st));
    HUTK_HIP_TRY(hipMemsetAsync(h->slot_cnt, 0, (size_t)slots * 8, st));
    h->n_slots = slots;
    HUTK_HIP_TRY(ugs_grow(&h->rec, &h->rec_cap, slots + 1, h->n_unique, st));  // (the lanes in flight may pass the limit)
    return HUTK_OK;
}

unsigned ugs_wave_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + TB / 64 - 1) / (TB / 64) + 1, 1 << 16); }

}  // namespace

extern "C" {

void hutk_ugseed_destroy(hutk_ugseed* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->front) hutk_unigram_destroy(h->front);
    if (h->arena) (void)hipFree(h->arena);
    if (h->rec) (void)hipFree(h->rec);
    if (h->claim) (void)hipFree(h->claim);
    if (h->slot_cnt) (void)hipFree(h->slot_cnt);
    if (h->ctl) (void)hipFree(h->ctl);
    if (h->h_ctl) (void)hipHostFree(h->h_ctl);
    h->pend1.release(); h->s_claim.release(); h->s_info.release(); h->s_freq.release(); h->s_fol.release();
    delete h;
}

int hutk_ugseed_create(hutk_ugseed** out, int device, uint32_t flags) {
    if (!out) return hutk::api_set_error(HUTK_E_ARG, "hutk_ugseed_create: out is NULL");
    *out = nullptr;
    const uint8_t line[] = "<unk>";
    const int64_t offs[2] = {0, 5};
    const double score = 0.0;
    hutk_unigram* front = nullptr;
    if (int rc = hutk_unigram_create(&front, device, line, offs, &score, 1, 0, flags)) return rc;
    hutk_ugseed* h = new hutk_ugseed();
    h->front = front, h->device = front->device;
    hipError_t e = hipMalloc((void**)&h->ctl, sizeof(SeedCtl));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_ctl, sizeof(SeedCtl), hipHostMallocDefault);
    if (e == hipSuccess) {
        *h->h_ctl = SeedCtl{};
        e = hipMemcpy(h->ctl, h->h_ctl, sizeof(SeedCtl), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        hutk_ugseed_destroy(h);
        return hutk::api_set_error(e == hipErrorOutOfMemory ? HUTK_E_MEMORY : HUTK_E_DEVICE, std::string("hutk_ugseed_create: ") + hipGetErrorString(e));
    }
    *out = h;
    return HUTK_OK;
}

int hutk_ugseed_info(const hutk_ugseed* h, int64_t* out8) {
    if (!h || !out8) return hutk::api_set_error(HUTK_E_ARG, "hutk_ugseed_info: bad arguments");
    out8[0] = h->n_unique, out8[1] = h->n_words, out8[2] = h->arena_used, out8[3] = h->n_slots;
    out8[4] = h->grows, out8[5] = SEED_TILE, out8[6] = SEED_HALO, out8[7] = h->s_slots;
    return HUTK_OK;
}

int hutk_ugseed_add_device(hutk_ugseed* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes, int32_t* d_err,
                           void* hip_stream) {
    const std::string who = "hutk_ugseed_add_device";
    if (!h) return hutk::api_set_error(HUTK_E_ARG, who + ": the handle is NULL");
    if (n_docs < 0 || n_bytes < 0 || !d_offsets || (n_bytes > 0 && !d_bytes)) return hutk::api_set_error(HUTK_E_ARG, who + ": bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    std::lock_guard<std::mutex> front_lock(h->front->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    MatchArgs m;
    int64_t chunks = 0;
    if (int rc = ug_front(h->front, d_bytes, d_offsets, n_docs, n_bytes, false, d_err, st, who, m, chunks)) return rc;
    if (!chunks) return ug_back(h->front, st);
    const int64_t cap_f = n_bytes + n_docs;
    if (cap_f >= (int64_t)W_VAL_MASK || cap_f > (int64_t)UINT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, who + ": the batch is too large");
    if (!h->n_slots)
        if (int rc = ugs_table(h, UGS_MIN_SLOTS, st)) return rc;
    HUTK_HIP_TRY(ugs_grow(&h->arena, &h->arena_cap, h->arena_used + 2 * cap_f + 256, h->arena_used, st));  // every word new, a 0x00 each
    InsArgs a;
    a.f = m.f, a.rec = h->rec, a.arena = h->arena, a.ctl = h->ctl;
    a.T = SeedTab{h->claim, h->slot_cnt, (uint64_t)h->n_slots - 1, (uint64_t)h->n_slots / 2};
    a.fresh = reinterpret_cast<uint32_t*>(h->front->w_tmp.p), a.pend = reinterpret_cast<int64_t*>(h->front->w_bp.p), a.which = 0, a.list_cap = cap_f + 1;
    hipLaunchKernelGGL(k_ugs_insert, dim3((unsigned)chunks), dim3(TB), 0, st, a, m.n_dev, m.ok);
    for (int round = 0;; round++) {
        hipLaunchKernelGGL(k_ugs_settle, dim3(ugs_wave_blocks(cap_f)), dim3(TB), 0, st, a, m.n_dev, h->arena, h->arena_cap, h->rec_cap);
        HUTK_HIP_TRY(hipGetLastError());
        HUTK_HIP_TRY(hipMemcpyAsync(h->h_ctl, h->ctl, sizeof(SeedCtl), hipMemcpyDeviceToHost, st));
        HUTK_HIP_TRY(hipStreamSynchronize(st));  // the call's one wait: the table's growth is the host's
        const SeedCtl c = *h->h_ctl;
        if (c.bad) return hutk::api_set_error(HUTK_E_DEVICE, who + ": the word table's lists overflowed");
        h->n_unique = (int64_t)c.n_unique, h->arena_used = (int64_t)c.arena_used;
        const int64_t n_pend = c.n_pend[a.which];
        if (!n_pend) {
            h->n_words = (int64_t)c.n_words;
            hipLaunchKernelGGL(k_ugs_round, dim3(1), dim3(1), 0, st, h->ctl, 0, 0);
            hipLaunchKernelGGL(k_ugs_round, dim3(1), dim3(1), 0, st, h->ctl, 1, 0);
            break;
        }
        if (round > 40) return hutk::api_set_error(HUTK_E_DEVICE, who + ": the word table does not settle");
        // the pending occurrences may all be new words: a table that holds them at a quarter
        int64_t slots = h->n_slots * 2;
        while (slots < 4 * (h->n_unique + n_pend)) slots *= 2;
        if (slots > (1ll << 32)) return hutk::api_set_error(HUTK_E_UNSUPPORTED, who + ": too many unique words (the word table stops at 2^32 slots)");
        if (int rc = ugs_table(h, slots, st)) return rc;
        h->grows++;
        a.rec = h->rec;
        a.T = SeedTab{h->claim, h->slot_cnt, (uint64_t)slots - 1, (uint64_t)slots / 2};
        if (h->n_unique) hipLaunchKernelGGL(k_ugs_rehash, dim3(blocks_for(h->n_unique)), dim3(TB), 0, st, h->rec, h->n_unique, a.T, h->ctl);
        const int in = a.which;
        const int64_t* pin = a.pend;
        if (in == 0) {
            HUTK_HIP_TRY(h->pend1.reserve((size_t)cap_f + 1));
            a.pend = h->pend1.p;
        } else {
            a.pend = reinterpret_cast<int64_t*>(h->front->w_bp.p);
        }
        a.which = in ^ 1;
        hipLaunchKernelGGL(k_ugs_round, dim3(1), dim3(1), 0, st, h->ctl, in, 1);
        hipLaunchKernelGGL(k_ugs_pending, dim3(ugs_wave_blocks(n_pend)), dim3(TB), 0, st, a, m.n_dev, pin, in);
    }
    return ug_back(h->front, st);
}

int hutk_ugseed_words_device(hutk_ugseed* h, uint8_t* d_arena, int64_t* d_start, int64_t* d_len, int64_t* d_count, void* hip_stream) {
    if (!h || !d_start || !d_len || !d_count) return hutk::api_set_error(HUTK_E_ARG, "hutk_ugseed_words_device: bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(h->device));
    if (h->front->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->front->ev, 0));
    if (h->arena_used && !d_arena) return hutk::api_set_error(HUTK_E_ARG, "hutk_ugseed_words_device: d_arena is NULL");
    if (h->arena_used) HUTK_HIP_TRY(hipMemcpyAsync(d_arena, h->arena, (size_t)h->arena_used, hipMemcpyDeviceToDevice, st));
    if (h->n_unique) hipLaunchKernelGGL(k_ugs_words, dim3(blocks_for(h->n_unique)), dim3(TB), 0, st, h->rec, h->n_unique, d_start, d_len, d_count);
    return ug_back(h->front, st);
}

int hutk_ugseed_char_counts_device(hutk_ugseed* h, int64_t* d_counts, void* hip_stream) {
    if (!h || !d_counts) return hutk::api_set_error(HUTK_E_ARG, "hutk_ugseed_char_counts_device: bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(h->device));
    if (h->front->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->front->ev, 0));
    hipLaunchKernelGGL(k_ug_fill_i32, dim3(1 << 12), dim3(TB), 0, st, reinterpret_cast<int32_t*>(d_counts), 2 * SEED_COUNTS, 0);
    if (h->n_unique)
        hipLaunchKernelGGL(k_ugs_chars, dim3(ugs_wave_blocks(h->n_unique)), dim3(TB), 0, st, h->rec, h->n_unique, h->arena,
                           reinterpret_cast<unsigned long long*>(d_counts));
    return ug_back(h->front, st);
}

int hutk_ugseed_count_device(hutk_ugseed* h, int32_t max_piece_chars, int64_t table_slots, int64_t* d_info, void* hip_stream) {
    const std::string who = "hutk_ugseed_count_device";
    if (!h || !d_info) return hutk::api_set_error(HUTK_E_ARG, who + ": bad arguments");
    if (max_piece_chars < 2 || max_piece_chars > SEED_MAX_CHARS) return hutk::api_set_error(HUTK_E_VALUE, who + ": max_piece_chars must be 2 .. 16");
    if (table_slots < 16 || table_slots > (1ll << 40) || (table_slots & (table_slots - 1)))
        return hutk::api_set_error(HUTK_E_VALUE, who + ": table_slots must be a power of two, 16 .. 2^40");
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->arena_used >= (1ll << 32)) return hutk::api_set_error(HUTK_E_UNSUPPORTED, who + ": an arena of 2^32 bytes or more (freq is 32 bits)");
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(h->device));
    HUTK_HIP_TRY(h->s_claim.reserve((size_t)table_slots));
    HUTK_HIP_TRY(h->s_freq.reserve((size_t)table_slots));
    HUTK_HIP_TRY(h->s_fol.reserve((size_t)table_slots));
    HUTK_HIP_TRY(h->s_info.reserve(4));
    if (h->front->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->front->ev, 0));
    h->s_slots = table_slots;
    HUTK_HIP_TRY(hipMemsetAsync(h->s_claim.p, 0, (size_t)table_slots * 8, st));
    HUTK_HIP_TRY(hipMemsetAsync(h->s_freq.p, 0, (size_t)table_slots * 4, st));
    HUTK_HIP_TRY(hipMemsetAsync(h->s_fol.p, 0, (size_t)table_slots * 4, st));
    HUTK_HIP_TRY(hipMemsetAsync(h->s_info.p, 0, 4 * 8, st));
    const SubTab T{h->s_claim.p, h->s_freq.p, h->s_fol.p, (uint64_t)table_slots - 1, (uint64_t)table_slots / 2, h->s_info.p};
    const int64_t tiles = (h->arena_used + SEED_TILE - 1) / SEED_TILE;
    if (h->arena && h->n_unique) hipLaunchKernelGGL(k_ugs_count, dim3((unsigned)tiles), dim3(TB), 0, st, h->arena, h->arena_used, (int)max_piece_chars, T);
    HUTK_HIP_TRY(hipMemcpyAsync(d_info, h->s_info.p, 2 * 8, hipMemcpyDeviceToDevice, st));
    return ug_back(h->front, st);
}

int hutk_ugseed_compact_device(hutk_ugseed* h, int64_t cap, int64_t* d_score, int64_t* d_pos, int32_t* d_len, int64_t* d_n, void* hip_stream) {
    if (!h || cap < 0 || !d_n || (cap > 0 && (!d_score || !d_pos || !d_len))) return hutk::api_set_error(HUTK_E_ARG, "hutk_ugseed_compact_device: bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    if (!h->s_slots) return hutk::api_set_error(HUTK_E_VALUE, "hutk_ugseed_compact_device: hutk_ugseed_count_device has not run on this handle");
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(h->device));
    if (h->front->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->front->ev, 0));
    const SubTab T{h->s_claim.p, h->s_freq.p, h->s_fol.p, (uint64_t)h->s_slots - 1, (uint64_t)h->s_slots / 2, h->s_info.p};
    HUTK_HIP_TRY(hipMemsetAsync(h->s_info.p + 2, 0, 8, st));
    hipLaunchKernelGGL(k_ugs_compact, dim3(blocks_for(h->s_slots)), dim3(TB), 0, st, T, h->s_slots, cap, d_score, d_pos, d_len);
    HUTK_HIP_TRY(hipMemcpyAsync(d_n, h->s_info.p + 2, 8, hipMemcpyDeviceToDevice, st));
    return ug_back(h->front, st);
}

int hutk_ugseed_gather_device(hutk_ugseed* h, const int64_t* d_pos, const int32_t* d_len, const int64_t* d_dst, int64_t n, uint8_t* d_blob,
                              int64_t blob_cap, void* hip_stream) {
    if (!h || n < 0 || blob_cap < 0 || (n > 0 && (!d_pos || !d_len || !d_dst || !d_blob)))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_ugseed_gather_device: bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(h->device));
    if (h->front->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->front->ev, 0));
    if (n) hipLaunchKernelGGL(k_ugs_gather, dim3(blocks_for(n)), dim3(TB), 0, st, h->arena, h->arena_used, d_pos, d_len, d_dst, n, d_blob, blob_cap);
    return ug_back(h->front, st);
}

}  // extern "C"
