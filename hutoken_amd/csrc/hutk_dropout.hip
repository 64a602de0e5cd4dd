// hutk_dropout.hip -- BPE-dropout of a packed batch on the GPU (include/hutoken_amd.h: hutk_encode_dropout_batch_device;
// DESIGN.md section 4e): the merge loop of every word in which a candidate merge is skipped for one step with
// probability p, decided by a Philox draw that is a function of (seed, document, byte offset, step) and of nothing else.
// A word has no single encoding here, so the whole-word table, the word cache, the seam maps and the (byte, next byte)
// table of k_tiles do not apply: the words, the item table, the pair table and rank_of are what is shared.
//
// A text is cut into chunks of CHUNK bytes, a workgroup each, and those into slices of 16 bytes, a lane each.
//
//   k_do_init / k_do_check   the error word and the flag; the offsets describe the bytes (else HUTK_E_ARG and nothing
//                            else is written), the status of every document
//   k_do_clear / k_do_docbits / k_do_starts   the built-in splitter only: the document-start bitmap, then the word
//                            starts of a chunk from the exact classifier of hutk_kdev.h over a window staged in LDS with
//                            look-back and look-ahead (a split preset has written its bitmap already)
//   k_do_words               the word kernel: lists the chunk's word starts in LDS; its lanes take the words of at most
//                            LANE_UNITS bytes from a queue, one word a lane, its wavefronts then the longer ones, one
//                            word a wavefront (units in LDS up to WAVE_LDS_UNITS; beyond, in a per-byte workspace
//                            with a second level of block minima, so that a step does not cost the word's length).
//                            Every byte of a word gets its final id or ID_EMPTY in the per-byte id workspace
//   k_do_count               ids per slice and chunk;  launch_scan_i64 over the chunks
//   k_do_docs                out_offsets;  k_do_write: the ids, compact
// A word of more than MAX_WORD_BYTES bytes lowers its document's byte bound to its own start, as the plain encoder ends the
// document there; count, docs and write leave out what lies at or behind a bound (they look at the bounds only in a batch
// that has such a word).
//
// Nothing synchronises; growing the workspace for a batch larger than any before may wait once.
#include <algorithm>
#include <string>

#include "hutk_host.h"
#include "hutk_kdev.h"
#include "hutk_philox.h"
#include "hutk_wave.h"

namespace {

using namespace hutk;

constexpr int TB = 256, SLICE = 16, CHUNK = TB * SLICE;  // 4096 bytes a workgroup
constexpr int LANE_UNITS = 32;       // longest word one lane merges: liveness and candidates are 32-bit masks
constexpr int WAVE_LDS_UNITS = 256;  // longest word a wavefront merges in LDS
constexpr int EDGE = 32;             // bytes staged in front of and behind a chunk by k_do_starts (a bitmap word each)
constexpr int WINDOW = EDGE + CHUNK + EDGE;
constexpr int MAX_LONG = CHUNK / (LANE_UNITS + 1) + 2;  // longer words that can start in one chunk
constexpr int32_t ID_EMPTY = INT32_MIN;                 // no token starts at this byte (-1 is an id: a unit without a key)
constexpr uint32_t NO_RANK = 0xFFFFFFFFu, DEAD = 0xFFFFFFFEu;
static_assert(LANE_UNITS == 32 && SLICE == 16 && CHUNK % 32 == 0 && EDGE == 32, "masks and bitmap words");

struct DoArgs {
    const uint8_t* bytes;
    const int64_t* offs;  // [n_docs + 1]
    int64_t n_docs, n_bytes, n_chunks;
    const uint32_t* wbits;  // bit p: a word starts at byte p; the bit at n_bytes is set, two zero words of slack behind it
    uint32_t* own_bits;     // the built-in splitter: what k_do_starts writes (wbits points here)
    uint32_t* dbits;        // ...: bit p: a document starts at p, and the bit at n_bytes
    int64_t n_bit_words;
    int32_t* tmp;           // [n_bytes]: the id of the token that starts at the byte, or ID_EMPTY
    // [n_bytes] each, for the words beyond WAVE_LDS_UNITS (their symbols live in tmp): rank, next, previous, the step a
    // position was dropped at, and from the word's first byte on the smallest rank of each block of 64 positions
    uint32_t *g_rank, *g_next, *g_prev, *g_stamp, *g_blk;
    int64_t* chunk;         // [n_chunks + 1]: ids per chunk, then their exclusive scan and the total
    uint16_t* slice;        // [n_chunks * TB]: ids of the chunk in front of the slice
    unsigned long long* bound;  // [n_docs]: the document's ids come from the bytes in front of this one
    int32_t* n_cut;         // documents with a lowered bound
    uint64_t drop_below, seed;
    int64_t first_doc;
    int32_t* ids;
    int64_t ids_cap;
    int64_t* out_offs;
    int32_t* status;  // may be null
    int32_t* err;
    int32_t* ok;
};

__global__ void k_do_init(int32_t* err, int32_t* ok, int32_t* n_cut) {
    *err = 0;
    *ok = 1;
    *n_cut = 0;
}

__global__ __launch_bounds__(TB) void k_do_check(const DoArgs a) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    bool bad = false;
    if (i < a.n_docs) {
        bad = a.offs[i + 1] < a.offs[i] || a.offs[i] < 0 || a.offs[i + 1] > a.n_bytes;
        if (a.status) a.status[i] = HUTK_DOC_OK;
        a.bound[i] = ~0ull;
    }
    if (i == 0) bad = bad || a.offs[0] != 0 || a.offs[a.n_docs] != a.n_bytes;
    if (bad) {
        *a.ok = 0;
        raise(a.err, HUTK_E_ARG);
    }
}

__global__ __launch_bounds__(TB) void k_do_clear(uint32_t* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) p[i] = 0;
}

// (dbits has been cleared; the offsets are sound)
__global__ __launch_bounds__(TB) void k_do_docbits(const DoArgs a) {
    if (!*a.ok) return;
    const int64_t d = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (d > a.n_docs) return;
    const int64_t o = a.offs[d];
    atomicOr(&a.dbits[o >> 5], 1u << (o & 31));
}

// The word starts of the built-in splitter (src/parser.c restated per position: code_at and word_starts of hutk_kdev.h),
// chunk by chunk.  Window index li is byte c0 - EDGE + li; bytes outside the batch are staged as 0, and the bit at
// n_bytes, which k_do_docbits set, ends the last word.  The grid has one chunk more than the text when n_bytes is a
// multiple of CHUNK: that bit's.
__global__ __launch_bounds__(TB) void k_do_starts(const DoArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_b[WINDOW + 8];
    __shared__ uint8_t s_code[WINDOW + 8];
    __shared__ uint32_t s_docm[WINDOW / 32 + 3];
    if (!*a.ok) return;
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK, w0 = c0 - EDGE;
    for (int li = tid; li < WINDOW + 8; li += TB) {
        const int64_t p = w0 + li;
        s_b[li] = p >= 0 && p < a.n_bytes ? a.bytes[p] : (uint8_t)0;
    }
    for (int w = tid; w < WINDOW / 32 + 3; w += TB) {
        const int64_t gw = (w0 >> 5) + w;  // (w0 is a multiple of 32, negative for the first chunk only)
        s_docm[w] = gw >= 0 && gw < a.n_bit_words ? a.dbits[gw] : 0u;
    }
    __syncthreads();
    // code_at looks three bytes back and lead_class three ahead; word_starts looks five codes back
    for (int li = tid; li < WINDOW + 8; li += TB) s_code[li] = li >= 8 && li < WINDOW ? code_at(s_b, s_docm, li) : (uint8_t)C_BAD;
    __syncthreads();
    uint32_t starts = 0;
    for (int i = 0; i < SLICE; i++) {
        const int li = EDGE + tid * SLICE + i;
        const int64_t p = w0 + li;
        if (p < a.n_bytes ? word_starts(s_code, s_docm, li) : p == a.n_bytes) starts |= 1u << i;
    }
    const uint32_t up = (uint32_t)__shfl_down((int)starts, 1);
    const int64_t gw = (c0 >> 5) + (tid >> 1);
    if (!(tid & 1) && gw < a.n_bit_words) a.own_bits[gw] = starts | (up << 16);
}

// 64 bits of a bitmap from bit `start` on (two words of slack behind the last bit in use)
__device__ __forceinline__ uint64_t gbits64(const uint32_t* m, int64_t start) {
    const int64_t k = start >> 5;
    const int sh = (int)(start & 31);
    uint64_t v = ((uint64_t)m[k] | ((uint64_t)m[k + 1] << 32)) >> sh;
    if (sh) v |= (uint64_t)m[k + 2] << (64 - sh);
    return v;
}

// the last document of [lo, hi) that starts at or before byte p (lo does)
__device__ __forceinline__ int64_t doc_at(const int64_t* offs, int64_t lo, int64_t hi, int64_t p) {
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (offs[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Is the candidate whose left unit begins at byte `o` of document `doc` dropped at step t?  (The rule: hutoken_amd.h.)
__device__ __forceinline__ bool dropped(const DoArgs& a, int64_t doc, int64_t o, uint32_t t) {
    const Philox4 r = philox4x32_10((uint32_t)(uint64_t)doc, (uint32_t)((uint64_t)doc >> 32), (uint32_t)(uint64_t)o,
                                    (t << 4) | DRAW_BPE_DROPOUT, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    return (uint64_t)r.x < a.drop_below;
}

__device__ __forceinline__ uint32_t rank_or_none(const DevTables& T, uint32_t merged) {
    return merged == SYM_NONE ? NO_RANK : rank_of(T, merged);
}

// One lane, one word of n <= LANE_UNITS bytes at byte ws.  The unit that begins at byte i of the word is S[i] for as long
// as it lives (a merge keeps the left unit's place), R[i] the rank of its pair with the next live unit or NO_RANK; which
// units live and which pairs are candidates are two masks in registers.  A pair is priced when the word is set up and
// again only beside an applied merge; the two new neighbour lookups are issued together.  The draws are lazy: the best
// candidate is drawn for, the next-best only when it was dropped.
__device__ __forceinline__ void lane_word(const DevTables& T, const DoArgs& a, uint32_t* S, uint32_t* R, int64_t ws, int n, int64_t d_lo,
                                          int64_t d_hi) {
    for (int i = 0; i < n; i++) S[i] = T.item_sym[a.bytes[ws + i]];
    uint32_t live = n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u, cand = 0;
    if (a.drop_below <= 0xFFFFFFFFull) {  // (p = 1 drops every candidate of every step: nothing is priced)
        for (int i = 0; i + 1 < n; i++) {
            const uint32_t r = rank_or_none(T, pair_lookup(T, S[i], S[i + 1]));
            R[i] = r;
            if (r != NO_RANK) cand |= 1u << i;
        }
    }
    if (cand) {
        int64_t doc = 0, o0 = 0;
        if (a.drop_below) {
            const int64_t d = doc_at(a.offs, d_lo, d_hi, ws);
            doc = a.first_doc + d, o0 = ws - a.offs[d];
        }
        for (uint32_t t = 0;; t++) {
            int best = -1;
            for (uint32_t avail = cand; avail;) {
                uint32_t bk = NO_RANK;
                int bi = -1;
                for (uint32_t m = avail; m; m &= m - 1) {  // rising positions and a strict compare: leftmost on ties
                    const int i = __ffs(m) - 1;
                    const uint32_t r = R[i];
                    if (r < bk) bk = r, bi = i;
                }
                if (!a.drop_below || !dropped(a, doc, o0 + bi, t)) {
                    best = bi;
                    break;
                }
                avail &= ~(1u << bi);
            }
            if (best < 0) break;
            const uint32_t above = live & ~((2u << best) - 1u);  // (best < 31: a candidate has a live unit behind it)
            const int r = __ffs(above) - 1;
            const uint32_t merged = T.rank_is_sym ? R[best] : pair_lookup(T, S[best], S[r]);
            S[best] = merged;
            live &= ~(1u << r);
            cand &= ~((1u << r) | (1u << best));
            const uint32_t above2 = above & (above - 1u), below = live & ((1u << best) - 1u);
            const int r2 = above2 ? __ffs(above2) - 1 : -1, l = below ? 31 - __clz(below) : -1;
            const uint32_t sr = r2 >= 0 ? S[r2] : SYM_UNK, sl = l >= 0 ? S[l] : SYM_UNK;  // (SYM_UNK: in no pair)
            const PairProbe pa = pair_issue(T, merged, sr), pb = pair_issue(T, sl, merged);
            const uint32_t ra = r2 >= 0 ? rank_or_none(T, pair_resolve(T, pa, merged, sr)) : NO_RANK;
            const uint32_t rb = l >= 0 ? rank_or_none(T, pair_resolve(T, pb, sl, merged)) : NO_RANK;
            R[best] = ra;
            if (ra != NO_RANK) cand |= 1u << best;
            if (l >= 0) {
                R[l] = rb;
                cand = rb != NO_RANK ? cand | (1u << l) : cand & ~(1u << l);
            }
        }
    }
    for (int i = 0; i < n; i++) a.tmp[ws + i] = (live >> i) & 1u ? sym_to_id(T, S[i]) : ID_EMPTY;
}

// What one lane of a word's wavefront wrote, the others read after this.  GLOBAL: the word's arrays are in global memory.
template <bool GLOBAL>
__device__ __forceinline__ void word_sync() {
    if constexpr (GLOBAL) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    } else {
        wave_sync();
    }
}

// One wavefront, one word of n bytes at byte ws (all 64 lanes run this with the same arguments).  S, R: as lane_word's;
// NX[i] / PV[i]: the next / the previous live unit of live unit i (n / all ones: none), NX[i] == DEAD: unit i is gone.
// A step: every lane looks at the positions lane, lane + 64, ..., draws for each candidate it finds there (eager, one
// Philox call a candidate) and keeps its smallest surviving (rank, position); a wave reduction picks the winner, every
// lane prices the winner's two new pairs (the same addresses: one broadcast load each) and lane 0 writes.  For words
// of up to WAVE_LDS_UNITS bytes, in LDS rows: at most four positions a lane.
__device__ __forceinline__ void wave_word(const DevTables& T, const DoArgs& a, uint32_t* S, uint32_t* R, uint32_t* NX, uint32_t* PV,
                                          int64_t ws, int64_t n, int lane, int64_t d_lo, int64_t d_hi) {
    for (int64_t i = lane; i < n; i += 64) {
        S[i] = T.item_sym[a.bytes[ws + i]];
        NX[i] = (uint32_t)(i + 1);
        PV[i] = (uint32_t)i - 1u;
    }
    word_sync<false>();
    if (a.drop_below <= 0xFFFFFFFFull) {
        for (int64_t i = lane; i < n; i += 64) R[i] = i + 1 < n ? rank_or_none(T, pair_lookup(T, S[i], S[i + 1])) : NO_RANK;
        word_sync<false>();
        int64_t doc = 0, o0 = 0;
        if (a.drop_below) {
            const int64_t d = doc_at(a.offs, d_lo, d_hi, ws);
            doc = a.first_doc + d, o0 = ws - a.offs[d];
        }
        for (uint32_t t = 0;; t++) {
            uint64_t best = ~0ull;
            for (int64_t i = lane; i < n; i += 64) {
                const uint32_t r = R[i];
                if (r == NO_RANK || (a.drop_below && dropped(a, doc, o0 + i, t))) continue;
                const uint64_t key = ((uint64_t)r << 32) | (uint64_t)i;
                if (key < best) best = key;
            }
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                const uint64_t other = __shfl_xor(best, o);
                if (other < best) best = other;
            }
            if (best == ~0ull) break;
            const uint32_t i = (uint32_t)best, r = NX[i], l = PV[i];
            const uint32_t r2 = NX[r];
            const uint32_t merged = T.rank_is_sym ? (uint32_t)(best >> 32) : pair_lookup(T, S[i], S[r]);
            const bool has_r2 = r2 < (uint32_t)n, has_l = l != 0xFFFFFFFFu;
            const uint32_t sr = has_r2 ? S[r2] : SYM_UNK, sl = has_l ? S[l] : SYM_UNK;
            const PairProbe pa = pair_issue(T, merged, sr), pb = pair_issue(T, sl, merged);
            const uint32_t ra = has_r2 ? rank_or_none(T, pair_resolve(T, pa, merged, sr)) : NO_RANK;
            const uint32_t rb = has_l ? rank_or_none(T, pair_resolve(T, pb, sl, merged)) : NO_RANK;
            if (lane == 0) {
                S[i] = merged;
                R[i] = ra;
                NX[i] = r2;
                if (has_r2) PV[r2] = i;
                if (has_l) R[l] = rb;
                NX[r] = DEAD;
                R[r] = NO_RANK;
            }
            word_sync<false>();
        }
    }
    for (int64_t i = lane; i < n; i += 64) a.tmp[ws + i] = NX[i] != DEAD ? sym_to_id(T, S[i]) : ID_EMPTY;
    word_sync<false>();  // (the rows are the next word's)
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// BR[b] = the smallest rank among the positions 64 b .. 64 b + 63 of a long word that are candidates and were not dropped
// at step t (ST[i] == t + 1: dropped at step t), by the whole wavefront.
__device__ __forceinline__ void block_min(const uint32_t* R, const uint32_t* ST, uint32_t* BR, int64_t b, int64_t n, uint32_t t, int lane) {
    const int64_t i = 64 * b + lane;
    uint32_t r = i < n ? R[i] : NO_RANK;
    if (r != NO_RANK && ST[i] == t + 1u) r = NO_RANK;
    r = wave_min_u32(r);
    if (lane == 0) BR[b] = r;
}

// One wavefront, one word of WAVE_LDS_UNITS < n <= MAX_WORD_BYTES bytes, its arrays in global memory (S is the word's
// stretch of the id workspace).  A step must not cost the word's length -- there can be n - 1 steps --, so the ranks
// have a second level: BR[b], the smallest rank of block b of 64 positions.  An attempt: the lanes look through BR
// (n / 4096 trips), a reduction gives the smallest (rank, block), one load of that block gives the leftmost position that
// holds it, ONE draw decides; a dropped candidate is stamped with the step, its block's minimum is made again without
// it, and the next attempt finds the next-best: lazy draws, about 1 / (1 - p) attempts a step.  Behind an applied merge
// the blocks of the three positions whose ranks changed and of the step's drops are made again.  Every value that steers
// the flow is read from lane 0 (readfirstlane): the flow is wave-uniform.  drops: DROP_LIST words of LDS, the wavefront's.
constexpr int DROP_LIST = 64;
__device__ __forceinline__ void big_word(const DevTables& T, const DoArgs& a, uint32_t* S, uint32_t* R, uint32_t* NX, uint32_t* PV,
                                         uint32_t* ST, uint32_t* BR, uint32_t* drops, int64_t ws, int64_t n, int lane, int64_t d_lo,
                                         int64_t d_hi) {
    for (int64_t i = lane; i < n; i += 64) {
        S[i] = T.item_sym[a.bytes[ws + i]];
        NX[i] = (uint32_t)(i + 1);
        PV[i] = (uint32_t)i - 1u;
        ST[i] = 0;
    }
    word_sync<true>();
    if (a.drop_below <= 0xFFFFFFFFull) {
        for (int64_t i = lane; i < n; i += 64) R[i] = i + 1 < n ? rank_or_none(T, pair_lookup(T, S[i], S[i + 1])) : NO_RANK;
        word_sync<true>();
        const int64_t nb = (n + 63) >> 6;
        for (int64_t b = 0; b < nb; b++) block_min(R, ST, BR, b, n, 0, lane);
        word_sync<true>();
        int64_t doc = 0, o0 = 0;
        if (a.drop_below) {
            const int64_t d = doc_at(a.offs, d_lo, d_hi, ws);
            doc = a.first_doc + d, o0 = ws - a.offs[d];
        }
        for (uint32_t t = 0;; t++) {
            int n_drop = 0;
            uint32_t pos = 0, rank = NO_RANK;
            bool found = false;
            for (;;) {
                uint64_t best = ~0ull;
                for (int64_t b = lane; b < nb; b += 64) {
                    const uint32_t r = BR[b];
                    const uint64_t key = ((uint64_t)r << 32) | (uint64_t)b;
                    if (r != NO_RANK && key < best) best = key;
                }
#pragma unroll
                for (int o = 32; o; o >>= 1) {
                    const uint64_t other = __shfl_xor(best, o);
                    if (other < best) best = other;
                }
                rank = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(best >> 32));
                if (rank == NO_RANK) break;  // no candidate is left, or none survived this step
                const int64_t b = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)best), i = 64 * b + lane;
                const uint64_t hit = __ballot(i < n && R[i] == rank && ST[i] != t + 1u);
                if (hit) {
                    pos = (uint32_t)(64 * b) + (uint32_t)__builtin_ctzll(hit);  // leftmost on ties: the first block, its first lane
                    if (!a.drop_below || !dropped(a, doc, o0 + pos, t)) {
                        found = true;
                        break;
                    }
                    if (lane == 0) {
                        ST[pos] = t + 1u;
                        if (n_drop < DROP_LIST) drops[n_drop] = pos;
                    }
                    n_drop++;
                    word_sync<true>();
                }
                block_min(R, ST, BR, b, n, t, lane);
                word_sync<true>();
            }
            if (!found) break;
            const uint32_t i = pos, r = NX[i], l = PV[i];
            const uint32_t r2 = NX[r];
            const uint32_t merged = T.rank_is_sym ? rank : pair_lookup(T, S[i], S[r]);
            const bool has_r2 = r2 < (uint32_t)n, has_l = l != 0xFFFFFFFFu;
            const uint32_t sr = has_r2 ? S[r2] : SYM_UNK, sl = has_l ? S[l] : SYM_UNK;
            const PairProbe pa = pair_issue(T, merged, sr), pb = pair_issue(T, sl, merged);
            const uint32_t ra = has_r2 ? rank_or_none(T, pair_resolve(T, pa, merged, sr)) : NO_RANK;
            const uint32_t rb = has_l ? rank_or_none(T, pair_resolve(T, pb, sl, merged)) : NO_RANK;
            if (lane == 0) {
                S[i] = merged;
                R[i] = ra;
                NX[i] = r2;
                if (has_r2) PV[r2] = i;
                if (has_l) R[l] = rb;
                NX[r] = DEAD;
                R[r] = NO_RANK;
            }
            word_sync<true>();
            // (made for the next step: its stamp t + 2 is on no position, so this step's drops are candidates again)
            block_min(R, ST, BR, i >> 6, n, t + 1u, lane);
            block_min(R, ST, BR, r >> 6, n, t + 1u, lane);
            if (has_l) block_min(R, ST, BR, l >> 6, n, t + 1u, lane);
            if (n_drop > DROP_LIST) {
                for (int64_t b = 0; b < nb; b++) block_min(R, ST, BR, b, n, t + 1u, lane);
            } else {
                for (int k = 0; k < n_drop; k++) block_min(R, ST, BR, drops[k] >> 6, n, t + 1u, lane);
            }
            word_sync<true>();
        }
    }
    for (int64_t i = lane; i < n; i += 64) a.tmp[ws + i] = NX[i] != DEAD ? sym_to_id(T, S[i]) : ID_EMPTY;  // (in place: S is tmp + ws)
    word_sync<true>();
}

__global__ __launch_bounds__(TB) void k_do_words(const DevTables T, const DoArgs a) {
    __shared__ uint32_t s_S[CHUNK + LANE_UNITS], s_R[CHUNK + LANE_UNITS];  // in place: a word's units at its bytes' indices
    __shared__ uint32_t s_row[TB / 64][4][WAVE_LDS_UNITS];                 // S, R, NX, PV of a wavefront's word
    __shared__ uint16_t s_ws[CHUNK], s_long[MAX_LONG];
    __shared__ uint32_t s_drops[TB / 64][DROP_LIST];
    __shared__ int s_part[TB / 64];
    __shared__ int s_next, s_n_long;
    __shared__ int64_t s_d_lo, s_d_hi;
    if (!*a.ok) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK, at = c0 + (int64_t)tid * SLICE;
    if (tid == 0) {
        s_next = s_n_long = 0;
        if (a.drop_below) {  // the documents that words of this chunk can lie in: [s_d_lo, s_d_hi)
            const int64_t lo = doc_at(a.offs, 0, a.n_docs, c0);
            const int64_t last = c0 + CHUNK - 1 < a.n_bytes ? c0 + CHUNK - 1 : a.n_bytes - 1;
            s_d_lo = lo;
            s_d_hi = doc_at(a.offs, lo, a.n_docs, last) + 1;
        }
    }
    // the chunk's word starts, in rising order, as offsets from c0; and the check for 0x00 bytes
    const int64_t bw = (c0 >> 5) + (tid >> 1);  // (the bitmap ends two words behind the bit at n_bytes)
    uint32_t starts = bw <= (a.n_bytes >> 5) ? (a.wbits[bw] >> (16 * (tid & 1))) & 0xFFFFu : 0u;
    bool nul = false;
    for (int i = 0; i < SLICE; i++) {
        if (at + i >= a.n_bytes) starts &= ~(1u << i);
        else nul = nul || a.bytes[at + i] == 0;
    }
    if (nul) raise(a.err, HUTK_E_NUL_BYTE);
    int n_words;
    int before = block_excl((int)__popc(starts), s_part, n_words);
    for (uint32_t m = starts; m; m &= m - 1) s_ws[before++] = (uint16_t)(tid * SLICE + __ffs(m) - 1);
    __syncthreads();
    const int64_t d_lo = a.drop_below ? s_d_lo : 0, d_hi = a.drop_below ? s_d_hi : 1;
    for (;;) {  // the short words, a lane each, dealt as the lanes come free
        const int i = atomicAdd(&s_next, 1);
        if (i >= n_words) break;
        const int w0 = s_ws[i];
        const int64_t ws = c0 + w0;
        const uint64_t ahead = gbits64(a.wbits, ws + 1);  // (the bit at n_bytes ends the last word)
        const int n = ahead ? __builtin_ctzll(ahead) + 1 : 65;
        if (n > LANE_UNITS) {
            s_long[atomicAdd(&s_n_long, 1)] = (uint16_t)w0;
            continue;
        }
        lane_word(T, a, s_S + w0, s_R + w0, ws, n, d_lo, d_hi);
    }
    __syncthreads();
    const int n_long = s_n_long;
    // The longer ones, a wavefront each.  The index is wave-uniform by construction: no value read from lane 0 inside a
    // loop that lanes could leave separately.
    for (int i = wave; i < n_long; i += TB / 64) {
        const int64_t ws = c0 + s_long[i];
        // the word's end: the next start, looked for 64 x 64 bits a trip, no further than the longest word allowed
        int64_t n = 0;
        for (int64_t base = ws + 1; n == 0 && base - ws <= MAX_WORD_BYTES + 1; base += 64 * 64) {
            const int64_t from = base + 64 * lane;
            const uint64_t bits = from <= a.n_bytes ? gbits64(a.wbits, from) : 0ull;
            const uint64_t found = __ballot(bits != 0);
            if (found) {
                const int src = __builtin_ctzll(found);
                const uint64_t b = __shfl(bits, src);
                n = base + 64 * src + __builtin_ctzll(b) - ws;
            }
        }
        if (n == 0 || n > MAX_WORD_BYTES) {  // as the plain encoder: the document ends in front of this word
            if (lane == 0) {
                const int64_t d = doc_at(a.offs, 0, a.n_docs, ws);
                atomicMin(&a.bound[d], (unsigned long long)ws);
                if (a.status) a.status[d] = HUTK_DOC_WORD_TOO_LARGE;
                raise(a.err, HUTK_E_WORD_TOO_LARGE);
                atomicAdd(a.n_cut, 1);
            }
        } else if (n <= WAVE_LDS_UNITS)
            wave_word(T, a, s_row[wave][0], s_row[wave][1], s_row[wave][2], s_row[wave][3], ws, n, lane, d_lo, d_hi);
        else
            big_word(T, a, reinterpret_cast<uint32_t*>(a.tmp + ws), a.g_rank + ws, a.g_next + ws, a.g_prev + ws, a.g_stamp + ws, a.g_blk + ws,
                     s_drops[wave], ws, n, lane, d_lo, d_hi);
    }
}

// Does byte p give an id?  d: the document of the position asked about last (-1: none yet); positions are asked in rising
// order.  The bounds are looked at only in a batch in which some document was cut.
__device__ __forceinline__ bool gives_id(const DoArgs& a, bool cut, int64_t p, int64_t& d) {
    if (cut) {
        if (d < 0) d = doc_at(a.offs, 0, a.n_docs, p);
        while (d + 1 < a.n_docs && a.offs[d + 1] <= p) d++;
        if ((unsigned long long)p >= a.bound[d]) return false;  // (what lies there may never have been written)
    }
    return a.tmp[p] != ID_EMPTY;
}

__global__ __launch_bounds__(TB) void k_do_count(const DoArgs a) {
    __shared__ int s_part[TB / 64];
    if (!*a.ok) return;
    const int64_t k = blockIdx.x, at = k * CHUNK + (int64_t)threadIdx.x * SLICE;
    const bool cut = *a.n_cut != 0;
    int ids = 0;
    int64_t d = -1;
    for (int64_t p = at; p < at + SLICE && p < a.n_bytes; p++) ids += gives_id(a, cut, p, d);
    int total;
    const int before = block_excl(ids, s_part, total);
    a.slice[k * TB + threadIdx.x] = (uint16_t)before;
    if (threadIdx.x == 0) a.chunk[k] = total;
}

__global__ __launch_bounds__(TB) void k_do_docs(const DoArgs a) {
    if (!*a.ok) return;
    const int64_t d = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (d > a.n_docs) return;
    const int64_t total = a.chunk[a.n_chunks];
    if (total > a.ids_cap) {  // nothing is written into buffers the ids do not fit
        if (d == 0) raise(a.err, HUTK_E_CAPACITY);
        return;
    }
    const int64_t o = a.offs[d];
    int64_t r = total;
    if (o < a.n_bytes) {
        const int64_t k = o / CHUNK, s0 = o & ~(int64_t)(SLICE - 1);
        r = a.chunk[k] + a.slice[k * TB + (s0 - k * CHUNK) / SLICE];
        const bool cut = *a.n_cut != 0;
        int64_t dd = -1;
        for (int64_t p = s0; p < o; p++) r += gives_id(a, cut, p, dd);
    }
    a.out_offs[d] = r;
}

__global__ __launch_bounds__(TB) void k_do_write(const DoArgs a) {
    if (!*a.ok || a.chunk[a.n_chunks] > a.ids_cap) return;
    const int64_t k = blockIdx.x, at = k * CHUNK + (int64_t)threadIdx.x * SLICE;
    const bool cut = *a.n_cut != 0;
    int64_t to = a.chunk[k] + a.slice[k * TB + threadIdx.x], d = -1;
    for (int64_t p = at; p < at + SLICE && p < a.n_bytes; p++)
        if (gives_id(a, cut, p, d)) a.ids[to++] = a.tmp[p];
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + TB) / TB); }

}  // namespace

extern "C" {

int hutk_debug_dropout_info(int64_t* out4) {
    if (!out4) return hutk::api_set_error(HUTK_E_ARG, "hutk_debug_dropout_info: out4 is NULL");
    out4[0] = CHUNK, out4[1] = LANE_UNITS, out4[2] = WAVE_LDS_UNITS, out4[3] = MAX_WORD_BYTES;
    return HUTK_OK;
}

int hutk_encode_dropout_batch_device(hutk_ctx* c, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                                     uint64_t drop_below, uint64_t seed, int64_t first_doc, int32_t* d_ids_out, int64_t ids_cap,
                                     int64_t* d_out_offsets, int32_t* d_status, int32_t* d_err, void* hip_stream) {
    const std::string who = "hutk_encode_dropout_batch_device: ";
    if (!c) return api_set_error(HUTK_E_ARG, who + "ctx is NULL");
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, who + "host-only context: no device to encode on");
    if (n_docs < 0 || n_bytes < 0 || !d_offsets || !d_out_offsets || (n_bytes > 0 && (!d_bytes || !d_ids_out)))
        return api_set_error(HUTK_E_ARG, who + "bad argument");
    if (first_doc < 0 || (n_docs > 0 && first_doc > INT64_MAX - n_docs))  // (first_doc + d stays an int64)
        return api_set_error(HUTK_E_ARG, who + "first_doc must not be negative");
    if (drop_below > (1ull << 32)) return api_set_error(HUTK_E_VALUE, who + "drop_below is above 2^32");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (!c->tab.is_byte_encoder || c->tab.has_prefix || c->tab.has_multi || !c->pattern.empty())
        return api_set_error(HUTK_E_UNSUPPORTED, who + "BPE-dropout takes a byte-encoder context without a prefix, without items of "
                                                       "several units and without a regex pattern");
    if (ids_cap < hutk_ids_capacity(c, n_bytes, n_docs) - 1) return api_set_error(HUTK_E_CAPACITY, who + "ids_cap is below hutk_ids_capacity()");
    const int64_t n_chunks = (n_bytes + CHUNK - 1) / CHUNK, n_bit_words = n_bytes / 32 + 8;
    if (n_chunks >= INT32_MAX || (n_docs + TB) / TB > INT32_MAX) return api_set_error(HUTK_E_UNSUPPORTED, who + "the batch is too large for one launch");
    HUTK_HIP_TRY(hipSetDevice(c->device));
    hutk_ctx::Dropout& W = c->dro;
    const bool preset = c->presplit >= 0;
    HUTK_HIP_TRY(c->w_err.reserve(1));
    HUTK_HIP_TRY(W.flags.reserve(2));
    HUTK_HIP_TRY(W.bound.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(W.chunk.reserve((size_t)n_chunks + 1));
    HUTK_HIP_TRY(W.slice.reserve((size_t)n_chunks * TB + 1));
    HUTK_HIP_TRY(W.tmp.reserve((size_t)n_bytes + 1));
    HUTK_HIP_TRY(W.link.reserve(5 * (size_t)n_bytes + 1));
    if (preset) HUTK_HIP_TRY(c->w_wbits.reserve((size_t)(n_bytes / 32 + 40)));
    else HUTK_HIP_TRY(W.bits.reserve(2 * (size_t)n_bit_words));
    StreamScope scope(c, hip_stream, false);  // the previous call still owns the workspace
    if (scope.rc) return scope.rc;
    hipStream_t s = scope.s;

    DoArgs a{};
    a.bytes = d_bytes, a.offs = d_offsets, a.n_docs = n_docs, a.n_bytes = n_bytes, a.n_chunks = n_chunks;
    a.n_bit_words = n_bit_words;
    a.tmp = W.tmp.p, a.g_rank = W.link.p, a.g_next = W.link.p + n_bytes, a.g_prev = W.link.p + 2 * n_bytes;
    a.g_stamp = W.link.p + 3 * n_bytes, a.g_blk = W.link.p + 4 * n_bytes;
    a.chunk = W.chunk.p, a.slice = W.slice.p, a.bound = W.bound.p;
    a.ok = W.flags.p, a.n_cut = W.flags.p + 1;
    a.drop_below = drop_below, a.seed = seed, a.first_doc = first_doc;
    a.ids = d_ids_out, a.ids_cap = ids_cap, a.out_offs = d_out_offsets, a.status = d_status, a.err = d_err ? d_err : c->w_err.p;

    if (preset && n_chunks) {
        // the preset's word starts (documents start words there, and the bit at n_bytes is set), first: what it refuses is
        // refused before anything of this call is enqueued
        if (int rc = hutk_pretokenize_batch_device(c->pretok, c->presplit, d_bytes, d_offsets, n_docs, n_bytes, c->w_wbits.p, nullptr, s))
            return rc;
    }
    hipLaunchKernelGGL(k_do_init, dim3(1), dim3(1), 0, s, a.err, a.ok, a.n_cut);
    hipLaunchKernelGGL(k_do_check, dim3(blocks_for(n_docs)), dim3(TB), 0, s, a);
    hipLaunchKernelGGL(k_do_clear, dim3((unsigned)std::min<int64_t>((n_chunks + 1 + TB) / TB, 4096)), dim3(TB), 0, s,
                       reinterpret_cast<uint32_t*>(a.chunk), 2 * (n_chunks + 1));
    if (n_chunks) {
        if (preset) {
            a.wbits = c->w_wbits.p;
        } else {
            a.own_bits = W.bits.p, a.dbits = W.bits.p + n_bit_words, a.wbits = a.own_bits;
            hipLaunchKernelGGL(k_do_clear, dim3((unsigned)std::min<int64_t>((2 * n_bit_words + TB) / TB, 4096)), dim3(TB), 0, s, W.bits.p,
                               2 * n_bit_words);
            hipLaunchKernelGGL(k_do_docbits, dim3(blocks_for(n_docs)), dim3(TB), 0, s, a);
            hipLaunchKernelGGL(k_do_starts, dim3((unsigned)(n_bytes / CHUNK + 1)), dim3(TB), 0, s, a);
        }
        hipLaunchKernelGGL(k_do_words, dim3((unsigned)n_chunks), dim3(TB), 0, s, c->dt, a);
        hipLaunchKernelGGL(k_do_count, dim3((unsigned)n_chunks), dim3(TB), 0, s, a);
    }
    launch_scan_i64(a.chunk, n_chunks, s);
    hipLaunchKernelGGL(k_do_docs, dim3(blocks_for(n_docs)), dim3(TB), 0, s, a);
    if (n_chunks) hipLaunchKernelGGL(k_do_write, dim3((unsigned)n_chunks), dim3(TB), 0, s, a);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

}  // extern "C"
