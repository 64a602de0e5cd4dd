// hutk_unigram.hip -- Unigram encoding of a packed batch on the GPU (include/hutoken_amd.h):
// (uint8 bytes, int64 offsets[n + 1]) in, the ragged (int32 ids, int64 out_offsets[n + 1]) of hutk_encode_batch_device
// out, and on request the word index of every id.  The rule -- fold, word starts, table and probe, the update of the
// best path, the backtrack -- is hutk_unigram.h, shared with the CPU check; this file is the chunking, the placement,
// the lanes of the lattice kernel and the C entry points.
//
// A text is cut into chunks of CHUNK_BYTES and those into slices of 16 bytes, a lane each.  The folded text's size is
// known to the device only: a grid is sized by the host's bound (n_bytes + n_docs) and the workgroups behind the real
// end leave at once.
//
//   k_ug_check       the offsets describe the bytes (else HUTK_E_ARG and nothing else is written)
//   k_ug_flags       flag[p] = a document starts at p
//   k_ug_fold_count  every lane counts what its slice folds to; a workgroup scan places the slice in the chunk
//   k_ug_scan        exclusive scan over the chunks (one workgroup)
//   k_ug_fold_write  every lane folds again and writes from its place
//   k_ug_fold_docs   the folded offsets and flags of the documents
//   k_ug_fill        the id workspace, one int32 per folded byte, is emptied
//   k_ug_lattice     word starts of a chunk; a group of 8 lanes takes the next word of the chunk's queue and walks its
//                    starts: the lanes probe 8 lengths of a start a trip, the best scores of the last max_len + 1
//                    positions live in a ring in LDS, the backpointers go to a per-byte workspace; lane 0 walks back
//   k_ug_sample      in k_ug_lattice's place when a segmentation is sampled (hutk_unigram_sample_batch_device): the same
//                    chunks, queue and groups; a group first sums the word's lattice from its end to its start (beta, a
//                    log-sum-exp per character start, in the ring and for a word longer than the ring in a per-byte
//                    workspace as well), then draws the path from the start, one Philox draw a piece
//   k_ug_count       ids and words per slice and chunk;  k_ug_scan over both
//   k_ug_docs        out_offsets, and the word count in front of every document
//   k_ug_write       the ids, compact, and the word ids
// Training (hutk_unigram_train.h, included below: k_ug_estep, k_ug_lattice_train, k_ug_hist and the small kernels of the
// M-step and the prune) starts from the same front half, ug_front.
//
// Nothing synchronises; growing the workspace for a batch larger than any before may wait once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "hutk_host.h"
#include "hutk_philox.h"
#include "hutk_unigram.h"
#include "hutk_wave.h"

namespace {

namespace U = hutk::ug;

constexpr int TB = U::CHUNK_SLICES;  // 256 lanes: a slice each
static_assert(TB == 256 && U::SLICE_BYTES == 16, "a lane owns 16 bytes");
constexpr int GROUP = 8;             // lanes that own a word
constexpr int GROUPS = TB / GROUP;
constexpr int RING_LDS_BYTES = 32768;  // all rings of a workgroup

__device__ __forceinline__ void note_error(int32_t* err, int code) { atomicCAS(err, 0, code); }

__global__ __launch_bounds__(TB) void k_ug_check(const int64_t* offs, int64_t n_docs, int64_t n_bytes, int32_t* ok, int32_t* err) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    bool bad = false;
    if (i < n_docs) bad = offs[i + 1] < offs[i] || offs[i] < 0 || offs[i + 1] > n_bytes;
    if (i == 0) bad = bad || offs[0] != 0 || offs[n_docs] != n_bytes;
    if (bad) {
        *ok = 0;
        note_error(err, HUTK_E_ARG);
    }
}

// (flag has been zeroed; offs is sound)
__global__ __launch_bounds__(TB) void k_ug_flags(const int64_t* offs, int64_t n_docs, uint8_t* flag, const int32_t* ok) {
    if (!*ok) return;
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i < n_docs) flag[offs[i]] = 1;
}

struct FoldArgs {
    U::Text x;             // the source
    uint32_t flags;
    int64_t* chunk;        // [n_chunks + 1]: sizes, then their exclusive scan and the total
    int64_t n_chunks;
    uint16_t* slice;       // [n_chunks * TB]: bytes of the chunk's output in front of the slice's
    uint8_t* out;
    uint8_t* out_flag;     // [cap + 1], zeroed
    const int64_t* offs;   // [n_docs + 1] of x
    int64_t* out_offs;     // [n_docs + 1]
    int64_t n_docs;
    int64_t* n_out;        // the folded text's size
    const int32_t* ok;
};

__global__ __launch_bounds__(TB) void k_ug_fold_count(const FoldArgs a) {
    __shared__ int s_part[TB / 64];
    if (!*a.ok) return;
    const int64_t k = blockIdx.x, at = k * U::CHUNK_BYTES + (int64_t)threadIdx.x * U::SLICE_BYTES;
    const int64_t e = at + U::SLICE_BYTES < a.x.n ? at + U::SLICE_BYTES : a.x.n;
    const int mine = at < e ? (int)U::fold_range(a.x, at, e, a.flags, nullptr) : 0;
    int total;
    const int before = hutk::block_excl(mine, s_part, total);
    a.slice[k * TB + threadIdx.x] = (uint16_t)before;  // (at most 2 * CHUNK_BYTES: a byte folds to at most two)
    if (threadIdx.x == 0) a.chunk[k] = total;
}

constexpr int SCAN_TB = 1024, SCAN_PER = 16;
// exclusive scan of v[0 .. n) in place, v[n] = the sum; blockIdx.x selects one of the arrays v + blockIdx.x * stride
__global__ __launch_bounds__(SCAN_TB) void k_ug_scan(int64_t* v0, int64_t stride, int64_t n, const int32_t* ok) {
    __shared__ int64_t s_part[SCAN_TB / 64];
    if (!*ok) return;
    int64_t* v = v0 + blockIdx.x * stride;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    for (int64_t at = 0; at < n; at += SCAN_TB * SCAN_PER) {
        const int64_t i0 = at + (int64_t)tid * SCAN_PER;
        int64_t x[SCAN_PER], sum = 0;
#pragma unroll
        for (int j = 0; j < SCAN_PER; j++) {
            x[j] = i0 + j < n ? v[i0 + j] : 0;
            sum += x[j];
        }
        const int64_t incl = hutk::wave_incl(sum, lane);
        if (lane == 63) s_part[w] = incl;
        __syncthreads();
        int64_t before = carry + incl - sum, total = 0;
        for (int u = 0; u < SCAN_TB / 64; u++) {
            if (u < w) before += s_part[u];
            total += s_part[u];
        }
#pragma unroll
        for (int j = 0; j < SCAN_PER; j++) {
            if (i0 + j < n) v[i0 + j] = before;
            before += x[j];
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) v[n] = carry;
}

__global__ __launch_bounds__(TB) void k_ug_fold_write(const FoldArgs a) {
    if (!*a.ok) return;
    const int64_t k = blockIdx.x, at = k * U::CHUNK_BYTES + (int64_t)threadIdx.x * U::SLICE_BYTES;
    const int64_t e = at + U::SLICE_BYTES < a.x.n ? at + U::SLICE_BYTES : a.x.n;
    if (at < e) (void)U::fold_range(a.x, at, e, a.flags, a.out + a.chunk[k] + a.slice[k * TB + threadIdx.x]);
}

__global__ __launch_bounds__(TB) void k_ug_fold_docs(const FoldArgs a) {
    if (!*a.ok) return;
    const int64_t d = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (d > a.n_docs) return;
    const int64_t total = a.chunk[a.n_chunks];
    if (d == a.n_docs) {
        a.out_offs[d] = total;
        *a.n_out = total;
        return;
    }
    const int64_t o = a.offs[d];
    int64_t at = total;
    if (o < a.x.n) {
        const int64_t k = o / U::CHUNK_BYTES, s0 = o & ~(int64_t)(U::SLICE_BYTES - 1);
        at = a.chunk[k] + a.slice[k * TB + (s0 - k * U::CHUNK_BYTES) / U::SLICE_BYTES] + U::fold_range(a.x, s0, o, a.flags, nullptr);
    }
    a.out_offs[d] = at;
    a.out_flag[at] = 1;
}

struct MatchArgs {
    U::Text f;             // the folded text; f.n is the host's bound, *n_dev the size
    const int64_t* n_dev;
    U::Vocab V;
    int32_t ring, n_groups;  // positions of a group's ring (a power of two above max_len); groups of a workgroup that take words
    int32_t* tmp;          // [cap]: the id workspace
    U::Back* bp;           // [cap + 1]: the backpointers
    int64_t n_chunks;
    int64_t* chunk;        // two arrays of [n_chunks + 1]: ids and words per chunk, then their scans
    uint16_t* slice;       // [2][n_chunks * TB]: ids (words) of the chunk in front of the slice
    const int64_t* offs;   // [n_docs + 1] of f
    int64_t n_docs;
    int64_t* out_offs;
    int64_t* word_base;    // [n_docs + 1]: words in front of the document
    int32_t* ids;
    int64_t ids_cap;
    int32_t* word_ids;     // or NULL
    int32_t* err;
    const int32_t* ok;
};

__global__ __launch_bounds__(TB) void k_ug_fill(int32_t* tmp, const int64_t* n_dev, const int32_t* ok) {
    if (!*ok) return;
    const int64_t n = *n_dev;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) tmp[i] = -1;
}

// The lanes of a group run in one wavefront, in step: what one of them wrote to LDS the others read after this.
__device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// What the training form of the best path adds (hutk_unigram_train.h): a piece whose score is NaN
// is dead and no candidate, the unknown edge's score is *low - 10 (low: the lowest score alive, on the device), the
// score the word's end holds goes to fin[ws] (NaN: nothing reached it), and with bar the edge that spans the whole word
// is no candidate (it still counts as the single character's key).
struct TrainArgs {
    const double* low;
    double* fin;  // or NULL
    int32_t bar;
};

// The word that starts at ws, by the GROUP lanes of one group (all of them run this with the same arguments; gl: the
// lane's place in the group, g0: the group's first lane in the wavefront).  Starts are taken in rising order; of one
// start the lanes probe lengths base + 1 .. base + GROUP a trip, each lane the length base + gl + 1, over a hash the
// group walks together: a lane loads one byte a trip and the others read it by a shuffle.  Only lengths that some key
// with the start's first byte has are probed.  The word's end is found on the way: it has no length limit.
// ring: the group's R best scores, NaN where a position holds nothing; all NaN between words.
template <bool TRAIN>
__device__ __forceinline__ void lattice_word(const MatchArgs& a, const TrainArgs& t, const U::Text& f, int64_t ws, double* ring, int gl,
                                             int g0) {
    const int R1 = a.ring - 1;
    const uint8_t* w = f.bytes + ws;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (gl == 0) ring[0] = 0.0;
    int64_t s = 0;
    for (;;) {
        group_sync();
        const double here = ring[(int)(s & R1)];
        group_sync();
        if (gl == 0) ring[(int)(s & R1)] = nan;  // (the slot is position s + R's next)
        const uint64_t lens = a.V.lens[w[s]];
        const int top = U::top_len(lens, a.V.max_len);
        int end_at = INT32_MAX;  // the first index behind s at which the word ends, once a trip has seen it
        int m = 1;
        bool single = false;
        uint32_t state = U::HASH_INIT;  // of the bytes before the trip's
        for (int base = 0; base == 0 || (base < top && end_at == INT32_MAX); base += GROUP) {
            const int idx = base + gl;
            const int64_t q = ws + s + idx;
            const bool ends = idx > 0 && U::word_ends(f, q);
            const uint32_t mine = ends || q >= f.n ? 0u : f.bytes[q];
            const uint32_t em = (uint32_t)(__ballot(ends) >> g0) & ((1u << GROUP) - 1u);
            if (em) end_at = base + __ffs(em) - 1;
            uint32_t h = state;
#pragma unroll
            for (int j = 0; j < GROUP; j++) {
                const uint32_t bj = __shfl(mine, g0 + j);
                if (j <= gl) h = U::hash_step(h, bj);
            }
            state = __shfl(h, g0 + GROUP - 1);
            if (base == 0) m = U::char_len(f.bytes, ws + s, ws + s + (end_at < 4 ? end_at : 4));
            const int len = idx + 1;
            int32_t id = -1;
            if (len <= end_at && len <= top && U::has_len(lens, len)) id = U::find(a.V, U::hash_end(h), w + s, len);
            bool use = id >= 0;
            if constexpr (TRAIN) {
                if (id >= 0 && a.V.scores[id] != a.V.scores[id]) id = -1;
                use = id >= 0 && !(t.bar && s == 0 && U::word_ends(f, ws + len));  // (end_at is known only once a trip has seen the end)
            }
            if (use) {
                const double cand = a.V.scores[id] + here;
                double* cur = ring + (int)((s + len) & R1);
                if (U::replaces(cand, *cur)) {
                    *cur = cand;
                    a.bp[ws + s + len] = U::Back{id, len};
                }
            }
            single = single || ((uint32_t)(__ballot(id >= 0 && len == m) >> g0) & ((1u << GROUP) - 1u)) != 0;
        }
        if (!single && gl == 0) {  // (no lane wrote position s + m from this start)
            double cand = a.V.unk_score + here;
            if constexpr (TRAIN) cand = (*t.low - 10.0) + here;
            double* cur = ring + (int)((s + m) & R1);
            if (U::replaces(cand, *cur)) {
                *cur = cand;
                a.bp[ws + s + m] = U::Back{a.V.unk, m};
            }
        }
        s += m;
        if (m == end_at) break;  // (m <= end_at: a character does not reach past the word)
    }
    group_sync();
    if constexpr (TRAIN) {
        const double end = ring[(int)(s & R1)];
        if (gl == 0 && t.fin) t.fin[ws] = end;
        group_sync();
        if (gl == 0) ring[(int)(s & R1)] = nan;
        __threadfence_block();
        if (gl == 0 && end == end) U::backtrack(a.bp, a.V.unk, ws, s, a.tmp);
        return;
    }
    if (gl == 0) ring[(int)(s & R1)] = nan;
    __threadfence_block();  // the backpointers of the group's other lanes
    if (gl == 0) U::backtrack(a.bp, a.V.unk, ws, s, a.tmp);
}

// The word starts of the chunk at c0, in rising order, into s_ws (as offsets from c0) by the whole workgroup -> their count.
__device__ __forceinline__ int list_words(const U::Text& f, int64_t c0, int* s_part, uint16_t* s_ws) {
    const int tid = threadIdx.x;
    const int64_t at = c0 + (int64_t)tid * U::SLICE_BYTES;
    uint32_t starts = 0;  // bit i: a word starts at at + i
    for (int i = 0; i < U::SLICE_BYTES; i++)
        if (U::word_starts(f, at + i)) starts |= 1u << i;
    int n_words;
    int before = hutk::block_excl((int)__popc(starts), s_part, n_words);
    for (uint32_t m = starts; m; m &= m - 1) s_ws[before++] = (uint16_t)(tid * U::SLICE_BYTES + __ffs(m) - 1);
    return n_words;
}

__global__ __launch_bounds__(TB) void k_ug_lattice(const MatchArgs a) {
    extern __shared__ double s_ring[];  // [n_groups][ring]
    __shared__ int s_part[TB / 64];
    __shared__ int s_next;
    __shared__ uint16_t s_ws[U::CHUNK_BYTES];
    if (!*a.ok) return;
    U::Text f = a.f;
    f.n = *a.n_dev;
    const int64_t c0 = (int64_t)blockIdx.x * U::CHUNK_BYTES;
    if (c0 >= f.n) return;
    const int tid = threadIdx.x;
    const int n_words = list_words(f, c0, s_part, s_ws);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int i = tid; i < a.n_groups * a.ring; i += TB) s_ring[i] = nan;
    if (tid == 0) s_next = 0;
    __syncthreads();
    const int gl = tid & (GROUP - 1), g0 = (tid & 63) & ~(GROUP - 1), g = tid / GROUP;
    if (g >= a.n_groups) return;
    // the words are dealt as the groups come free: a long word holds its group, not its wavefront's other groups' share
    for (;;) {
        int i = 0;
        if (gl == 0) i = atomicAdd(&s_next, 1);
        i = __shfl(i, g0);
        if (i >= n_words) break;
        lattice_word<false>(a, TrainArgs{}, f, c0 + s_ws[i], s_ring + g * a.ring, gl, g0);
    }
}

// ---- a sampled segmentation (include/hutoken_amd.h: hutk_unigram_sample_batch_device) ----
struct SampleArgs {
    double alpha;
    uint64_t seed;
    int64_t first_doc;
    double* beta;  // [cap + 1]: beta of the character starts of the words that do not fit their group's ring
};

// bit j: the group's lane j says v
__device__ __forceinline__ uint32_t group_ballot(bool v, int g0) { return (uint32_t)(__ballot(v) >> g0) & ((1u << GROUP) - 1u); }

// Does a character of the word w[0 .. n) start at p?  A byte that is no continuation byte always does.  A continuation
// byte lies inside a character iff the nearest byte in front of it that is none -- at most three back, inside the word --
// starts a well-formed character that reaches past p; every other continuation byte is an ill-formed character of its own.
__device__ __forceinline__ bool char_starts(const uint8_t* w, int64_t p, int64_t n) {
    if ((w[p] & 0xC0u) != 0x80u) return true;
    for (int j = 1; j <= 3 && p - j >= 0; j++)
        if ((w[p - j] & 0xC0u) != 0x80u) return U::char_len(w, p - j, n) <= j;
    return true;
}

// One trip of the probes of the start s of the word w[0 .. n), for the filter and the sampler alike: lane gl takes the
// length base + gl + 1 over the hash the group walks together, exactly as lattice_word does.  -> the id of the lane's
// candidate or -1, and alpha * its score in *x.  The unknown edge stands in the first trip: its length m is at most 4, so
// it is lane m - 1's, which has no candidate of its own when no key is the single character.  state: the hash of the bytes
// before the trip's.
__device__ __forceinline__ int32_t sample_trip(const U::Vocab& V, double alpha, const uint8_t* w, int64_t s, int64_t n, int base,
                                               uint64_t lens, int top, int m, uint32_t& state, int gl, int g0, double* x) {
    const int idx = base + gl, len = idx + 1;
    const uint32_t mine = s + idx < n ? w[s + idx] : 0u;
    uint32_t h = state;
#pragma unroll
    for (int j = 0; j < GROUP; j++) {
        const uint32_t bj = __shfl(mine, g0 + j);
        if (j <= gl) h = U::hash_step(h, bj);
    }
    state = __shfl(h, g0 + GROUP - 1);
    int32_t id = -1;
    if (s + len <= n && len <= top && U::has_len(lens, len)) id = U::find(V, U::hash_end(h), w + s, len);
    double score = id >= 0 ? V.scores[id] : 0.0;
    if (base == 0) {
        const bool single = group_ballot(id >= 0 && len == m, g0) != 0;
        if (!single && len == m) id = V.unk, score = V.unk_score;
    }
    *x = alpha * score;
    return id;
}

// The word that starts at ws, by the GROUP lanes of one group (as lattice_word: all of them run this with the same
// arguments).  ring: the group's R values of beta; what another word left there is never read, because a candidate ends
// at a character start of this word, and those are written before they are read.
__device__ __forceinline__ void sample_word(const MatchArgs& a, const SampleArgs& sa, const U::Text& f, int64_t ws, double* ring, int gl,
                                            int g0) {
    const int R1 = a.ring - 1;
    const uint8_t* w = f.bytes + ws;
    int64_t n = 0;  // the word's bytes
    for (int64_t base = 1; n == 0; base += GROUP) {
        const uint32_t em = group_ballot(U::word_ends(f, ws + base + gl), g0);
        if (em) n = base + __ffs(em) - 1;
    }
    const bool in_lds = n < a.ring;  // every position of the word has a slot of its own: the sampler needs no global copy
    group_sync();                    // (the sampler of the group's last word has read the ring)
    if (gl == 0) ring[(int)(n & R1)] = 0.0;

    // the filter: beta[s] = log sum exp(alpha * score + beta[s + len]), the starts in falling order, eight positions a look
    for (int64_t hi = n - 1; hi >= 0; hi -= GROUP) {
        const int64_t p = hi - gl;
        for (uint32_t sm = group_ballot(p >= 0 && char_starts(w, p, n), g0); sm; sm &= sm - 1) {
            const int64_t s = hi - (__ffs(sm) - 1);
            group_sync();  // beta of the starts behind s
            const uint64_t lens = a.V.lens[w[s]];
            const int top = U::top_len(lens, a.V.max_len);
            const int m = U::char_len(w, s, n);
            double mx = -INFINITY, sum = 0.0;  // the lane's own candidates: their maximum, and the sum of exp(x - mx)
            uint32_t state = U::HASH_INIT;
            for (int base = 0; base == 0 || (base < top && s + base < n); base += GROUP) {
                double x;
                if (sample_trip(a.V, sa.alpha, w, s, n, base, lens, top, m, state, gl, g0, &x) < 0) continue;
                x += ring[(int)((s + base + gl + 1) & R1)];
                if (x > mx) {
                    sum = sum * exp(mx - x) + 1.0;
                    mx = x;
                } else {
                    sum += exp(x - mx);
                }
            }
            double top_x = mx;
#pragma unroll
            for (int d = 1; d < GROUP; d <<= 1) top_x = fmax(top_x, __shfl_xor(top_x, d));
            double total = sum * exp(mx - top_x);  // (a lane without a candidate: 0 * exp(-inf) = 0)
#pragma unroll
            for (int d = 1; d < GROUP; d <<= 1) total += __shfl_xor(total, d);
            if (gl == 0) {
                const double b = top_x + log(total);
                ring[(int)(s & R1)] = b;
                if (!in_lds) sa.beta[ws + s] = b;
            }
        }
    }
    if (!in_lds) __threadfence_block();  // lane 0's stores, for the group's other lanes
    group_sync();

    // the sampler: from the start, a draw a piece
    int64_t d = 0;
    for (int64_t hi = a.n_docs; hi - d > 1;) {  // the last document that starts at or before ws
        const int64_t mid = d + (hi - d) / 2;
        if (a.offs[mid] <= ws) d = mid;
        else hi = mid;
    }
    const int64_t row = sa.first_doc + d, in_doc = ws - a.offs[d];
    bool after_unk = false;
    for (int64_t s = 0; s < n;) {
        const hutk::Philox4 r = hutk::draw(sa.seed, row, (uint32_t)(uint64_t)(in_doc + s), hutk::DRAW_UNIGRAM);
        const double u = (double)(((uint64_t)r.x << 21) | (uint64_t)(r.y >> 11)) * 0x1p-53;
        const double here = in_lds ? ring[(int)(s & R1)] : sa.beta[ws + s];
        const uint64_t lens = a.V.lens[w[s]];
        const int top = U::top_len(lens, a.V.max_len);
        const int m = U::char_len(w, s, n);
        double carry = 0.0;  // p of the candidates of the trips before
        int32_t id = -1;     // the piece taken, or the last candidate so far
        int len = 0;
        uint32_t state = U::HASH_INIT;
        for (int base = 0; base == 0 || (base < top && s + base < n); base += GROUP) {
            double x;
            const int32_t mine = sample_trip(a.V, sa.alpha, w, s, n, base, lens, top, m, state, gl, g0, &x);
            double c = 0.0;
            if (mine >= 0) {
                const int64_t e = s + base + gl + 1;  // (byte ws + n of the workspace is the next word's first)
                c = exp(x + (in_lds ? ring[(int)(e & R1)] : e < n ? sa.beta[ws + e] : 0.0) - here);
            }
#pragma unroll
            for (int k = 1; k < GROUP; k <<= 1) {
                const double before = __shfl_up(c, k);
                if (gl >= k) c += before;
            }
            c += carry;
            const uint32_t cands = group_ballot(mine >= 0, g0), take = group_ballot(mine >= 0 && u < c, g0);
            const int from = take ? __ffs(take) - 1 : cands ? 31 - __clz(cands) : -1;
            if (from >= 0) id = __shfl(mine, g0 + from), len = base + from + 1;
            if (take) break;
            carry = __shfl(c, g0 + GROUP - 1);
        }
        const bool is_unk = id == a.V.unk;
        if (gl == 0 && !(is_unk && after_unk)) a.tmp[ws + s] = id | (s == 0 ? U::ID_START : 0);
        after_unk = is_unk;
        s += len;
    }
}

__global__ __launch_bounds__(TB) void k_ug_sample(const MatchArgs a, const SampleArgs sa) {
    extern __shared__ double s_ring[];  // [n_groups][ring]
    __shared__ int s_part[TB / 64];
    __shared__ int s_next;
    __shared__ uint16_t s_ws[U::CHUNK_BYTES];
    if (!*a.ok) return;
    U::Text f = a.f;
    f.n = *a.n_dev;
    const int64_t c0 = (int64_t)blockIdx.x * U::CHUNK_BYTES;
    if (c0 >= f.n) return;
    const int tid = threadIdx.x;
    const int n_words = list_words(f, c0, s_part, s_ws);
    if (tid == 0) s_next = 0;
    __syncthreads();
    const int gl = tid & (GROUP - 1), g0 = (tid & 63) & ~(GROUP - 1), g = tid / GROUP;
    if (g >= a.n_groups) return;
    for (;;) {
        int i = 0;
        if (gl == 0) i = atomicAdd(&s_next, 1);
        i = __shfl(i, g0);
        if (i >= n_words) break;
        sample_word(a, sa, f, c0 + s_ws[i], s_ring + g * a.ring, gl, g0);
    }
}

__global__ __launch_bounds__(TB) void k_ug_count(const MatchArgs a) {
    __shared__ int s_part[TB / 64];
    if (!*a.ok) return;
    const int64_t n = *a.n_dev;
    const int64_t k = blockIdx.x, c0 = k * U::CHUNK_BYTES;
    if (c0 >= n) return;
    const int64_t at = c0 + (int64_t)threadIdx.x * U::SLICE_BYTES;
    int ids = 0, words = 0;
    for (int64_t p = at; p < at + U::SLICE_BYTES && p < n; p++) {
        const int32_t v = a.tmp[p];
        ids += v >= 0;
        words += v >= 0 && (v & U::ID_START);
    }
    int total;
    int before = hutk::block_excl(ids, s_part, total);
    a.slice[k * TB + threadIdx.x] = (uint16_t)before;
    if (threadIdx.x == 0) a.chunk[k] = total;
    before = hutk::block_excl(words, s_part, total);
    a.slice[(a.n_chunks + k) * TB + threadIdx.x] = (uint16_t)before;
    if (threadIdx.x == 0) a.chunk[a.n_chunks + 1 + k] = total;
}

// ids (which = 0) or words (1) in front of folded byte o
__device__ __forceinline__ int64_t rank_before(const MatchArgs& a, int64_t n, int64_t o, int which) {
    const int64_t* chunk = a.chunk + which * (a.n_chunks + 1);
    if (o >= n) return chunk[a.n_chunks];
    const int64_t k = o / U::CHUNK_BYTES, s0 = o & ~(int64_t)(U::SLICE_BYTES - 1);
    int64_t r = chunk[k] + a.slice[(which * a.n_chunks + k) * TB + (s0 - k * U::CHUNK_BYTES) / U::SLICE_BYTES];
    for (int64_t p = s0; p < o; p++) {
        const int32_t v = a.tmp[p];
        r += which ? v >= 0 && (v & U::ID_START) : v >= 0;
    }
    return r;
}

__global__ __launch_bounds__(TB) void k_ug_docs(const MatchArgs a) {
    if (!*a.ok) return;
    const int64_t n = *a.n_dev;
    const int64_t d = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (d > a.n_docs) return;
    if (a.chunk[a.n_chunks] > a.ids_cap) {  // nothing is written into buffers the ids do not fit
        if (d == 0) note_error(a.err, HUTK_E_CAPACITY);
        return;
    }
    const int64_t o = a.offs[d];
    a.out_offs[d] = rank_before(a, n, o, 0);
    if (a.word_ids) a.word_base[d] = rank_before(a, n, o, 1);
}

__global__ __launch_bounds__(TB) void k_ug_write(const MatchArgs a) {
    if (!*a.ok) return;
    const int64_t n = *a.n_dev;
    const int64_t k = blockIdx.x, c0 = k * U::CHUNK_BYTES;
    if (c0 >= n || a.chunk[a.n_chunks] > a.ids_cap) return;
    const int64_t at = c0 + (int64_t)threadIdx.x * U::SLICE_BYTES;
    int64_t to = a.chunk[k] + a.slice[k * TB + threadIdx.x];
    int64_t word = a.word_ids ? a.chunk[a.n_chunks + 1 + k] + a.slice[(a.n_chunks + k) * TB + threadIdx.x] : 0;
    int64_t d = -1;
    for (int64_t p = at; p < at + U::SLICE_BYTES && p < n; p++) {
        const int32_t v = a.tmp[p];
        if (v < 0) continue;
        a.ids[to] = v & U::ID_MASK;
        if (a.word_ids) {
            word += (v & U::ID_START) != 0;
            // the document of the id: that of the word, and ids lie inside their word's bytes
            if (d < 0) {
                int64_t lo = 0, hi = a.n_docs;  // the last document that starts at or before p
                while (hi - lo > 1) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (a.offs[mid] <= p) lo = mid;
                    else hi = mid;
                }
                d = lo;
            }
            while (d + 1 < a.n_docs && a.offs[d + 1] <= p) d++;
            a.word_ids[to] = (int32_t)(word - 1 - a.word_base[d]);
        }
        to++;
    }
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + TB) / TB); }

}  // namespace

struct hutk_unigram {
    int device = 0;
    uint32_t flags = 0;
    int32_t unk = 0, max_len = 0, ring = 16, n_groups = GROUPS;
    int64_t n_pieces = 0, n_slots = 0;
    DevBuf<uint8_t> d_keys, w_flag[2], w_text, s_bytes;
    DevBuf<U::Slot> d_slots;
    DevBuf<double> d_scores;
    DevBuf<uint64_t> d_lens;
    DevBuf<U::Back> w_bp;
    DevBuf<int64_t> w_offs, w_chunk, w_small, w_word_base, s_offs, s_oo;
    DevBuf<uint16_t> w_slice;
    DevBuf<int32_t> w_tmp, w_ok, s_ids, s_wids;
    U::Vocab V{};
    // training (hutk_unigram_train.h): the lowest score alive, the M-step's sums, and what a prune keeps between its calls
    // -- the key blob's flags, the best path of every key with its spanning edge barred, that path's score, the classes
    int64_t n_key_bytes = 0;
    bool train_ready = false;
    DevBuf<double> t_low, t_fin;
    DevBuf<uint8_t> t_kflag;
    DevBuf<int32_t> t_alt, t_class;
    DevBuf<U::Back> t_kbp;
    std::mutex mu;
    hipEvent_t ev = nullptr;  // behind the last kernel of the last call: calls share the workspace, so they are serialised
    bool ev_recorded = false;
};

extern "C" {

int hutk_debug_unigram_chunk_bytes(void) { return U::CHUNK_BYTES; }

void hutk_unigram_destroy(hutk_unigram* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev) {
        if (h->ev_recorded) (void)hipEventSynchronize(h->ev);  // nothing is freed under a running kernel
        (void)hipEventDestroy(h->ev);
    }
    h->d_keys.release(); h->w_text.release(); h->s_bytes.release(); h->d_slots.release(); h->d_scores.release(); h->d_lens.release();
    h->w_bp.release(); h->w_offs.release(); h->w_chunk.release(); h->w_small.release(); h->w_word_base.release(); h->s_offs.release();
    h->s_oo.release(); h->w_slice.release(); h->w_tmp.release(); h->w_ok.release(); h->s_ids.release(); h->s_wids.release();
    for (int i = 0; i < 2; i++) h->w_flag[i].release();
    h->t_low.release(); h->t_fin.release(); h->t_kflag.release(); h->t_alt.release(); h->t_class.release(); h->t_kbp.release();
    delete h;
}

int hutk_unigram_create(hutk_unigram** out, int device, const uint8_t* piece_bytes, const int64_t* piece_offsets, const double* scores,
                        int64_t n_pieces, int64_t unk_id, uint32_t flags) {
    if (!out) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_create: out is NULL");
    *out = nullptr;
    if (!piece_offsets || n_pieces < 0 || (n_pieces > 0 && (!scores || (piece_offsets[n_pieces] > 0 && !piece_bytes))))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_create: bad arguments");
    if (flags & ~(U::F_PREPEND | U::F_WS_SPLIT | U::F_COLLAPSE))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_create: flags holds bits that are no HUTK_UG_* flag");
    if ((flags & U::F_WS_SPLIT) && !(flags & U::F_PREPEND))
        return hutk::api_set_error(HUTK_E_VALUE, "hutk_unigram_create: HUTK_UG_WHITESPACE_SPLIT needs HUTK_UG_PREPEND");
    U::VocabHost vh;
    std::string why;
    if (int bad = U::build_vocab(piece_bytes, piece_offsets, scores, n_pieces, unk_id, vh, &why))
        return hutk::api_set_error(bad == 1 ? HUTK_E_VALUE : HUTK_E_ARG, "hutk_unigram_create: " + why);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_unigram_create: no HIP device");
    if (device < 0) HUTK_HIP_TRY(hipGetDevice(&device));
    if (device >= n) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_unigram_create: no such device");
    HUTK_HIP_TRY(hipSetDevice(device));
    hutk_unigram* h = new hutk_unigram();
    h->device = device;
    h->flags = flags, h->unk = (int32_t)unk_id, h->max_len = vh.max_len, h->n_pieces = n_pieces, h->n_slots = (int64_t)vh.slots.size();
    h->n_key_bytes = (int64_t)vh.keys.size();
    h->ring = U::ring_size(vh.max_len);
    h->n_groups = std::min(GROUPS, RING_LDS_BYTES / (8 * h->ring));
    hipError_t e = h->d_slots.reserve(vh.slots.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_slots.p, vh.slots.data(), vh.slots.size() * sizeof(U::Slot), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->d_keys.reserve(vh.keys.size() + 16);
    if (e == hipSuccess && !vh.keys.empty()) e = hipMemcpy(h->d_keys.p, vh.keys.data(), vh.keys.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->d_scores.reserve((size_t)n_pieces);
    if (e == hipSuccess) e = hipMemcpy(h->d_scores.p, scores, (size_t)n_pieces * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->d_lens.reserve(256);
    if (e == hipSuccess) e = hipMemcpy(h->d_lens.p, vh.lens.data(), 256 * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->w_ok.reserve(2);
    if (e == hipSuccess) e = h->w_small.reserve(8);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        hutk_unigram_destroy(h);
        return hutk::api_set_error(e == hipErrorOutOfMemory ? HUTK_E_MEMORY : HUTK_E_DEVICE,
                                   std::string("hutk_unigram_create: ") + hipGetErrorString(e));
    }
    h->V = vh.view(h->d_slots.p, h->d_keys.p, h->d_scores.p, h->d_lens.p, h->unk);
    *out = h;
    return HUTK_OK;
}

int hutk_unigram_info(const hutk_unigram* h, int64_t* out8) {
    if (!h || !out8) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_info: bad arguments");
    out8[0] = U::CHUNK_BYTES;
    out8[1] = h->n_pieces;
    out8[2] = h->n_slots;
    out8[3] = h->flags;
    out8[4] = h->unk;
    out8[5] = h->max_len;
    out8[6] = U::MAX_PIECE;
    out8[7] = GROUP;
    return HUTK_OK;
}

int64_t hutk_debug_unigram_bucket(const hutk_unigram* h, const uint8_t* bytes, int64_t len) {
    if (!h || len < 0 || len > INT32_MAX || (len > 0 && !bytes)) return -1;
    return (int64_t)(U::piece_hash(bytes, (int)len) & (uint32_t)(h->n_slots - 1));
}

/* An id covers at least one character of the folded text, and the fold adds at most one character per document. */
int64_t hutk_unigram_ids_capacity(const hutk_unigram* h, int64_t n_bytes, int64_t n_docs) {
    if (!h || n_bytes < 0 || n_docs < 0) return -1;
    return n_bytes + n_docs;
}

}  // extern "C"

// What every device entry starts with (the caller holds h->mu and has checked h and the batch's arguments): the
// workspace, the wait for the handle's last call, the check of the offsets, the fold, and the emptied id workspace.
// -> m: the folded text and the handle's workspace, without the outputs of an encode; chunks: those of the folded text.
static int ug_front(hutk_unigram* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes, bool word_ids,
                    int32_t* d_err, hipStream_t st, const std::string& who, MatchArgs& m, int64_t& chunks) {
    const int64_t cap_f = n_bytes + n_docs;  // the folded text's bound
    const int64_t src_chunks = (n_bytes + U::CHUNK_BYTES - 1) / U::CHUNK_BYTES;
    chunks = (cap_f + U::CHUNK_BYTES - 1) / U::CHUNK_BYTES;
    if (chunks > INT32_MAX / 2 || (n_docs + TB) / TB > INT32_MAX)
        return hutk::api_set_error(HUTK_E_UNSUPPORTED, who + ": the batch is too large for one launch");
    HUTK_HIP_TRY(hipSetDevice(h->device));
    HUTK_HIP_TRY(h->w_flag[0].reserve((size_t)n_bytes + 1));
    HUTK_HIP_TRY(h->w_flag[1].reserve((size_t)cap_f + 1));
    HUTK_HIP_TRY(h->w_text.reserve((size_t)cap_f + 16));
    HUTK_HIP_TRY(h->w_offs.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(h->w_chunk.reserve(2 * ((size_t)chunks + 1)));
    HUTK_HIP_TRY(h->w_slice.reserve(2 * (size_t)chunks * TB + 1));
    HUTK_HIP_TRY(h->w_tmp.reserve((size_t)cap_f + 1));
    HUTK_HIP_TRY(h->w_bp.reserve((size_t)cap_f + 1));
    if (word_ids) HUTK_HIP_TRY(h->w_word_base.reserve((size_t)n_docs + 1));
    if (h->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
    int32_t* ok = h->w_ok.p;
    int32_t* err = d_err ? d_err : h->w_ok.p + 1;
    HUTK_HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), st));
    HUTK_HIP_TRY(hipMemsetAsync(ok, 1, sizeof(int32_t), st));  // (bytes of 1: any value but 0 says "sound")
    hipLaunchKernelGGL(k_ug_check, dim3(blocks_for(n_docs)), dim3(TB), 0, st, d_offsets, n_docs, n_bytes, ok, err);
    HUTK_HIP_TRY(hipMemsetAsync(h->w_flag[0].p, 0, (size_t)n_bytes + 1, st));
    hipLaunchKernelGGL(k_ug_flags, dim3(blocks_for(n_docs)), dim3(TB), 0, st, d_offsets, n_docs, h->w_flag[0].p, ok);

    int64_t* n_fold = h->w_small.p;
    FoldArgs fa;
    fa.x = U::Text{d_bytes, h->w_flag[0].p, n_bytes}, fa.flags = h->flags;
    fa.chunk = h->w_chunk.p, fa.n_chunks = src_chunks, fa.slice = h->w_slice.p;
    fa.out = h->w_text.p, fa.out_flag = h->w_flag[1].p;
    fa.offs = d_offsets, fa.out_offs = h->w_offs.p, fa.n_docs = n_docs, fa.n_out = n_fold, fa.ok = ok;
    HUTK_HIP_TRY(hipMemsetAsync(fa.chunk, 0, ((size_t)src_chunks + 1) * sizeof(int64_t), st));
    HUTK_HIP_TRY(hipMemsetAsync(fa.out_flag, 0, (size_t)cap_f + 1, st));
    HUTK_HIP_TRY(hipMemsetAsync(n_fold, 0, sizeof(int64_t), st));
    if (src_chunks) hipLaunchKernelGGL(k_ug_fold_count, dim3((unsigned)src_chunks), dim3(TB), 0, st, fa);
    hipLaunchKernelGGL(k_ug_scan, dim3(1), dim3(SCAN_TB), 0, st, fa.chunk, (int64_t)0, src_chunks, ok);
    if (src_chunks) hipLaunchKernelGGL(k_ug_fold_write, dim3((unsigned)src_chunks), dim3(TB), 0, st, fa);
    hipLaunchKernelGGL(k_ug_fold_docs, dim3(blocks_for(n_docs)), dim3(TB), 0, st, fa);

    m.f = U::Text{h->w_text.p, h->w_flag[1].p, cap_f}, m.n_dev = n_fold, m.V = h->V, m.ring = h->ring, m.n_groups = h->n_groups;
    m.tmp = h->w_tmp.p, m.bp = h->w_bp.p;
    m.n_chunks = chunks, m.chunk = h->w_chunk.p, m.slice = h->w_slice.p;
    m.offs = h->w_offs.p, m.n_docs = n_docs, m.out_offs = nullptr, m.word_base = h->w_word_base.p;
    m.ids = nullptr, m.ids_cap = 0, m.word_ids = nullptr, m.err = err, m.ok = ok;
    HUTK_HIP_TRY(hipMemsetAsync(m.chunk, 0, 2 * ((size_t)chunks + 1) * sizeof(int64_t), st));
    if (chunks) {
        const unsigned fill = (unsigned)std::min<int64_t>((cap_f + TB - 1) / TB, 1 << 16);
        hipLaunchKernelGGL(k_ug_fill, dim3(fill), dim3(TB), 0, st, m.tmp, n_fold, ok);
    }
    return HUTK_OK;
}

// Behind a call's last kernel: what was enqueued is checked, and the next call on the handle waits for it.
static int ug_back(hutk_unigram* h, hipStream_t st) {
    HUTK_HIP_TRY(hipGetLastError());
    HUTK_HIP_TRY(hipEventRecord(h->ev, st));
    h->ev_recorded = true;
    return HUTK_OK;
}

// Both device entries: the best path (sample NULL), or a sampled segmentation with sample's alpha, seed and first_doc.
static int ug_encode_device(hutk_unigram* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                            int32_t* d_ids, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_word_ids, int32_t* d_err, void* hip_stream,
                            const SampleArgs* sample, const std::string& who) {
    if (!h) return hutk::api_set_error(HUTK_E_ARG, who + ": the handle is NULL");
    if (n_docs < 0 || n_bytes < 0 || ids_cap < 0 || !d_offsets || !d_out_offsets || (n_bytes > 0 && !d_bytes) || (ids_cap > 0 && !d_ids))
        return hutk::api_set_error(HUTK_E_ARG, who + ": bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    MatchArgs m;
    int64_t chunks = 0;
    if (int rc = ug_front(h, d_bytes, d_offsets, n_docs, n_bytes, d_word_ids != nullptr, d_err, st, who, m, chunks)) return rc;
    const int32_t* ok = m.ok;
    m.out_offs = d_out_offsets, m.ids = d_ids, m.ids_cap = ids_cap, m.word_ids = d_word_ids;
    if (chunks) {
        const size_t rings = (size_t)h->n_groups * h->ring * sizeof(double);
        if (sample) {
            SampleArgs sa = *sample;
            sa.beta = reinterpret_cast<double*>(h->w_bp.p);  // (this path has no backpointers: their workspace, 8 bytes a byte as well)
            hipLaunchKernelGGL(k_ug_sample, dim3((unsigned)chunks), dim3(TB), rings, st, m, sa);
        } else {
            hipLaunchKernelGGL(k_ug_lattice, dim3((unsigned)chunks), dim3(TB), rings, st, m);
        }
        hipLaunchKernelGGL(k_ug_count, dim3((unsigned)chunks), dim3(TB), 0, st, m);
    }
    hipLaunchKernelGGL(k_ug_scan, dim3(2), dim3(SCAN_TB), 0, st, m.chunk, chunks + 1, chunks, ok);
    hipLaunchKernelGGL(k_ug_docs, dim3(blocks_for(n_docs)), dim3(TB), 0, st, m);
    if (chunks) hipLaunchKernelGGL(k_ug_write, dim3((unsigned)chunks), dim3(TB), 0, st, m);
    return ug_back(h, st);
}

#include "hutk_unigram_train.h"  // the training kernels and their entry points, over everything above
#include "hutk_unigram_seed.h"   // the seed of a training: unique words, characters and substrings of a corpus

extern "C" {

int hutk_unigram_encode_batch_device(hutk_unigram* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                                     int32_t* d_ids, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_word_ids, int32_t* d_err,
                                     void* hip_stream) {
    return ug_encode_device(h, d_bytes, d_offsets, n_docs, n_bytes, d_ids, ids_cap, d_out_offsets, d_word_ids, d_err, hip_stream, nullptr,
                            "hutk_unigram_encode_batch_device");
}

int hutk_unigram_sample_batch_device(hutk_unigram* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                                     int32_t* d_ids, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_word_ids, const double* alpha,
                                     uint64_t seed, int64_t first_doc, int32_t* d_err, void* hip_stream) {
    if (!alpha || first_doc < 0 || (n_docs > 0 && first_doc > INT64_MAX - n_docs))  // (first_doc + d stays an int64)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_sample_batch_device: bad arguments");
    if (!std::isfinite(*alpha)) return hutk::api_set_error(HUTK_E_VALUE, "hutk_unigram_sample_batch_device: alpha is not finite");
    const SampleArgs sa{*alpha, seed, first_doc, nullptr};
    return ug_encode_device(h, d_bytes, d_offsets, n_docs, n_bytes, d_ids, ids_cap, d_out_offsets, d_word_ids, d_err, hip_stream, &sa,
                            "hutk_unigram_sample_batch_device");
}

int hutk_unigram_encode_batch(hutk_unigram* h, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, int32_t** out_ids,
                              int64_t** out_offsets, int32_t** out_word_ids) {
    if (!h || !out_ids || !out_offsets || n_docs < 0 || !offsets) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_encode_batch: bad arguments");
    *out_ids = nullptr;
    *out_offsets = nullptr;
    if (out_word_ids) *out_word_ids = nullptr;
    if (int rc = hutk::check_offsets(offsets, n_docs, true, "offsets")) return rc;
    const int64_t n_bytes = offsets[n_docs];
    if (n_bytes > 0 && !bytes) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_encode_batch: bytes is NULL");
    const int64_t cap = hutk_unigram_ids_capacity(h, n_bytes, n_docs);
    HUTK_HIP_TRY(hipSetDevice(h->device));
    {
        std::lock_guard<std::mutex> lock(h->mu);
        HUTK_HIP_TRY(h->s_bytes.reserve((size_t)n_bytes + 16));
        HUTK_HIP_TRY(h->s_offs.reserve((size_t)n_docs + 1));
        HUTK_HIP_TRY(h->s_oo.reserve((size_t)n_docs + 1));
        HUTK_HIP_TRY(h->s_ids.reserve((size_t)cap + 1));
        if (out_word_ids) HUTK_HIP_TRY(h->s_wids.reserve((size_t)cap + 1));
        if (h->ev_recorded) HUTK_HIP_TRY(hipEventSynchronize(h->ev));  // (the staging buffers are the handle's)
        if (n_bytes) HUTK_HIP_TRY(hipMemcpy(h->s_bytes.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice));
        HUTK_HIP_TRY(hipMemcpy(h->s_offs.p, offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    }
    if (int rc = hutk_unigram_encode_batch_device(h, h->s_bytes.p, h->s_offs.p, n_docs, n_bytes, h->s_ids.p, cap, h->s_oo.p,
                                                  out_word_ids ? h->s_wids.p : nullptr, nullptr, nullptr))
        return rc;
    HUTK_HIP_TRY(hipStreamSynchronize(nullptr));
    int32_t err = 0;
    HUTK_HIP_TRY(hipMemcpy(&err, h->w_ok.p + 1, 4, hipMemcpyDeviceToHost));
    if (err) return hutk::api_set_error(err, "hutk_unigram_encode_batch: device-side failure");
    int64_t* oo = (int64_t*)hutk_host_alloc((size_t)(n_docs + 1) * 8);
    if (!oo) return hutk::api_set_error(HUTK_E_MEMORY, "hutk_unigram_encode_batch: out of host memory");
    hipError_t e = hipMemcpy(oo, h->s_oo.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost);
    const int64_t total = e == hipSuccess ? oo[n_docs] : 0;
    int32_t* ids = (int32_t*)hutk_host_alloc((size_t)(total > 0 ? total : 1) * 4);
    int32_t* wids = out_word_ids ? (int32_t*)hutk_host_alloc((size_t)(total > 0 ? total : 1) * 4) : nullptr;
    if (e == hipSuccess && (!ids || (out_word_ids && !wids))) {
        hutk_host_free(oo);
        if (ids) hutk_host_free(ids);
        if (wids) hutk_host_free(wids);
        return hutk::api_set_error(HUTK_E_MEMORY, "hutk_unigram_encode_batch: out of host memory");
    }
    if (e == hipSuccess && total) e = hipMemcpy(ids, h->s_ids.p, (size_t)total * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && total && wids) e = hipMemcpy(wids, h->s_wids.p, (size_t)total * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        hutk_host_free(oo);
        if (ids) hutk_host_free(ids);
        if (wids) hutk_host_free(wids);
        HUTK_HIP_TRY(e);
    }
    *out_ids = ids;
    *out_offsets = oo;
    if (out_word_ids) *out_word_ids = wids;
    return HUTK_OK;
}

}  // extern "C"
