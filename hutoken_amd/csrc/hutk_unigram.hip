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
//   k_ug_count       ids and words per slice and chunk;  k_ug_scan over both
//   k_ug_docs        out_offsets, and the word count in front of every document
//   k_ug_write       the ids, compact, and the word ids
//
// Nothing synchronises; growing the workspace for a batch larger than any before may wait once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "hutk_host.h"
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

// The word that starts at ws, by the GROUP lanes of one group (all of them run this with the same arguments; gl: the
// lane's place in the group, g0: the group's first lane in the wavefront).  Starts are taken in rising order; of one
// start the lanes probe lengths base + 1 .. base + GROUP a trip, each lane the length base + gl + 1, over a hash the
// group walks together: a lane loads one byte a trip and the others read it by a shuffle.  Only lengths that some key
// with the start's first byte has are probed.  The word's end is found on the way: it has no length limit.
// ring: the group's R best scores, NaN where a position holds nothing; all NaN between words.
__device__ __forceinline__ void lattice_word(const MatchArgs& a, const U::Text& f, int64_t ws, double* ring, int gl, int g0) {
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
            if (id >= 0) {
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
            const double cand = a.V.unk_score + here;
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
    if (gl == 0) ring[(int)(s & R1)] = nan;
    __threadfence_block();  // the backpointers of the group's other lanes
    if (gl == 0) U::backtrack(a.bp, a.V.unk, ws, s, a.tmp);
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
    const int64_t at = c0 + (int64_t)tid * U::SLICE_BYTES;
    uint32_t starts = 0;  // bit i: a word starts at at + i
    for (int i = 0; i < U::SLICE_BYTES; i++)
        if (U::word_starts(f, at + i)) starts |= 1u << i;
    int n_words;
    int before = hutk::block_excl((int)__popc(starts), s_part, n_words);
    for (uint32_t m = starts; m; m &= m - 1) s_ws[before++] = (uint16_t)(tid * U::SLICE_BYTES + __ffs(m) - 1);
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
        lattice_word(a, f, c0 + s_ws[i], s_ring + g * a.ring, gl, g0);
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

int hutk_unigram_encode_batch_device(hutk_unigram* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                                     int32_t* d_ids, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_word_ids, int32_t* d_err,
                                     void* hip_stream) {
    if (!h) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_encode_batch_device: the handle is NULL");
    if (n_docs < 0 || n_bytes < 0 || ids_cap < 0 || !d_offsets || !d_out_offsets || (n_bytes > 0 && !d_bytes) || (ids_cap > 0 && !d_ids))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_encode_batch_device: bad arguments");
    const int64_t cap_f = n_bytes + n_docs;  // the folded text's bound
    const int64_t src_chunks = (n_bytes + U::CHUNK_BYTES - 1) / U::CHUNK_BYTES, chunks = (cap_f + U::CHUNK_BYTES - 1) / U::CHUNK_BYTES;
    if (chunks > INT32_MAX / 2 || (n_docs + TB) / TB > INT32_MAX)
        return hutk::api_set_error(HUTK_E_UNSUPPORTED, "hutk_unigram_encode_batch_device: the batch is too large for one launch");
    std::lock_guard<std::mutex> lock(h->mu);
    HUTK_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(h->w_flag[0].reserve((size_t)n_bytes + 1));
    HUTK_HIP_TRY(h->w_flag[1].reserve((size_t)cap_f + 1));
    HUTK_HIP_TRY(h->w_text.reserve((size_t)cap_f + 16));
    HUTK_HIP_TRY(h->w_offs.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(h->w_chunk.reserve(2 * ((size_t)chunks + 1)));
    HUTK_HIP_TRY(h->w_slice.reserve(2 * (size_t)chunks * TB + 1));
    HUTK_HIP_TRY(h->w_tmp.reserve((size_t)cap_f + 1));
    HUTK_HIP_TRY(h->w_bp.reserve((size_t)cap_f + 1));
    if (d_word_ids) HUTK_HIP_TRY(h->w_word_base.reserve((size_t)n_docs + 1));
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

    MatchArgs m;
    m.f = U::Text{h->w_text.p, h->w_flag[1].p, cap_f}, m.n_dev = n_fold, m.V = h->V, m.ring = h->ring, m.n_groups = h->n_groups;
    m.tmp = h->w_tmp.p, m.bp = h->w_bp.p;
    m.n_chunks = chunks, m.chunk = h->w_chunk.p, m.slice = h->w_slice.p;
    m.offs = h->w_offs.p, m.n_docs = n_docs, m.out_offs = d_out_offsets, m.word_base = h->w_word_base.p;
    m.ids = d_ids, m.ids_cap = ids_cap, m.word_ids = d_word_ids, m.err = err, m.ok = ok;
    HUTK_HIP_TRY(hipMemsetAsync(m.chunk, 0, 2 * ((size_t)chunks + 1) * sizeof(int64_t), st));
    if (chunks) {
        const unsigned fill = (unsigned)std::min<int64_t>((cap_f + TB - 1) / TB, 1 << 16);
        hipLaunchKernelGGL(k_ug_fill, dim3(fill), dim3(TB), 0, st, m.tmp, n_fold, ok);
        hipLaunchKernelGGL(k_ug_lattice, dim3((unsigned)chunks), dim3(TB), (size_t)h->n_groups * h->ring * sizeof(double), st, m);
        hipLaunchKernelGGL(k_ug_count, dim3((unsigned)chunks), dim3(TB), 0, st, m);
    }
    hipLaunchKernelGGL(k_ug_scan, dim3(2), dim3(SCAN_TB), 0, st, m.chunk, chunks + 1, chunks, ok);
    hipLaunchKernelGGL(k_ug_docs, dim3(blocks_for(n_docs)), dim3(TB), 0, st, m);
    if (chunks) hipLaunchKernelGGL(k_ug_write, dim3((unsigned)chunks), dim3(TB), 0, st, m);
    HUTK_HIP_TRY(hipGetLastError());
    HUTK_HIP_TRY(hipEventRecord(h->ev, st));
    h->ev_recorded = true;
    return HUTK_OK;
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
