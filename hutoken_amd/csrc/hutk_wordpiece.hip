// hutk_wordpiece.hip -- WordPiece encoding of a packed batch on the GPU (include/hutoken_amd.h):
// (uint8 bytes, int64 offsets[n + 1]) in, the ragged (int32 ids, int64 out_offsets[n + 1]) of hutk_encode_batch_device
// out, and on request the word index of every id.  The rule -- classes, fold, character grid, word starts, hash and
// probe -- is hutk_wordpiece.h, shared with the CPU check; this file is the chunking, the placement and the C entry points.
//
// A text is cut into chunks of CHUNK_BYTES and those into slices of 16 bytes, a lane each.  Sizes that only the device
// knows (the folded text's, the ids') are read from device memory: a grid is sized by the host's bound and the
// workgroups behind the real end leave at once.
//
//   k_wp_check     the offsets describe the bytes (else HUTK_E_ARG and nothing else is written)
//   k_wp_flags     flag[p] = a document starts at p
//   fold, once (or twice around NFD with strip_accents: clean first, marks and lower case after it):
//     k_wp_fold_count   every lane counts what the characters that start in its slice fold to; a workgroup scan gives
//                       the slice's place in the chunk and the chunk's size
//     k_wp_scan         exclusive scan over the chunks (one workgroup)
//     k_wp_fold_write   every lane folds again and writes from its place
//     k_wp_fold_docs    the folded offsets and flags of the documents
//   match:
//     k_wp_fill         the id workspace, one int32 per folded byte, is emptied
//     k_wp_match        word starts by class; a group of 8 lanes owns a word and probes 8 candidate ends a trip, longest
//                       first; the ids of the word that starts at byte w go to workspace[w], [w + 1], ..
//     k_wp_count        ids and words per slice and chunk;  k_wp_scan over both
//     k_wp_docs         out_offsets, and the word count in front of every document
//     k_wp_write        the ids, compact, and the word ids
//
// Nothing synchronises; growing the workspace for a batch larger than any before may wait once.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "hutk_host.h"
#include "hutk_wave.h"
#include "hutk_wordpiece.h"

namespace {

namespace W = hutk::wp;
namespace N = hutk::norm;

constexpr int TB = W::CHUNK_SLICES;  // 256 lanes: a slice each
static_assert(TB == 256 && W::SLICE_BYTES == 16, "a lane owns 16 bytes");
constexpr int GROUP = 8;             // lanes that own a word
constexpr int GROUPS = TB / GROUP;

__device__ __forceinline__ void note_error(int32_t* err, int code) { atomicCAS(err, 0, code); }

__global__ __launch_bounds__(TB) void k_wp_check(const int64_t* offs, int64_t n_docs, int64_t n_bytes, int32_t* ok, int32_t* err) {
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
__global__ __launch_bounds__(TB) void k_wp_flags(const int64_t* offs, int64_t n_docs, uint8_t* flag, const int32_t* ok) {
    if (!*ok) return;
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i < n_docs) flag[offs[i]] = 1;
}

// one fold pass: text `x` with n_in bytes known to the device only (x.n is filled in by the kernel from *n_dev when set)
struct FoldArgs {
    W::Tables T;
    W::Text x;
    const int64_t* n_dev;  // the text's size when only the device knows it, else NULL and x.n holds
    uint32_t mode;
    int64_t* chunk;        // [n_chunks + 1]: sizes, then their exclusive scan and the total
    int64_t n_chunks;      // by the host's bound
    uint16_t* slice;       // [n_chunks * TB]: bytes of the chunk's output in front of the slice's
    uint8_t* out;
    uint8_t* out_flag;     // [cap + 1], zeroed
    const int64_t* offs;   // [n_docs + 1] of x
    int64_t* out_offs;     // [n_docs + 1]
    int64_t n_docs;
    int64_t* n_out;        // the folded text's size
    int64_t pad_to;        // >= 0: the output is padded with ' ' to this size, into the last document (the clean pass in
                           // front of NFD keeps the size the host knows; a space more or less changes no word)
    const int32_t* ok;
};

__device__ __forceinline__ W::Text text_of(const W::Text& x, const int64_t* n_dev) {
    W::Text t = x;
    if (n_dev) t.n = *n_dev;
    return t;
}

__global__ __launch_bounds__(TB) void k_wp_fold_count(const FoldArgs a) {
    __shared__ int64_t s_part[TB / 64];
    if (!*a.ok) return;
    const W::Text x = text_of(a.x, a.n_dev);
    const int64_t k = blockIdx.x, c0 = k * W::CHUNK_BYTES;
    if (c0 >= x.n) return;
    const int64_t at = c0 + (int64_t)threadIdx.x * W::SLICE_BYTES;
    const int64_t e = at + W::SLICE_BYTES < x.n ? at + W::SLICE_BYTES : x.n;
    const int64_t mine = at < e ? W::fold_range(a.T, x, at, e, a.mode, nullptr) : 0;
    int64_t total;
    const int64_t before = hutk::block_excl(mine, s_part, total);
    a.slice[k * TB + threadIdx.x] = (uint16_t)before;  // (at most 2 * CHUNK_BYTES: a character folds to at most twice its bytes)
    if (threadIdx.x == 0) a.chunk[k] = total;
}

constexpr int SCAN_TB = 1024, SCAN_PER = 16;
// exclusive scan of v[0 .. n) in place, v[n] = the sum; blockIdx.x selects one of the arrays v + blockIdx.x * stride
__global__ __launch_bounds__(SCAN_TB) void k_wp_scan(int64_t* v0, int64_t stride, int64_t n, const int32_t* ok) {
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

__global__ __launch_bounds__(TB) void k_wp_fold_write(const FoldArgs a) {
    if (!*a.ok) return;
    const W::Text x = text_of(a.x, a.n_dev);
    const int64_t k = blockIdx.x, c0 = k * W::CHUNK_BYTES;
    const int64_t total = a.chunk[a.n_chunks];
    if (a.pad_to >= 0) {  // (the pad lies behind every chunk's output: every workgroup of the grid helps to write it)
        for (int64_t i = total + (int64_t)blockIdx.x * TB + threadIdx.x; i < a.pad_to; i += (int64_t)gridDim.x * TB) a.out[i] = 0x20u;
    }
    if (c0 >= x.n) return;
    const int64_t at = c0 + (int64_t)threadIdx.x * W::SLICE_BYTES;
    const int64_t e = at + W::SLICE_BYTES < x.n ? at + W::SLICE_BYTES : x.n;
    if (at < e) (void)W::fold_range(a.T, x, at, e, a.mode, a.out + a.chunk[k] + a.slice[k * TB + threadIdx.x]);
}

__global__ __launch_bounds__(TB) void k_wp_fold_docs(const FoldArgs a) {
    if (!*a.ok) return;
    const W::Text x = text_of(a.x, a.n_dev);
    const int64_t d = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (d > a.n_docs) return;
    const int64_t total = a.chunk[a.n_chunks];
    const int64_t end = a.pad_to >= 0 ? a.pad_to : total;
    if (d == a.n_docs) {
        a.out_offs[d] = end;
        *a.n_out = end;
        return;
    }
    const int64_t o = a.offs[d];
    int64_t at = total;
    if (o < x.n) {
        const int64_t k = o / W::CHUNK_BYTES, s0 = o & ~(int64_t)(W::SLICE_BYTES - 1);
        at = a.chunk[k] + a.slice[k * TB + (s0 - k * W::CHUNK_BYTES) / W::SLICE_BYTES] + W::fold_range(a.T, x, s0, o, a.mode, nullptr);
    }
    a.out_offs[d] = at;
    a.out_flag[at] = 1;
}

struct MatchArgs {
    W::Tables T;
    W::Text x;             // the folded text
    const int64_t* n_dev;
    W::Vocab V;
    uint32_t flags;
    int32_t max_chars, unk;
    int32_t* tmp;          // [cap]: the id workspace
    int64_t n_chunks;
    int64_t* chunk;        // two arrays of [n_chunks + 1]: ids and words per chunk, then their scans
    uint16_t* slice;       // [2][n_chunks * TB]: ids (words) of the chunk in front of the slice
    const int64_t* offs;   // [n_docs + 1] of x
    int64_t n_docs;
    int64_t* out_offs;
    int64_t* word_base;    // [n_docs + 1]: words in front of the document
    int32_t* ids;
    int64_t ids_cap;
    int32_t* word_ids;     // or NULL
    int32_t* err;
    const int32_t* ok;
};

__global__ __launch_bounds__(TB) void k_wp_fill(int32_t* tmp, const int64_t* n_dev, const int32_t* ok) {
    if (!*ok) return;
    const int64_t n = *n_dev;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) tmp[i] = -1;
}

// The word that starts at ws, by the GROUP lanes of one group (all of them run this with the same arguments; gl: the
// lane's place in the group, g0: the group's first lane in the wavefront).  At most max_chars + 1 characters are walked
// and at most max_chars trips made, so a word costs O(max_chars) whatever its length in bytes.
__device__ __forceinline__ void match_word(const MatchArgs& a, const W::Text& x, int64_t ws, int gl, int g0) {
    // the word's end: a space, a character that is a word of its own, a document start, the text's end
    uint32_t cp;
    int len = W::char_at(x, ws, &cp);
    int64_t p = ws + len;
    int chars = 1;
    if (!W::is_alone(W::class_of(W::entry(a.T, cp), a.flags), a.flags)) {
        while (chars <= a.max_chars && p < x.n && !x.flag[p]) {
            len = W::char_at(x, p, &cp);
            const int c = W::class_of(W::entry(a.T, cp), a.flags);
            if (W::is_space(c) || W::is_alone(c, a.flags)) break;
            p += len;
            chars++;
        }
    }
    if (chars > a.max_chars) {
        if (gl == 0) a.tmp[ws] = a.unk | W::ID_START;
        return;
    }
    const int wl = (int)(p - ws);  // at most 4 * max_chars
    const uint8_t* w = x.bytes + ws;
    int s = 0, np = 0;
    while (s < wl) {
        const int kind = s > 0;
        const int top = wl - s < a.V.max_len[kind] ? wl : s + a.V.max_len[kind];
        int hit_end = -1;
        int32_t hit_id = -1;
        for (int base = top; base > s; base -= GROUP) {
            const int e = base - gl;
            int32_t id = -1;
            if (e > s && (e == wl || W::is_char_start(x, ws + e))) id = W::probe(a.V, w + s, e - s, kind);
            const uint32_t m = (uint32_t)(__ballot(id >= 0) >> g0) & ((1u << GROUP) - 1u);
            if (m) {
                const int src = __ffs(m) - 1;  // the lowest lane holds the longest candidate
                hit_end = base - src;
                hit_id = __shfl(id, g0 + src);
                break;
            }
        }
        if (hit_end < 0) {  // the whole word is one unk: what was found so far is taken back
            if (gl == 0) {
                for (int j = 1; j < np; j++) a.tmp[ws + j] = -1;
                a.tmp[ws] = a.unk | W::ID_START;
            }
            return;
        }
        if (gl == 0) a.tmp[ws + np] = hit_id | (np ? 0 : W::ID_START);  // (np < wl: a piece is at least a byte)
        np++;
        s = hit_end;
    }
}

__global__ __launch_bounds__(TB) void k_wp_match(const MatchArgs a) {
    __shared__ int s_part[TB / 64];
    __shared__ uint16_t s_ws[W::CHUNK_BYTES];
    if (!*a.ok) return;
    const W::Text x = text_of(a.x, a.n_dev);
    const int64_t c0 = (int64_t)blockIdx.x * W::CHUNK_BYTES;
    if (c0 >= x.n) return;
    const int tid = threadIdx.x;
    const int64_t at = c0 + (int64_t)tid * W::SLICE_BYTES;
    const int64_t e = at + W::SLICE_BYTES < x.n ? at + W::SLICE_BYTES : x.n;
    uint32_t starts = 0;  // bit i: a word starts at at + i
    for (int64_t p = at; p < e; p++) {
        if (!W::is_char_start(x, p)) continue;
        uint32_t cp;
        (void)W::char_at(x, p, &cp);
        if (W::word_starts(a.T, x, p, W::class_of(W::entry(a.T, cp), a.flags), a.flags)) starts |= 1u << (p - at);
    }
    int n_words;
    int before = hutk::block_excl((int)__popc(starts), s_part, n_words);
    for (uint32_t m = starts; m; m &= m - 1) s_ws[before++] = (uint16_t)(tid * W::SLICE_BYTES + __ffs(m) - 1);
    __syncthreads();
    const int gl = tid & (GROUP - 1), g0 = (tid & 63) & ~(GROUP - 1);
    for (int i = tid / GROUP; i < n_words; i += GROUPS) match_word(a, x, c0 + s_ws[i], gl, g0);
}

__global__ __launch_bounds__(TB) void k_wp_count(const MatchArgs a) {
    __shared__ int s_part[TB / 64];
    if (!*a.ok) return;
    const int64_t n = *a.n_dev;
    const int64_t k = blockIdx.x, c0 = k * W::CHUNK_BYTES;
    if (c0 >= n) return;
    const int64_t at = c0 + (int64_t)threadIdx.x * W::SLICE_BYTES;
    int ids = 0, words = 0;
    for (int64_t p = at; p < at + W::SLICE_BYTES && p < n; p++) {
        const int32_t v = a.tmp[p];
        ids += v >= 0;
        words += v >= 0 && (v & W::ID_START);
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
    const int64_t k = o / W::CHUNK_BYTES, s0 = o & ~(int64_t)(W::SLICE_BYTES - 1);
    int64_t r = chunk[k] + a.slice[(which * a.n_chunks + k) * TB + (s0 - k * W::CHUNK_BYTES) / W::SLICE_BYTES];
    for (int64_t p = s0; p < o; p++) {
        const int32_t v = a.tmp[p];
        r += which ? v >= 0 && (v & W::ID_START) : v >= 0;
    }
    return r;
}

__global__ __launch_bounds__(TB) void k_wp_docs(const MatchArgs a) {
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

__global__ __launch_bounds__(TB) void k_wp_write(const MatchArgs a) {
    if (!*a.ok) return;
    const int64_t n = *a.n_dev;
    const int64_t k = blockIdx.x, c0 = k * W::CHUNK_BYTES;
    if (c0 >= n || a.chunk[a.n_chunks] > a.ids_cap) return;
    const int64_t at = c0 + (int64_t)threadIdx.x * W::SLICE_BYTES;
    int64_t to = a.chunk[k] + a.slice[k * TB + threadIdx.x];
    int64_t word = a.word_ids ? a.chunk[a.n_chunks + 1 + k] + a.slice[(a.n_chunks + k) * TB + threadIdx.x] : 0;
    int64_t d = -1;
    for (int64_t p = at; p < at + W::SLICE_BYTES && p < n; p++) {
        const int32_t v = a.tmp[p];
        if (v < 0) continue;
        a.ids[to] = v & W::ID_MASK;
        if (a.word_ids) {
            word += (v & W::ID_START) != 0;
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

struct hutk_wordpiece {
    int device = 0;
    uint32_t head[W::HEADER_WORDS] = {0};
    int64_t blob_bytes = 0;
    uint32_t flags = 0;
    int32_t max_chars = 100, unk = 0;
    int64_t n_vocab = 0, n_slots = 0;
    std::string prefix;
    hutk_normalizer* nz = nullptr;
    uint32_t nfd_ratio = 1;
    DevBuf<uint8_t> d_blob, d_keys, w_flag[3], w_text[3], s_bytes;
    DevBuf<W::Slot> d_slots;
    DevBuf<int64_t> w_offs[3], w_chunk, w_small, w_word_base, s_offs, s_oo;
    DevBuf<uint16_t> w_slice;
    DevBuf<int32_t> w_tmp, w_ok, s_ids, s_wids;
    W::Tables T{};
    W::Vocab V{};
    std::mutex mu;
    hipEvent_t ev = nullptr;  // behind the last kernel of the last call: calls share the workspace, so they are serialised
    bool ev_recorded = false;
};

extern "C" {

int hutk_debug_wordpiece_chunk_bytes(void) { return W::CHUNK_BYTES; }

void hutk_wordpiece_destroy(hutk_wordpiece* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev) {
        if (h->ev_recorded) (void)hipEventSynchronize(h->ev);  // nothing is freed under a running kernel
        (void)hipEventDestroy(h->ev);
    }
    if (h->nz) hutk_normalizer_destroy(h->nz);
    h->d_blob.release(); h->d_keys.release(); h->s_bytes.release(); h->d_slots.release(); h->w_chunk.release();
    h->w_small.release(); h->w_word_base.release(); h->s_offs.release(); h->s_oo.release(); h->w_slice.release();
    h->w_tmp.release(); h->w_ok.release(); h->s_ids.release(); h->s_wids.release();
    for (int i = 0; i < 3; i++) { h->w_flag[i].release(); h->w_text[i].release(); h->w_offs[i].release(); }
    delete h;
}

int hutk_wordpiece_create(hutk_wordpiece** out, int device, const uint8_t* tables, int64_t n_table_bytes, const uint8_t* norm_blob,
                          int64_t n_norm_bytes, const uint8_t* vocab_bytes, const int64_t* vocab_offsets, int64_t n_vocab,
                          const char* unk_token, const char* prefix, int32_t max_input_chars_per_word, uint32_t flags) {
    if (!out) return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_create: out is NULL");
    *out = nullptr;
    if (!vocab_offsets || n_vocab < 0 || !unk_token || !prefix || (n_vocab > 0 && vocab_offsets[n_vocab] > 0 && !vocab_bytes))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_create: bad arguments");
    if (flags & ~(W::F_CLEAN | W::F_CJK | W::F_STRIP | W::F_LOWER))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_create: flags holds bits that are no HUTK_WP_* flag");
    const std::string pre(prefix), unk(unk_token);
    uint32_t head[W::HEADER_WORDS];
    std::string why;
    if (!W::validate_blob(tables, n_table_bytes, head, &why)) return hutk::api_set_error(HUTK_E_VALUE, "hutk_wordpiece_create: " + why);
    if ((flags & W::F_STRIP) && (!norm_blob || n_norm_bytes <= 0))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_create: HUTK_WP_STRIP_ACCENTS needs the normaliser's table blob");
    W::VocabHost vh;
    if (int bad = W::build_vocab(vocab_bytes, vocab_offsets, n_vocab, unk, pre, max_input_chars_per_word, vh, &why))
        return hutk::api_set_error(bad == 1 ? HUTK_E_VALUE : HUTK_E_ARG, "hutk_wordpiece_create: " + why);
    const std::vector<W::Slot>& table = vh.slots;
    const std::vector<uint8_t>& keys = vh.keys;
    const size_t slots = table.size();
    const int32_t unk_id = vh.unk;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_wordpiece_create: no HIP device");
    if (device < 0) HUTK_HIP_TRY(hipGetDevice(&device));
    if (device >= n) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_wordpiece_create: no such device");
    HUTK_HIP_TRY(hipSetDevice(device));
    hutk_wordpiece* h = new hutk_wordpiece();
    h->device = device;
    h->blob_bytes = n_table_bytes;
    std::memcpy(h->head, head, sizeof(head));
    h->flags = flags, h->max_chars = max_input_chars_per_word, h->unk = unk_id, h->n_vocab = n_vocab, h->n_slots = (int64_t)slots;
    h->prefix = pre;
    if (flags & W::F_STRIP) {
        if (int rc = hutk_normalizer_create(&h->nz, device, norm_blob, n_norm_bytes)) {
            hutk_wordpiece_destroy(h);
            return rc;
        }
        int64_t info[8];
        (void)hutk_normalizer_info(h->nz, info);
        h->nfd_ratio = (uint32_t)((info[7] >> (8 * N::FORM_NFD)) & 0xFF);
    }
    hipError_t e = h->d_blob.reserve((size_t)n_table_bytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_blob.p, tables, (size_t)n_table_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->d_slots.reserve(slots);
    if (e == hipSuccess) e = hipMemcpy(h->d_slots.p, table.data(), slots * sizeof(W::Slot), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->d_keys.reserve(keys.size() + 16);
    if (e == hipSuccess && !keys.empty()) e = hipMemcpy(h->d_keys.p, keys.data(), keys.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->w_ok.reserve(2);
    if (e == hipSuccess) e = h->w_small.reserve(8);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        hutk_wordpiece_destroy(h);
        return hutk::api_set_error(e == hipErrorOutOfMemory ? HUTK_E_MEMORY : HUTK_E_DEVICE,
                                   std::string("hutk_wordpiece_create: ") + hipGetErrorString(e));
    }
    h->T = W::tables_of(h->d_blob.p, h->head);
    h->V = vh.view(h->d_slots.p, h->d_keys.p);
    *out = h;
    return HUTK_OK;
}

int hutk_wordpiece_info(const hutk_wordpiece* h, int64_t* out8) {
    if (!h || !out8) return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_info: bad arguments");
    out8[0] = h->head[W::H_VERSION];
    out8[1] = h->head[W::H_UNIDATA];
    out8[2] = h->blob_bytes;
    out8[3] = W::CHUNK_BYTES;
    out8[4] = h->n_vocab;
    out8[5] = h->n_slots;
    out8[6] = h->flags;
    out8[7] = h->unk;
    return HUTK_OK;
}

int64_t hutk_debug_wordpiece_bucket(const hutk_wordpiece* h, const uint8_t* bytes, int64_t len, int continuation) {
    if (!h || len < 0 || len > INT32_MAX || (len > 0 && !bytes)) return -1;
    return (int64_t)(W::piece_hash(bytes, (int)len, continuation ? 1 : 0) & (uint32_t)(h->n_slots - 1));
}

static int64_t wp_setting(const hutk_wordpiece* h) { return ((h->flags & W::F_LOWER) ? 1 : 0) | ((h->flags & W::F_STRIP) ? 2 : 0); }

/* An id is at least one character of the folded text, and the header holds the most characters a byte can become. */
int64_t hutk_wordpiece_ids_capacity(const hutk_wordpiece* h, int64_t n_bytes, int64_t n_docs) {
    (void)n_docs;
    if (!h || n_bytes < 0) return -1;
    return n_bytes * (int64_t)h->head[W::H_CHAR_RATIO + wp_setting(h)];
}

int hutk_wordpiece_encode_batch_device(hutk_wordpiece* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                       int64_t n_bytes, int32_t* d_ids, int64_t ids_cap, int64_t* d_out_offsets,
                                       int32_t* d_word_ids, int32_t* d_err, void* hip_stream) {
    if (!h) return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_encode_batch_device: the handle is NULL");
    if (n_docs < 0 || n_bytes < 0 || ids_cap < 0 || !d_offsets || !d_out_offsets || (n_bytes > 0 && !d_bytes) || (ids_cap > 0 && !d_ids))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_encode_batch_device: bad arguments");
    const bool strip = (h->flags & W::F_STRIP) != 0, clean = (h->flags & W::F_CLEAN) != 0, lower = (h->flags & W::F_LOWER) != 0;
    // the sizes the host can bound: the text in front of NFD keeps n_bytes, NFD's and the fold's grow by the tables' ratios
    const int64_t cap_nfd = strip ? n_bytes * (int64_t)h->nfd_ratio : 0;
    const int64_t cap_f = (n_bytes * (int64_t)h->head[W::H_BYTE_RATIO16 + wp_setting(h)] + 15) / 16;
    const int64_t cap_max = std::max(std::max(cap_nfd, cap_f), n_bytes);
    const int64_t chunks_max = (cap_max + W::CHUNK_BYTES - 1) / W::CHUNK_BYTES;
    if (chunks_max > INT32_MAX / 2 || (n_docs + TB) / TB > INT32_MAX)
        return hutk::api_set_error(HUTK_E_UNSUPPORTED, "hutk_wordpiece_encode_batch_device: the batch is too large for one launch");
    std::lock_guard<std::mutex> lock(h->mu);
    HUTK_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(h->w_flag[0].reserve((size_t)n_bytes + 1));
    for (int i = 1; i < 3; i++) {  // the two texts that take turns: either may hold any stage
        HUTK_HIP_TRY(h->w_flag[i].reserve((size_t)cap_max + 1));
        HUTK_HIP_TRY(h->w_text[i].reserve((size_t)cap_max + 16));
        HUTK_HIP_TRY(h->w_offs[i].reserve((size_t)n_docs + 1));
    }
    HUTK_HIP_TRY(h->w_chunk.reserve(2 * ((size_t)chunks_max + 1)));
    HUTK_HIP_TRY(h->w_slice.reserve(2 * (size_t)chunks_max * TB + 1));
    HUTK_HIP_TRY(h->w_tmp.reserve((size_t)cap_f + 1));
    if (d_word_ids) HUTK_HIP_TRY(h->w_word_base.reserve((size_t)n_docs + 1));
    if (h->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
    int32_t* ok = h->w_ok.p;
    int32_t* err = d_err ? d_err : h->w_ok.p + 1;
    HUTK_HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), st));
    HUTK_HIP_TRY(hipMemsetAsync(ok, 1, sizeof(int32_t), st));  // (bytes of 1: any value but 0 says "sound")
    hipLaunchKernelGGL(k_wp_check, dim3(blocks_for(n_docs)), dim3(TB), 0, st, d_offsets, n_docs, n_bytes, ok, err);
    HUTK_HIP_TRY(hipMemsetAsync(h->w_flag[0].p, 0, (size_t)n_bytes + 1, st));
    hipLaunchKernelGGL(k_wp_flags, dim3(blocks_for(n_docs)), dim3(TB), 0, st, d_offsets, n_docs, h->w_flag[0].p, ok);

    // the text as it stands: where it is, its flags and offsets, its size on the host (a bound when n_dev is set)
    W::Text cur{d_bytes, h->w_flag[0].p, n_bytes};
    const int64_t* cur_offs = d_offsets;
    const int64_t* cur_n = nullptr;
    int64_t cur_cap = n_bytes;
    int64_t* sizes = h->w_small.p;  // [0], [1]: the sizes of the two fold outputs; [2], [3]: the normaliser's totals
    int next = 1;
    auto fold = [&](uint32_t mode, int64_t cap_out, int64_t pad_to, int64_t* n_out) -> int {
        FoldArgs a;
        a.T = h->T, a.x = cur, a.n_dev = cur_n, a.mode = mode;
        a.n_chunks = (cur_cap + W::CHUNK_BYTES - 1) / W::CHUNK_BYTES;
        a.chunk = h->w_chunk.p, a.slice = h->w_slice.p;
        a.out = h->w_text[next].p, a.out_flag = h->w_flag[next].p;
        a.offs = cur_offs, a.out_offs = h->w_offs[next].p, a.n_docs = n_docs, a.n_out = n_out, a.pad_to = pad_to, a.ok = ok;
        HUTK_HIP_TRY(hipMemsetAsync(a.chunk, 0, ((size_t)a.n_chunks + 1) * sizeof(int64_t), st));
        HUTK_HIP_TRY(hipMemsetAsync(a.out_flag, 0, (size_t)cap_out + 1, st));
        if (a.n_chunks) hipLaunchKernelGGL(k_wp_fold_count, dim3((unsigned)a.n_chunks), dim3(TB), 0, st, a);
        hipLaunchKernelGGL(k_wp_scan, dim3(1), dim3(SCAN_TB), 0, st, a.chunk, (int64_t)0, a.n_chunks, ok);
        if (a.n_chunks) hipLaunchKernelGGL(k_wp_fold_write, dim3((unsigned)a.n_chunks), dim3(TB), 0, st, a);
        hipLaunchKernelGGL(k_wp_fold_docs, dim3(blocks_for(n_docs)), dim3(TB), 0, st, a);
        HUTK_HIP_TRY(hipGetLastError());
        cur = W::Text{a.out, a.out_flag, cap_out};
        cur_offs = a.out_offs, cur_n = n_out, cur_cap = cap_out;
        next = 3 - next;
        return HUTK_OK;
    };
    if (strip) {
        if (clean) {  // the result keeps n_bytes bytes (padded), so the normaliser's host-side size holds
            if (int rc = fold(W::M_CLEAN, n_bytes, n_bytes, sizes)) return rc;
            cur.n = n_bytes, cur_n = nullptr;
        }
        // NFD through the normaliser: its sizes call, then its write call, on the same stream
        uint8_t* nfd = h->w_text[next].p;
        int64_t* nfd_offs = h->w_offs[next].p;
        if (int rc = hutk_normalize_batch_device(h->nz, N::FORM_NFD, cur.bytes, cur_offs, n_docs, n_bytes, nullptr, 0, nfd_offs, nullptr,
                                                 sizes + 2, nullptr, st))
            return rc;
        if (int rc = hutk_normalize_batch_device(h->nz, N::FORM_NFD, cur.bytes, cur_offs, n_docs, n_bytes, nfd, cap_nfd, nullptr, nullptr,
                                                 nullptr, nullptr, st))
            return rc;
        HUTK_HIP_TRY(hipMemsetAsync(h->w_flag[next].p, 0, (size_t)cap_nfd + 1, st));
        hipLaunchKernelGGL(k_wp_flags, dim3(blocks_for(n_docs)), dim3(TB), 0, st, nfd_offs, n_docs, h->w_flag[next].p, ok);
        cur = W::Text{nfd, h->w_flag[next].p, cap_nfd};
        cur_offs = nfd_offs, cur_n = sizes + 2, cur_cap = cap_nfd;
        next = 3 - next;
        if (int rc = fold(W::M_MARKS | (lower ? W::M_LOWER : 0u), cap_f, -1, sizes + 1)) return rc;
    } else {
        if (int rc = fold((clean ? W::M_CLEAN : 0u) | (lower ? W::M_LOWER : 0u), cap_f, -1, sizes + 1)) return rc;
    }

    MatchArgs m;
    m.T = h->T, m.x = cur, m.n_dev = cur_n, m.V = h->V, m.flags = h->flags, m.max_chars = h->max_chars, m.unk = h->unk;
    m.tmp = h->w_tmp.p;
    m.n_chunks = (cap_f + W::CHUNK_BYTES - 1) / W::CHUNK_BYTES;
    m.chunk = h->w_chunk.p, m.slice = h->w_slice.p;
    m.offs = cur_offs, m.n_docs = n_docs, m.out_offs = d_out_offsets, m.word_base = h->w_word_base.p;
    m.ids = d_ids, m.ids_cap = ids_cap, m.word_ids = d_word_ids, m.err = err, m.ok = ok;
    HUTK_HIP_TRY(hipMemsetAsync(m.chunk, 0, 2 * ((size_t)m.n_chunks + 1) * sizeof(int64_t), st));
    if (m.n_chunks) {
        const unsigned fill = (unsigned)std::min<int64_t>((cap_f + TB - 1) / TB, 1 << 16);
        hipLaunchKernelGGL(k_wp_fill, dim3(fill), dim3(TB), 0, st, m.tmp, cur_n, ok);
        hipLaunchKernelGGL(k_wp_match, dim3((unsigned)m.n_chunks), dim3(TB), 0, st, m);
        hipLaunchKernelGGL(k_wp_count, dim3((unsigned)m.n_chunks), dim3(TB), 0, st, m);
    }
    hipLaunchKernelGGL(k_wp_scan, dim3(2), dim3(SCAN_TB), 0, st, m.chunk, m.n_chunks + 1, m.n_chunks, ok);
    hipLaunchKernelGGL(k_wp_docs, dim3(blocks_for(n_docs)), dim3(TB), 0, st, m);
    if (m.n_chunks) hipLaunchKernelGGL(k_wp_write, dim3((unsigned)m.n_chunks), dim3(TB), 0, st, m);
    HUTK_HIP_TRY(hipGetLastError());
    HUTK_HIP_TRY(hipEventRecord(h->ev, st));
    h->ev_recorded = true;
    return HUTK_OK;
}

int hutk_wordpiece_encode_batch(hutk_wordpiece* h, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, int32_t** out_ids,
                                int64_t** out_offsets, int32_t** out_word_ids) {
    if (!h || !out_ids || !out_offsets || n_docs < 0 || !offsets) return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_encode_batch: bad arguments");
    *out_ids = nullptr;
    *out_offsets = nullptr;
    if (out_word_ids) *out_word_ids = nullptr;
    if (int rc = hutk::check_offsets(offsets, n_docs, true, "offsets")) return rc;
    const int64_t n_bytes = offsets[n_docs];
    if (n_bytes > 0 && !bytes) return hutk::api_set_error(HUTK_E_ARG, "hutk_wordpiece_encode_batch: bytes is NULL");
    const int64_t cap = hutk_wordpiece_ids_capacity(h, n_bytes, n_docs);
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
    if (int rc = hutk_wordpiece_encode_batch_device(h, h->s_bytes.p, h->s_offs.p, n_docs, n_bytes, h->s_ids.p, cap, h->s_oo.p,
                                                    out_word_ids ? h->s_wids.p : nullptr, nullptr, nullptr))
        return rc;
    HUTK_HIP_TRY(hipStreamSynchronize(nullptr));
    int32_t err = 0;
    HUTK_HIP_TRY(hipMemcpy(&err, h->w_ok.p + 1, 4, hipMemcpyDeviceToHost));
    if (err) return hutk::api_set_error(err, "hutk_wordpiece_encode_batch: device-side failure");
    int64_t* oo = (int64_t*)hutk_host_alloc((size_t)(n_docs + 1) * 8);
    if (!oo) return hutk::api_set_error(HUTK_E_MEMORY, "hutk_wordpiece_encode_batch: out of host memory");
    hipError_t e = hipMemcpy(oo, h->s_oo.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost);
    const int64_t total = e == hipSuccess ? oo[n_docs] : 0;
    int32_t* ids = (int32_t*)hutk_host_alloc((size_t)(total > 0 ? total : 1) * 4);
    int32_t* wids = out_word_ids ? (int32_t*)hutk_host_alloc((size_t)(total > 0 ? total : 1) * 4) : nullptr;
    if (e == hipSuccess && (!ids || (out_word_ids && !wids))) {
        hutk_host_free(oo);
        if (ids) hutk_host_free(ids);
        if (wids) hutk_host_free(wids);
        return hutk::api_set_error(HUTK_E_MEMORY, "hutk_wordpiece_encode_batch: out of host memory");
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
