// hutk_special.hip -- special tokens: byte strings of the text that encode as ONE id each, matched on the device
// (include/hutoken_amd.h).  The matches (leftmost first, then longest, never overlapping, never
// across two documents) cut every document into pieces: text, special, text, ..., text.  The pieces are encoded by the
// encode direction as documents of their own (hutk_api.cpp, encode_device_impl: none of its kernels knows of this
// file) and put together again with the special ids in the places of the special pieces.
//
//   k_sc_find     ONE pass over the text, 16 bytes a lane: mlen[p] = length of the longest special string at p, 0: none.
//                 Almost every 16 bytes leave after a word-wise compare with the (at most four) first bytes of the set;
//                 a position whose byte is in the first-byte set and whose next byte is in the second-byte set is
//                 hashed forwards (FNV-1a, a byte at a time) and looked up at every length the set has: the cost per
//                 candidate grows with the longest string and the number of distinct LENGTHS, not with the set.
//   k_sc_resolve  a candidate no earlier candidate reaches over is a chain head; its lane walks the chain greedily
//                 (take, jump to the end, the next candidate at or after it) until nothing reaches further: sel[p] = 1
//   k_sc_count    selected matches per tile;  k_scan_i64: exclusive scan (one workgroup)     -- then the host reads the
//   k_sc_write    match k in text order: m_start[k], and the piece offsets and the id of ITS pieces     number of matches
//   k_sc_docs     document i: first_piece[i] = i + 2 x (matches in front of it), piece_off[first_piece[i]] = offsets[i]
//   -- the pieces are encoded --
//   k_st_sum / k_scan_i64 / k_st_dst   ids every piece keeps (a special piece: one) and their exclusive scan
//   k_st_docs     out_offsets and the documents' status (the worst of their pieces)
//   k_st_copy     ragged to ragged: a workgroup finds the pieces of its 2048 output ids by search, a lane walks on
//                 from there; 16-byte stores
// No workgroup waits for another one: every order is count, scan, write over three launches.
//
// The other direction, ids -> text with special ids among them (hutk_decode_special_batch_device), needs ONE kernel here:
//   k_dsp_remap   a pass over the ids in front of the decode kernels of hutk_decode.hip, which then run unchanged over
//                 tables that hutk_ctx_set_special_tokens extended by the special strings (build_decode_specials)
//
// The C entry points are at the end of the file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <set>
#include <string>

#include "hutk_host.h"
#include "hutk_wave.h"

namespace hutk {

namespace {

constexpr int SC_THREADS = 256, SC_PER = 16, SC_TILE = SC_THREADS * SC_PER;  // bytes per workgroup of the scan
constexpr int ST_THREADS = 256, ST_PER = 4, ST_BLOCK = ST_THREADS * ST_PER;  // pieces per workgroup of the stitch scan
constexpr int CP_THREADS = 256, CP_PER = 8, CP_TILE = CP_THREADS * CP_PER;   // output ids per workgroup of the copy
constexpr uint32_t SLOT_NONE = 0xFFFFFFFFu;
constexpr uint32_t FNV_BASIS = 2166136261u;
constexpr int MAX_SPECIALS = 1024, MAX_SPECIAL_BYTES = 255;

// the same on the host (table build) and on the device (lookup)
HUTK_HD uint32_t sc_step(uint32_t h, uint32_t b) { return (h ^ b) * 16777619u; }
HUTK_HD uint32_t sc_slot(uint32_t h, uint32_t len) {
    uint32_t x = h ^ (len * 0x9E3779B1u);
    x ^= x >> 15;
    x *= 0x85EBCA6Bu;
    return x ^ (x >> 13);
}

struct SpecTab {
    const uint2* slots;    // [mask + 1] {hash, index | length << 16}, y == SLOT_NONE: empty; linear probing
    const uint8_t* blob;
    const uint32_t* off;   // [n + 1]
    const int32_t* ids;    // [n]
    const uint32_t* filt;  // [24] first bytes, second bytes (all ones when a one-byte string exists), lengths
    uint32_t mask, max_len, n_first;  // n_first: distinct first bytes when there are at most four, else 0
    uint32_t first[4];                // ... each in all four bytes of a word
};

struct SpecArgs {
    const uint8_t* bytes;
    const int64_t* offs;
    int64_t n_docs, n_bytes, n_tiles;
    uint8_t* mlen;         // [n_bytes] longest special string at the position
    uint8_t* sel;          // [n_bytes] 1: the match at the position is taken
    int64_t* tile_base;    // [n_tiles + 1] taken matches per tile, then in front of it
    int64_t* m_start;      // [n_matches]
    int64_t n_matches, n_pieces;
    int64_t* piece_off;      // [n_pieces + 1]
    int32_t* piece_special;  // [n_pieces] the id of a special piece, -1 for a text piece
    int64_t* first_piece;    // [n_docs + 1]
    const int64_t* piece_oo;      // [n_pieces + 1] what the encode wrote for the pieces
    const int32_t* piece_status;  // [n_pieces]
    const int32_t* piece_ids;
    int64_t* blk;          // [pieces / ST_BLOCK + 1]
    int64_t* dst;          // [n_pieces + 1] first output id of every piece
    int32_t* out_ids;
    int64_t ids_cap;
    int64_t* out_offsets;
    int32_t* status;
    int32_t* err;
};

__device__ __forceinline__ void sc_raise(int32_t* err, int32_t code) { atomicCAS(err, 0, code); }
__device__ __forceinline__ bool in_set(const uint32_t* set, uint32_t b) { return (set[b >> 5] >> (b & 31)) & 1u; }

// 16 bytes of a byte array at pos (a multiple of 16; the array is 16-byte aligned) as four words, zeros beyond n
__device__ __forceinline__ uint4 load16(const uint8_t* a, int64_t pos, int64_t n) {
    if (pos + 16 <= n) return *reinterpret_cast<const uint4*>(a + pos);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (pos + 4 * j + b < n) w[j] |= (uint32_t)a[pos + 4 * j + b] << (8 * b);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the smallest i in [1, n_docs] with offs[i] > p (n_docs when there is none): document i - 1 holds byte p
__device__ __forceinline__ int64_t sc_doc_after(const int64_t* offs, int64_t n_docs, int64_t p) {
    int64_t lo = 1, hi = n_docs;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (offs[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the index of the special string that equals text[0, len) and whose hash is h; -1: none
__device__ __forceinline__ int sc_lookup(const SpecTab& T, const uint8_t* text, uint32_t h, uint32_t len) {
    uint32_t s = sc_slot(h, len) & T.mask;
    for (uint32_t i = 0; i <= T.mask; i++, s = (s + 1) & T.mask) {
        const uint2 e = T.slots[s];
        if (e.y == SLOT_NONE) return -1;
        if (e.x != h || (e.y >> 16) != len) continue;
        const uint8_t* want = T.blob + T.off[e.y & 0xFFFFu];
        uint32_t j = 0;
        while (j < len && want[j] == text[j]) j++;
        if (j == len) return (int)(e.y & 0xFFFFu);
    }
    return -1;
}

// the longest special string at byte p (its first byte is in the first-byte set) that ends inside p's document
__device__ __forceinline__ uint32_t sc_match(const SpecTab& T, const SpecArgs& A, const uint32_t* s_filt, int64_t p) {
    int64_t end = A.offs[sc_doc_after(A.offs, A.n_docs, p)];
    if (end > A.n_bytes) end = A.n_bytes;  // (offsets that do not describe the buffer: nothing beyond it is read)
    if (end <= p) return 0;
    const uint32_t limit = end - p < (int64_t)T.max_len ? (uint32_t)(end - p) : T.max_len;
    const uint8_t* text = A.bytes + p;
    if (limit >= 2 && !in_set(s_filt + 8, text[1])) return 0;
    uint32_t h = FNV_BASIS, best = 0;
    for (uint32_t k = 1; k <= limit; k++) {
        h = sc_step(h, text[k - 1]);
        if (in_set(s_filt + 16, k) && sc_lookup(T, text, h, k) >= 0) best = k;
    }
    return best;
}

// ---- find ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void k_sc_find(SpecTab T, SpecArgs A) {
    __shared__ uint32_t s_filt[24];
    const int tid = threadIdx.x;
    if (tid < 24) s_filt[tid] = T.filt[tid];
    __syncthreads();
    const int64_t pos = (int64_t)blockIdx.x * SC_TILE + (int64_t)tid * SC_PER;
    if (pos >= A.n_bytes) return;
    const uint4 v = load16(A.bytes, pos, A.n_bytes);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};  // (only ever indexed by unrolled loops)
    bool any = T.n_first == 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if ((uint32_t)k < T.n_first) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t x = w[j] ^ T.first[k];
                any = any || ((x - 0x01010101u) & ~x & 0x80808080u) != 0;  // a zero byte: a first byte of the set
            }
        }
    // (the sixteen positions in a loop that is NOT unrolled: sixteen copies of the candidate's path would be code nobody
    // runs; the bytes leave the two words at the bottom, the lengths enter at the top)
    uint64_t lo = v.x | (uint64_t)v.y << 32, hi = v.z | (uint64_t)v.w << 32, out_lo = 0, out_hi = 0;
    if (any) {
#pragma unroll 1
        for (int i = 0; i < SC_PER; i++) {
            const uint32_t c = (uint32_t)lo & 0xFFu;
            lo = lo >> 8 | hi << 56;
            hi >>= 8;
            const int64_t p = pos + i;
            uint64_t m = 0;
            if (p < A.n_bytes && in_set(s_filt, c)) m = sc_match(T, A, s_filt, p);
            out_lo = out_lo >> 8 | out_hi << 56;
            out_hi = out_hi >> 8 | m << 56;
        }
    }
    if (pos + 16 <= A.n_bytes) {
        *reinterpret_cast<uint4*>(A.mlen + pos) =
            make_uint4((uint32_t)out_lo, (uint32_t)(out_lo >> 32), (uint32_t)out_hi, (uint32_t)(out_hi >> 32));
    } else {
        for (int i = 0; i < SC_PER && pos + i < A.n_bytes; i++) {
            A.mlen[pos + i] = (uint8_t)out_lo;
            out_lo = out_lo >> 8 | out_hi << 56;
            out_hi >>= 8;
        }
    }
}

// ---- resolve -------------------------------------------------------------------------------------------------------
// Candidate p is a chain head when no candidate q < p has q + mlen[q] > p (such a q lies within max_len - 1 bytes).  The
// left-to-right scan of the contract arrives at every head with its cursor at or in front of it, so a head is taken;
// behind it the scan is: take, cursor = end, the next candidate at or behind the cursor.  The walk ends where no
// candidate seen since the head reaches any further: a candidate there is the next head (its own lane's).
__global__ __launch_bounds__(SC_THREADS) void k_sc_resolve(SpecArgs A, uint32_t max_len) {
    const int64_t pos = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_PER;
    if (pos >= A.n_bytes) return;
    const uint4 v = load16(A.mlen, pos, A.n_bytes);
    if ((v.x | v.y | v.z | v.w) == 0) return;
    uint64_t w_lo = v.x | (uint64_t)v.y << 32, w_hi = v.z | (uint64_t)v.w << 32;
#pragma unroll 1
    for (int i = 0; i < SC_PER; i++) {
        {
            const uint32_t m = (uint32_t)w_lo & 0xFFu;
            w_lo = w_lo >> 8 | w_hi << 56;
            w_hi >>= 8;
            if (m == 0) continue;
            const int64_t p = pos + i;
            const int64_t lo = p - (int64_t)(max_len - 1) > 0 ? p - (int64_t)(max_len - 1) : 0;
            bool head = true;
            for (int64_t q = p - 1; q >= lo && head; q--) head = (int64_t)A.mlen[q] <= p - q;
            if (!head) continue;
            A.sel[p] = 1;
            int64_t cur = p + m, reach = p + m;  // (reach <= the end of the document <= n_bytes: mlen ends inside it)
            for (int64_t s = p + 1; s < reach; s++) {
                const int64_t ms = A.mlen[s];
                if (ms == 0) continue;
                if (s + ms > reach) reach = s + ms;
                if (s >= cur) {
                    A.sel[s] = 1;
                    cur = s + ms;
                }
            }
        }
    }
}

// ---- compact and cut -----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sel_count(uint4 v) { return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }

__global__ __launch_bounds__(SC_THREADS) void k_sc_count(SpecArgs A) {
    __shared__ uint32_t s_part[4];
    const int64_t pos = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_PER;
    uint32_t n = 0;
    if (pos < A.n_bytes) n = sel_count(load16(A.sel, pos, A.n_bytes));
    uint32_t total;
    (void)block_excl(n, s_part, total);
    if (threadIdx.x == 0) A.tile_base[blockIdx.x] = total;
}

// a[0, n) becomes its exclusive scan, a[n] the sum.  One workgroup.
__global__ __launch_bounds__(1024) void k_scan_i64(int64_t* a, int64_t n) {
    __shared__ int64_t s_part[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    for (int64_t at = 0; at < n; at += 1024) {
        const int64_t i = at + tid;
        const int64_t v = i < n ? a[i] : 0;
        const int64_t incl = wave_incl(v, lane);
        if (lane == 63) s_part[w] = incl;
        __syncthreads();
        int64_t before = 0, total = 0;
        for (int u = 0; u < 16; u++) {
            if (u < w) before += s_part[u];
            total += s_part[u];
        }
        if (i < n) a[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) a[n] = carry;
}

// Match k (in text order) of document d is piece d + 2k + 1; the text behind it is piece d + 2k + 2.
__global__ __launch_bounds__(SC_THREADS) void k_sc_write(SpecTab T, SpecArgs A) {
    __shared__ uint32_t s_part[4];
    const int64_t pos = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_PER;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (pos < A.n_bytes) v = load16(A.sel, pos, A.n_bytes);
    uint32_t total;
    const uint32_t before = block_excl(sel_count(v), s_part, total);
    if ((v.x | v.y | v.z | v.w) == 0) return;
    int64_t k = A.tile_base[blockIdx.x] + before;
    uint64_t w_lo = v.x | (uint64_t)v.y << 32, w_hi = v.z | (uint64_t)v.w << 32;
#pragma unroll 1
    for (int i = 0; i < SC_PER; i++) {
        {
            const bool taken = (w_lo & 0xFFu) != 0;
            w_lo = w_lo >> 8 | w_hi << 56;
            w_hi >>= 8;
            if (!taken) continue;
            const int64_t p = pos + i;
            const uint32_t len = A.mlen[p];
            const uint8_t* text = A.bytes + p;
            uint32_t h = FNV_BASIS;
            for (uint32_t i = 0; i < len; i++) h = sc_step(h, text[i]);
            const int idx = sc_lookup(T, text, h, len);
            if (idx < 0 || k >= A.n_matches) {  // (cannot happen: k_sc_find found it, the host read the count)
                sc_raise(A.err, HUTK_E_DEVICE);
                continue;
            }
            const int64_t d = sc_doc_after(A.offs, A.n_docs, p) - 1;
            A.m_start[k] = p;
            A.piece_off[d + 2 * k + 1] = p;
            A.piece_off[d + 2 * k + 2] = p + len;
            A.piece_special[d + 2 * k + 1] = T.ids[idx];
            k++;
        }
    }
}

__global__ void k_sc_docs(SpecArgs A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > A.n_docs) return;
    const int64_t o = A.offs[i];
    int64_t lo = 0, hi = A.n_matches;  // matches that start in front of offsets[i]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.m_start[mid] < o) lo = mid + 1; else hi = mid;
    }
    A.first_piece[i] = i + 2 * lo;
    A.piece_off[i + 2 * lo] = o;
}

// ---- stitch --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t st_kept(const SpecArgs& A, int64_t j) {
    return A.piece_special[j] >= 0 ? 1 : A.piece_oo[j + 1] - A.piece_oo[j];
}

__global__ __launch_bounds__(ST_THREADS) void k_st_sum(SpecArgs A) {
    __shared__ int64_t s_part[4];
    const int64_t j0 = (int64_t)blockIdx.x * ST_BLOCK + (int64_t)threadIdx.x * ST_PER;
    int64_t n = 0;
#pragma unroll
    for (int k = 0; k < ST_PER; k++)
        if (j0 + k < A.n_pieces) n += st_kept(A, j0 + k);
    int64_t total;
    (void)block_excl(n, s_part, total);
    if (threadIdx.x == 0) A.blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(ST_THREADS) void k_st_dst(SpecArgs A, int64_t n_blocks) {
    __shared__ int64_t s_part[4];
    const int64_t j0 = (int64_t)blockIdx.x * ST_BLOCK + (int64_t)threadIdx.x * ST_PER;
    int64_t kept[ST_PER], n = 0;
#pragma unroll
    for (int k = 0; k < ST_PER; k++) {
        kept[k] = j0 + k < A.n_pieces ? st_kept(A, j0 + k) : 0;
        n += kept[k];
    }
    int64_t total;
    int64_t at = A.blk[blockIdx.x] + block_excl(n, s_part, total);
#pragma unroll
    for (int k = 0; k < ST_PER; k++) {
        if (j0 + k < A.n_pieces) A.dst[j0 + k] = at;
        at += kept[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) A.dst[A.n_pieces] = A.blk[n_blocks];
}

__global__ void k_st_docs(SpecArgs A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > A.n_docs) return;
    const int64_t j0 = A.first_piece[i];
    A.out_offsets[i] = A.dst[j0];
    if (i == A.n_docs || !A.status) return;
    int32_t worst = 0;
    for (int64_t j = j0, j1 = A.first_piece[i + 1]; j < j1; j++) {
        const int32_t s = A.piece_status[j];
        worst = s > worst ? s : worst;
    }
    A.status[i] = worst;
}

// the largest j in [lo, hi] with dst[j] <= o (dst[lo] <= o)
__device__ __forceinline__ int64_t st_piece_of(const int64_t* dst, int64_t lo, int64_t hi, int64_t o) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (dst[mid] <= o) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(CP_THREADS) void k_st_copy(SpecArgs A) {
    __shared__ int64_t s_j[2];
    const int64_t total = A.dst[A.n_pieces];
    const int64_t o0 = (int64_t)blockIdx.x * CP_TILE;
    if (o0 >= total) return;
    const int64_t o1 = o0 + CP_TILE < total ? o0 + CP_TILE : total;
    const int tid = threadIdx.x;
    if (tid < 2) s_j[tid] = st_piece_of(A.dst, 0, A.n_pieces - 1, tid == 0 ? o0 : o1 - 1);
    __syncthreads();
    if (total > A.ids_cap) {  // (cannot happen: hutk_special_ids_capacity is a bound and the call checked ids_cap)
        if (tid == 0) sc_raise(A.err, HUTK_E_CAPACITY);
        return;
    }
    const int64_t j_lo = s_j[0], j_hi = s_j[1];
    const bool aligned = (reinterpret_cast<uintptr_t>(A.out_ids) & 15) == 0;
#pragma unroll
    for (int g = 0; g < CP_PER / 4; g++) {
        const int64_t o = o0 + (int64_t)tid * CP_PER + g * 4;
        if (o >= o1) break;
        int64_t j = st_piece_of(A.dst, j_lo, j_hi, o);
        int64_t next = A.dst[j + 1], src = A.piece_oo[j] - A.dst[j];
        int32_t sp = A.piece_special[j];
        int32_t val[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t oo = o + k;
            if (oo >= o1) break;
            while (next <= oo) {  // (oo < total = dst[n_pieces]: the walk ends at a piece that holds oo)
                j++;
                next = A.dst[j + 1];
                src = A.piece_oo[j] - A.dst[j];
                sp = A.piece_special[j];
            }
            val[k] = sp >= 0 ? sp : A.piece_ids[src + oo];
        }
        if (aligned && o + 4 <= o1) {
            *reinterpret_cast<int4*>(A.out_ids + o) = make_int4(val[0], val[1], val[2], val[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (o + k < o1) A.out_ids[o + k] = val[k];
        }
    }
}

// ---- decode: special ids become entries behind the vocabulary's ----------------------------------------------------
constexpr int DSP_THREADS = 256, DSP_PER = 4, DSP_TILE = DSP_THREADS * DSP_PER;  // ids per workgroup of the pass

// (dsp_slot, dsp_index, dsp_bit: hutk_device.h -- the byte-fallback decode's pass uses them too)

// out[i] = ids[i] for a vocabulary id, n_vocab + k for the k-th special id, -1 for anything else (an id in
// [n_vocab, n_vocab + specials) that is not special must NOT reach the extended tables).  first_bits (a context that
// strips a prefix; k_dec_mark has run) gets the bits the contract adds:
//   DSP_BITS_AFTER  every run of ordinary ids is a document of its own: bit i + 1 behind a special at i
//   DSP_BITS_SKIP   the specials are deleted: the lane of a document's first token, when that is special, walks to the
//                   first id that is not and marks it.  A special never GETS a bit from this pass (a walk ends on an
//                   ordinary id or on a bit that is set), so a special with a bit is a document's first token; the walk
//                   stops at the next such token, whose own lane goes on from there: every id is walked over once.
__global__ __launch_bounds__(DSP_THREADS) void k_dsp_remap(DecSpecial S, const int32_t* ids, int32_t* out, int64_t n_ids,
                                                           uint32_t* first_bits) {
    const int64_t i0 = ((int64_t)blockIdx.x * DSP_THREADS + threadIdx.x) * DSP_PER;
    if (i0 >= n_ids) return;
    const bool full = i0 + DSP_PER <= n_ids;
    int32_t id[DSP_PER];
    if (full && (reinterpret_cast<uintptr_t>(ids) & 15) == 0) {
        const int4 a = *reinterpret_cast<const int4*>(ids + i0);
        id[0] = a.x; id[1] = a.y; id[2] = a.z; id[3] = a.w;
    } else {
#pragma unroll
        for (int k = 0; k < DSP_PER; k++) id[k] = (i0 + k < n_ids) ? ids[i0 + k] : 0;
    }
    int32_t v[DSP_PER];
#pragma unroll
    for (int k = 0; k < DSP_PER; k++) {
        const int64_t i = i0 + k;
        v[k] = id[k] >= S.n_vocab ? -1 : id[k];
        if (i >= n_ids) continue;
        const int32_t x = dsp_index(S, id[k]);
        if (x < 0) continue;
        v[k] = S.n_vocab + x;
        if (S.bits == DSP_BITS_AFTER) {
            if (i + 1 < n_ids) atomicOr(&first_bits[(i + 1) >> 5], 1u << ((i + 1) & 31));
        } else if (S.bits == DSP_BITS_SKIP && dsp_bit(first_bits, i)) {
            int64_t j = i + 1;
            while (j < n_ids && !dsp_bit(first_bits, j) && dsp_index(S, ids[j]) >= 0) j++;
            if (j < n_ids) atomicOr(&first_bits[j >> 5], 1u << (j & 31));
        }
    }
    if (full) {  // (out is the context's: 16-byte aligned)
        *reinterpret_cast<int4*>(out + i0) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < DSP_PER; k++)
            if (i0 + k < n_ids) out[i0 + k] = v[k];
    }
}

// ---- host: the set -------------------------------------------------------------------------------------------------
int build_specials(hutk_ctx::Specials& S, const uint8_t* bytes, const int64_t* offsets, const int32_t* ids, int64_t n) {
    if (n > MAX_SPECIALS) return api_set_error(HUTK_E_VALUE, "at most 1024 special tokens");
    if (offsets[0] < 0) return api_set_error(HUTK_E_VALUE, "special tokens: offsets[0] must not be negative");
    std::set<std::string> seen;
    for (int64_t i = 0; i < n; i++) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len < 1) return api_set_error(HUTK_E_VALUE, "a special token must not be empty");
        if (len > MAX_SPECIAL_BYTES) return api_set_error(HUTK_E_VALUE, "a special token must not be longer than 255 bytes");
        if (memchr(bytes + offsets[i], 0, (size_t)len)) return api_set_error(HUTK_E_VALUE, "a special token must not hold a 0x00 byte");
        if (ids[i] < 0) return api_set_error(HUTK_E_VALUE, "the id of a special token must not be negative");
        if (!seen.emplace(reinterpret_cast<const char*>(bytes + offsets[i]), (size_t)len).second)
            return api_set_error(HUTK_E_VALUE, "two special tokens are equal");
    }
    S.blob.clear();
    S.off.assign(1, 0u);
    S.ids.assign(ids, ids + n);
    S.filt.assign(24, 0u);
    S.max_len = 0;
    std::set<uint32_t> firsts;
    bool one_byte = false;
    for (int64_t i = 0; i < n; i++) {
        const uint8_t* s = bytes + offsets[i];
        const uint32_t len = (uint32_t)(offsets[i + 1] - offsets[i]);
        S.blob.insert(S.blob.end(), s, s + len);
        S.off.push_back((uint32_t)S.blob.size());
        S.filt[s[0] >> 5] |= 1u << (s[0] & 31);
        if (len >= 2) S.filt[8 + (s[1] >> 5)] |= 1u << (s[1] & 31);
        else one_byte = true;
        S.filt[16 + (len >> 5)] |= 1u << (len & 31);
        S.max_len = std::max(S.max_len, len);
        firsts.insert(s[0]);
    }
    if (one_byte)
        for (int k = 8; k < 16; k++) S.filt[k] = 0xFFFFFFFFu;
    S.n_first = firsts.size() <= 4 ? (uint32_t)firsts.size() : 0;
    int f = 0;
    for (int k = 0; k < 4; k++) S.first[k] = 0;
    if (S.n_first)
        for (uint32_t b : firsts) S.first[f++] = b * 0x01010101u;
    S.mask = 4 * MAX_SPECIALS - 1;  // at most a quarter full
    S.slots.assign((size_t)S.mask + 1, make_uint2(0, SLOT_NONE));
    for (int64_t i = 0; i < n; i++) {
        const uint32_t len = S.off[i + 1] - S.off[i];
        uint32_t h = FNV_BASIS;
        for (uint32_t j = 0; j < len; j++) h = sc_step(h, S.blob[S.off[i] + j]);
        uint32_t s = sc_slot(h, len) & S.mask;
        while (S.slots[s].y != SLOT_NONE) s = (s + 1) & S.mask;
        S.slots[s] = make_uint2(h, (uint32_t)i | len << 16);
    }
    S.n = n;
    return HUTK_OK;
}

// (the set's own tables and its decode tables: the device is selected and idle behind the first lines)
int upload_specials(hutk_ctx* c) {
    const hutk_ctx::Specials& S = c->sx;
    hutk_ctx::SpecialsDev& D = c->sxd;
    HUTK_HIP_TRY(hipSetDevice(c->device));
    HUTK_HIP_TRY(hipDeviceSynchronize());  // an earlier asynchronous call may still read the tables
    HUTK_HIP_TRY(D.d_blob.reserve(S.blob.size() + 16));
    HUTK_HIP_TRY(D.d_off.reserve(S.off.size()));
    HUTK_HIP_TRY(D.d_ids.reserve(S.ids.size() + 1));
    HUTK_HIP_TRY(D.d_filt.reserve(S.filt.size()));
    HUTK_HIP_TRY(D.d_slots.reserve(S.slots.size()));
    HUTK_HIP_TRY(hipMemcpy(D.d_blob.p, S.blob.data(), S.blob.size(), hipMemcpyHostToDevice));
    HUTK_HIP_TRY(hipMemcpy(D.d_off.p, S.off.data(), S.off.size() * 4, hipMemcpyHostToDevice));
    HUTK_HIP_TRY(hipMemcpy(D.d_ids.p, S.ids.data(), S.ids.size() * 4, hipMemcpyHostToDevice));
    HUTK_HIP_TRY(hipMemcpy(D.d_filt.p, S.filt.data(), S.filt.size() * 4, hipMemcpyHostToDevice));
    HUTK_HIP_TRY(hipMemcpy(D.d_slots.p, S.slots.data(), S.slots.size() * sizeof(uint2), hipMemcpyHostToDevice));
    return D.dec.upload(S.dec);
}

// The decode tables of the context extended by the set (hutk_ctx::Specials::dec): validated and built on the host, whatever
// the context.  Entry k belongs to the k-th DISTINCT id in the order of the pairs, its bytes are those of the id's first pair.
int build_decode_specials(const hutk_ctx* c, hutk_ctx::Specials& S) {
    DecExt::Host& X = S.dec;
    X.slots.assign(DSP_SLOTS, make_uint2(0, DSP_EMPTY));
    X.id_min = INT32_MAX;
    X.id_max = 0;
    std::vector<std::pair<const uint8_t*, uint32_t>> extra;
    for (int64_t i = 0; i < S.n; i++) {
        const int32_t id = S.ids[i];
        uint32_t s = dsp_slot((uint32_t)id);
        while (X.slots[s].y != DSP_EMPTY && (int32_t)X.slots[s].x != id) s = (s + 1) & (DSP_SLOTS - 1);
        if (X.slots[s].y != DSP_EMPTY) continue;  // a later string of the same id: the first one is the id's text
        X.slots[s] = make_uint2((uint32_t)id, (uint32_t)extra.size());
        X.id_min = std::min(X.id_min, id);
        X.id_max = std::max(X.id_max, id);
        extra.emplace_back(S.blob.data() + S.off[i], S.off[i + 1] - S.off[i]);
    }
    return dec_ext_build(c->tab, nullptr, extra, true, "special tokens: the vocabulary leaves no ids for the decode tables", X);
}

// prefix units a document can get, units an input item can become: what hutk_ids_capacity multiplies by
int64_t cap_pad(const hutk_ctx* c) { return hutk_ids_capacity(c, 0, 1) - 1; }
int64_t cap_units(const hutk_ctx* c) { return hutk_ids_capacity(c, 1, 0) - 1; }

}  // namespace

void launch_scan_i64(int64_t* a, int64_t n, hipStream_t s) { hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(1024), 0, s, a, n); }

void launch_dec_remap(const DecSpecial& sp, const int32_t* ids, int32_t* ids_out, int64_t n_ids, uint32_t* first_bits,
                      hipStream_t s) {
    hipLaunchKernelGGL(k_dsp_remap, dim3((unsigned)((n_ids + DSP_TILE - 1) / DSP_TILE)), dim3(DSP_THREADS), 0, s, sp, ids,
                       ids_out, n_ids, first_bits);
}

}  // namespace hutk

using namespace hutk;

extern "C" {

int hutk_ctx_set_special_tokens(hutk_ctx* c, const uint8_t* bytes, const int64_t* offsets, const int32_t* ids, int64_t n) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!bytes || !offsets || !ids))) return api_set_error(HUTK_E_ARG, "hutk_ctx_set_special_tokens: bad arguments");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (n == 0) {
        c->sx.n = 0;
        return fallback_rebuild_decode(c);
    }
    // A set that is refused leaves the one in force as it was, its decode tables too: the new one is built aside.  While
    // the uploads run no set is in force (n is 0: a failed upload leaves the device arrays half replaced).  The byte-fallback
    // decode's tables hold the set's entries: they are rebuilt after every change of the set, its removal above included.
    hutk_ctx::Specials fresh;
    if (int rc = build_specials(fresh, bytes, offsets, ids, n)) return rc;
    if (int rc = build_decode_specials(c, fresh)) return rc;
    c->sx = std::move(fresh);
    c->sx.n = 0;
    if (!c->host_only)
        if (int rc = upload_specials(c)) return rc;
    c->sx.n = n;
    return fallback_rebuild_decode(c);
}

int64_t hutk_ctx_special_token_count(const hutk_ctx* c) { return c ? c->sx.n : 0; }
int64_t hutk_special_last_matches(const hutk_ctx* c) { return c ? c->sxd.last_matches : 0; }
int hutk_debug_special_tile_bytes(void) { return SC_TILE; }

int64_t hutk_special_ids_capacity(const hutk_ctx* c, int64_t n_bytes, int64_t n_docs) {
    if (!c) return 0;
    const int64_t pad = cap_pad(c), units = cap_units(c);
    return n_bytes * std::max(units, pad + 1) + pad * n_docs + 1;
}

int hutk_encode_special_batch_device(hutk_ctx* c, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                     int64_t n_bytes, int32_t* d_ids_out, int64_t ids_cap, int64_t* d_out_offsets,
                                     int32_t* d_status, int32_t* d_err, void* hip_stream) {
    return encode_special_impl(c, false, d_bytes, d_offsets, n_docs, n_bytes, d_ids_out, ids_cap, d_out_offsets, d_status, d_err,
                               hip_stream);
}

}  // extern "C"

// fallback: the text pieces are encoded with byte fallback (hutk_fallback.hip, which has checked what that needs)
int hutk::encode_special_impl(hutk_ctx* c, bool fallback, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                              int64_t n_bytes, int32_t* d_ids_out, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_status,
                              int32_t* d_err, void* hip_stream) {
    const auto encode = [&](const int64_t* offs, int64_t n, int32_t* ids, int64_t cap, int64_t* oo, int32_t* status, int32_t* err) {
        return fallback ? encode_fallback_device_impl(c, d_bytes, offs, n, n_bytes, ids, cap, oo, status, err, hip_stream)
                        : encode_device_impl(c, d_bytes, offs, n, n_bytes, ids, cap, oo, status, err, hip_stream, nullptr, nullptr);
    };
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to encode on");
    if (n_docs < 0 || n_bytes < 0 || !d_offsets || !d_out_offsets || (n_bytes > 0 && (!d_bytes || !d_ids_out)))
        return api_set_error(HUTK_E_ARG, "hutk_encode_special_batch_device: bad arguments");
    if (((uintptr_t)d_bytes & 15u) != 0) return api_set_error(HUTK_E_ARG, "d_bytes must be 16-byte aligned");
    std::lock_guard<std::recursive_mutex> lock(c->mu);  // held once around the whole call: scan, encode, stitch
    if (!c->pattern.empty())
        return api_set_error(HUTK_E_UNSUPPORTED, "hutk_encode_special_batch_device: a regex pattern drops the text between its "
                                                 "matches; the pieces between special tokens are not documents of their own");
    if (ids_cap < hutk_special_ids_capacity(c, n_bytes, n_docs) - 1)
        return api_set_error(HUTK_E_CAPACITY, "ids_cap is below hutk_special_ids_capacity()");
    const hutk_ctx::Specials& S = c->sx;
    hutk_ctx::SpecialsDev& W = c->sxd;
    W.last_matches = 0;
    if (S.n == 0 || n_docs == 0 || n_bytes == 0)  // nothing to find: the plain encode
        return encode(d_offsets, n_docs, d_ids_out, ids_cap, d_out_offsets, d_status, d_err);
    const int64_t n_tiles = (n_bytes + SC_TILE - 1) / SC_TILE;
    if (n_tiles > 0x7FFFFFFFll) return api_set_error(HUTK_E_ARG, "batch too large");
    HUTK_HIP_TRY(hipSetDevice(c->device));
    HUTK_HIP_TRY(W.w_mlen.reserve((size_t)n_bytes + 16));
    HUTK_HIP_TRY(W.w_sel.reserve((size_t)n_bytes + 16));
    HUTK_HIP_TRY(W.w_tile.reserve((size_t)n_tiles + 1));
    HUTK_HIP_TRY(c->w_err.reserve(1));
    SpecTab T{};
    T.slots = W.d_slots.p;
    T.blob = W.d_blob.p;
    T.off = W.d_off.p;
    T.ids = W.d_ids.p;
    T.filt = W.d_filt.p;
    T.mask = S.mask;
    T.max_len = S.max_len;
    T.n_first = S.n_first;
    memcpy(T.first, S.first, sizeof T.first);
    SpecArgs A{};
    A.bytes = d_bytes;
    A.offs = d_offsets;
    A.n_docs = n_docs;
    A.n_bytes = n_bytes;
    A.n_tiles = n_tiles;
    A.mlen = W.w_mlen.p;
    A.sel = W.w_sel.p;
    A.tile_base = W.w_tile.p;
    A.err = d_err ? d_err : c->w_err.p;
    A.out_ids = d_ids_out;
    A.ids_cap = ids_cap;
    A.out_offsets = d_out_offsets;
    A.status = d_status;
    int64_t n_matches = 0;
    hipStream_t s;
    {
        StreamScope scope(c, hip_stream, false);  // (the device was selected in front of the allocations)
        if (scope.rc) return scope.rc;
        s = scope.s;
        const dim3 grid((unsigned)n_tiles), block(SC_THREADS);
        HUTK_HIP_TRY(hipMemsetAsync(A.sel, 0, (size_t)n_bytes + 16, s));
        hipLaunchKernelGGL(k_sc_find, grid, block, 0, s, T, A);
        hipLaunchKernelGGL(k_sc_resolve, grid, block, 0, s, A, T.max_len);
        hipLaunchKernelGGL(k_sc_count, grid, block, 0, s, A);
        hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(1024), 0, s, A.tile_base, n_tiles);
        HUTK_HIP_TRY(hipGetLastError());
        // the ONE synchronisation of the call: the number of matches sizes the piece-wise encode
        HUTK_HIP_TRY(hipMemcpyAsync(&n_matches, A.tile_base + n_tiles, 8, hipMemcpyDeviceToHost, s));
        HUTK_HIP_TRY(hipStreamSynchronize(s));
    }
    if (n_matches < 0 || n_matches > n_bytes) return api_set_error(HUTK_E_DEVICE, "hutk_encode_special_batch_device: bad match count");
    W.last_matches = n_matches;
    if (n_matches == 0)
        return encode(d_offsets, n_docs, d_ids_out, ids_cap, d_out_offsets, d_status, d_err);
    const int64_t n_pieces = n_docs + 2 * n_matches;
    if (n_pieces > (int64_t)INT32_MAX - 1) return api_set_error(HUTK_E_UNSUPPORTED, "hutk_encode_special_batch_device: too many pieces for one encode");
    const int64_t pieces_cap = hutk_ids_capacity(c, n_bytes, n_pieces);
    const int64_t n_blocks = (n_pieces + ST_BLOCK - 1) / ST_BLOCK;
    HUTK_HIP_TRY(W.w_mstart.reserve((size_t)n_matches));
    HUTK_HIP_TRY(W.w_poff.reserve((size_t)n_pieces + 1));
    HUTK_HIP_TRY(W.w_pspecial.reserve((size_t)n_pieces));
    HUTK_HIP_TRY(W.w_first.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(W.w_poo.reserve((size_t)n_pieces + 1));
    HUTK_HIP_TRY(W.w_pstatus.reserve((size_t)n_pieces));
    HUTK_HIP_TRY(W.w_pids.reserve((size_t)pieces_cap + 16));
    HUTK_HIP_TRY(W.w_blk.reserve((size_t)n_blocks + 1));
    HUTK_HIP_TRY(W.w_dst.reserve((size_t)n_pieces + 1));
    A.m_start = W.w_mstart.p;
    A.n_matches = n_matches;
    A.n_pieces = n_pieces;
    A.piece_off = W.w_poff.p;
    A.piece_special = W.w_pspecial.p;
    A.first_piece = W.w_first.p;
    A.piece_oo = W.w_poo.p;
    A.piece_status = W.w_pstatus.p;
    A.piece_ids = W.w_pids.p;
    A.blk = W.w_blk.p;
    A.dst = W.w_dst.p;
    {
        StreamScope scope(c, hip_stream, false);
        if (scope.rc) return scope.rc;
        HUTK_HIP_TRY(hipMemsetAsync(A.piece_special, 0xFF, (size_t)n_pieces * 4, s));
        hipLaunchKernelGGL(k_sc_write, dim3((unsigned)n_tiles), dim3(SC_THREADS), 0, s, T, A);
        hipLaunchKernelGGL(k_sc_docs, dim3((unsigned)((n_docs + 256) / 256)), dim3(256), 0, s, A);
        HUTK_HIP_TRY(hipGetLastError());
    }
    // the pieces, special ones included (a document's pieces are contiguous, a marker is a few ids), as documents of their own
    if (int rc = encode(A.piece_off, n_pieces, W.w_pids.p, pieces_cap, W.w_poo.p, W.w_pstatus.p, A.err)) return rc;
    {
        StreamScope scope(c, hip_stream, false);
        if (scope.rc) return scope.rc;
        hipLaunchKernelGGL(k_st_sum, dim3((unsigned)n_blocks), dim3(ST_THREADS), 0, s, A);
        hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(1024), 0, s, A.blk, n_blocks);
        hipLaunchKernelGGL(k_st_dst, dim3((unsigned)n_blocks), dim3(ST_THREADS), 0, s, A, n_blocks);
        hipLaunchKernelGGL(k_st_docs, dim3((unsigned)((n_docs + 256) / 256)), dim3(256), 0, s, A);
        // (the host does not know the number of ids: a workgroup for every CP_TILE ids the output can hold at most)
        const int64_t bound = hutk_special_ids_capacity(c, n_bytes, n_docs);
        const int64_t copy_blocks = (bound + CP_TILE - 1) / CP_TILE;
        if (copy_blocks > 0x7FFFFFFFll) return api_set_error(HUTK_E_ARG, "batch too large");
        hipLaunchKernelGGL(k_st_copy, dim3((unsigned)copy_blocks), dim3(CP_THREADS), 0, s, A);
        HUTK_HIP_TRY(hipGetLastError());
    }
    return HUTK_OK;
}

extern "C" {

int hutk_encode_special_batch(hutk_ctx* c, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, int32_t* ids_out,
                              int64_t ids_cap, int64_t* out_offsets, int32_t* status) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to encode on");
    if (n_docs < 0 || !offsets || !out_offsets) return api_set_error(HUTK_E_ARG, "hutk_encode_special_batch: bad arguments");
    if (int rc = check_offsets(offsets, n_docs, true, "offsets")) return rc;
    const int64_t n_bytes = offsets[n_docs];
    if (n_bytes > 0 && (!bytes || !ids_out)) return api_set_error(HUTK_E_ARG, "hutk_encode_special_batch: a buffer is NULL");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    const int64_t cap = hutk_special_ids_capacity(c, n_bytes, n_docs);
    if (ids_cap < cap - 1) return api_set_error(HUTK_E_CAPACITY, "ids_cap is below hutk_special_ids_capacity()");
    const auto device = [&](const uint8_t* d_bytes, const int64_t* d_offs, int32_t* d_ids, int64_t* d_oo, int32_t* d_status,
                            int32_t* d_err, hipStream_t s) {
        return hutk_encode_special_batch_device(c, d_bytes, d_offs, n_docs, n_bytes, d_ids, cap, d_oo, d_status, d_err, s);
    };
    const auto refuse = [](int err) { return api_set_error(err, device_error_message(Direction::Encode, err)), true; };
    return encode_host_impl(c, "hutk_encode_special_batch", cap, device, refuse, bytes, offsets, n_docs, n_bytes, ids_out, ids_cap,
                            out_offsets, status);
}

int hutk_decode_special_batch_device(hutk_ctx* c, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_docs,
                                     int64_t n_ids, int flags, uint8_t* d_bytes_out, int64_t bytes_cap, int64_t* d_out_offsets,
                                     int32_t* d_status, int32_t* d_err, void* hip_stream) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (flags & ~HUTK_DECODE_SKIP_SPECIAL) return api_set_error(HUTK_E_ARG, "hutk_decode_special_batch_device: unknown flags");
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to decode on");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    const DecExt::Host& X = c->sx.dec;
    if (c->sx.n == 0)  // no set: the plain decode
        return decode_device_impl(c, c->dec, nullptr, d_ids, d_id_offsets, n_docs, n_ids, d_bytes_out, bytes_cap, d_out_offsets,
                                  d_status, d_err, hip_stream);
    const bool skip = (flags & HUTK_DECODE_SKIP_SPECIAL) != 0;
    DecSpecial P{};
    P.slots = c->sxd.dec.dx_slots.p;
    P.id_min = X.id_min;
    P.id_max = X.id_max;
    P.n_vocab = (int32_t)c->dec.n;
    P.bits = !X.strip ? DSP_BITS_NONE : skip ? DSP_BITS_SKIP : DSP_BITS_AFTER;
    return decode_device_impl(c, c->sxd.dec.tables(skip), &P, d_ids, d_id_offsets, n_docs, n_ids, d_bytes_out, bytes_cap,
                              d_out_offsets, d_status, d_err, hip_stream);
}

int hutk_decode_special_batch(hutk_ctx* c, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, int flags,
                              uint8_t* bytes_out, int64_t bytes_cap, int64_t* out_offsets, int32_t* status) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (flags & ~HUTK_DECODE_SKIP_SPECIAL) return api_set_error(HUTK_E_ARG, "hutk_decode_special_batch: unknown flags");
    const auto device = [&](const int32_t* d_ids, const int64_t* d_offs, int64_t n_ids, uint8_t* d_bytes, int64_t* d_oo,
                            int32_t* d_status, int32_t* d_err, hipStream_t s) {
        return hutk_decode_special_batch_device(c, d_ids, d_offs, n_docs, n_ids, flags, d_bytes, bytes_cap, d_oo, d_status, d_err, s);
    };
    return decode_host_impl(c, device, ids, id_offsets, n_docs, bytes_out, bytes_cap, out_offsets, status);
}

}  // extern "C"
