// hutk_spans.hip -- token offset mapping on the device: for every id of an encoded batch, the stretch [start, end) of its
// document that the token covers, in bytes or in characters (include/hutoken_amd.h).
//
// A token covers a whole number of the pretokenizer's items (src/pretokenizer.c:102-168): its decoded text -- the entry of
// the decode tables, prefix-stripped for a document's first token -- or, for an id of -1, the one item at the cursor.  So
//   byte-encoder mode   a token's BYTE count is a constant of its id (-1: one byte); a segmented scan over the ids gives
//                       the byte spans; character offsets are ranks in the bitmap of character starts of the source
//   character mode      a token's ITEM count is a constant of its id (-1: one item) and items are characters; the same
//                       scan gives the character spans; byte offsets are selects: where the k-th character starts
// and nothing is trusted: the decoded bytes of every known id are compared with the source bytes of its span, the length
// of every -1 item with what the pretokenizer's rule says at that place.  A difference marks the document
// (HUTK_DOC_SPAN_MISMATCH) and the call (HUTK_E_UNSUPPORTED).
//
//   k_sp_check    offsets that do not describe the buffers end the call (HUTK_E_ARG, nothing else runs); first-token bitmap
//   k_sp_bits     character-start bits of the source, 64 per word, and their counts inside chunks of 16 KiB
//   k_sp_chunks   exclusive scan of the chunk counts (one workgroup)
//   k_sp_scatter  character mode: sel[k] = byte position of the k-th character start (HUTK_SPANS_SELECT=search: not
//                 built; select searches the counts of the rank structure instead -- the slower form)
//   k_sp_pre      first document per tile of SP_TILE ids
//   k_sp_tiles    ONE pass over the ids: units per token, segmented workgroup scan, the units since the document's start
//                 in front of the tile by decoupled look-back (as k_dec_tiles: flag and value in one 64-bit word, relaxed
//                 agent-scope atomics, and a tile that waits too long adds its predecessor up itself), verify, write
//
// The direction's C entry points are at the end of the file: hutk_token_spans_device (device buffers, asynchronous) and
// hutk_token_spans (host buffers, staged through the context's).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "hutk_host.h"

namespace hutk {

namespace {

constexpr int SP_THREADS = 256, SP_PER = 8, SP_TILE = SP_THREADS * SP_PER;
static_assert(SP_PER % 4 == 0 && 32 % SP_PER == 0, "16-byte id loads; a thread's first-token bits sit in one word");
constexpr int SP_BLOCKS_PER_CHUNK = SPAN_CHUNK_BYTES / 64;
static_assert(SP_BLOCKS_PER_CHUNK == 256, "k_sp_bits: one thread per 64-byte block of a chunk");
// look-back state: PART = units of a tile without a document start (the sum goes on in front of it), FINAL = units
// between the last document start at or before the tile's end and that end (nothing in front of the tile matters)
constexpr unsigned long long SP_ST_MASK = 3ull << 62, SP_ST_PART = 1ull << 62, SP_ST_FINAL = 2ull << 62;
constexpr uint64_t HI_BITS = 0x8080808080808080ull;

__device__ __forceinline__ void sp_raise(int32_t* err, int32_t code) { atomicCAS(err, 0, code); }
__device__ __forceinline__ uint32_t is_start(uint32_t b) { return (b & 0xC0u) != 0x80u; }
// continuation bytes (10xxxxxx) among the eight bytes of x, as their top bits
__device__ __forceinline__ uint64_t cont_bits(uint64_t x) { return x & ~(x << 1) & HI_BITS; }
// the four character-start flags of a dword, as bits 0..3
__device__ __forceinline__ uint32_t start_nibble(uint32_t x) {
    const uint32_t y = ((~(x & ~(x << 1))) >> 7) & 0x01010101u;
    return (y * 0x01020408u) >> 24 & 0xFu;
}

template <class V>
__device__ __forceinline__ V wave_incl(V v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const V p = __shfl_up(v, off);
        if (lane >= off) v += p;
    }
    return v;
}

// ---- offsets, first tokens ----------------------------------------------------------------------------------------
__global__ void k_sp_check(SpanArgs A, int narrow) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= A.n_docs) return;
    const int64_t b0 = A.doc_offs[d], b1 = A.doc_offs[d + 1], i0 = A.id_offs[d], i1 = A.id_offs[d + 1];
    bool bad = b0 < 0 || b1 < b0 || b1 > A.n_bytes || i0 < 0 || i1 < i0 || i1 > A.n_ids;
    if (d == 0) bad = bad || i0 != 0;
    if (d == A.n_docs - 1) bad = bad || i1 != A.n_ids;
    if (narrow && !bad) bad = b1 - b0 > (int64_t)INT32_MAX;  // the span would not fit an int32
    if (bad) {
        *A.ok = 0;
        sp_raise(A.err, HUTK_E_ARG);
        return;
    }
    if (i1 > i0) atomicOr(&A.first_bits[i0 >> 5], 1u << (i0 & 31));
}

// first document whose first token is at or after the tile's first token (as k_dec_pre)
__global__ void k_sp_pre(SpanArgs A) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n_tiles || !*A.ok) return;
    const int64_t t0 = t * SP_TILE;
    int64_t lo = 0, hi = A.n_docs + 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.id_offs[mid] < t0) lo = mid + 1; else hi = mid;
    }
    A.tile_first_doc[t] = lo;
}

// ---- rank / select over the character starts of the source -----------------------------------------------------
__global__ __launch_bounds__(SP_BLOCKS_PER_CHUNK) void k_sp_bits(SpanArgs A) {
    __shared__ __attribute__((aligned(8))) uint16_t s_m[SPAN_CHUNK_BYTES / 16];
    __shared__ uint32_t s_part[SP_BLOCKS_PER_CHUNK / 64];
    const int tid = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    const int64_t base = chunk * SPAN_CHUNK_BYTES;
    const bool aligned = (reinterpret_cast<uintptr_t>(A.bytes) & 15) == 0;
    // coalesced: consecutive threads read consecutive 16-byte pieces, each gives 16 start bits
#pragma unroll
    for (int j = 0; j < SPAN_CHUNK_BYTES / 16 / SP_BLOCKS_PER_CHUNK; j++) {
        const int q = j * SP_BLOCKS_PER_CHUNK + tid;
        const int64_t pos = base + (int64_t)q * 16;
        uint32_t m = 0;
        if (aligned && pos + 16 <= A.n_bytes) {
            const uint4 v = *reinterpret_cast<const uint4*>(A.bytes + pos);
            m = start_nibble(v.x) | start_nibble(v.y) << 4 | start_nibble(v.z) << 8 | start_nibble(v.w) << 12;
        } else {
            for (int b = 0; b < 16; b++)
                if (pos + b < A.n_bytes) m |= is_start(A.bytes[pos + b]) << b;
        }
        s_m[q] = (uint16_t)m;
    }
    __syncthreads();
    const uint64_t w = *reinterpret_cast<const uint64_t*>(&s_m[tid * 4]);  // the 64 bytes of this thread's block
    const uint32_t cnt = (uint32_t)__popcll(w);
    const int lane = tid & 63;
    const uint32_t incl = wave_incl(cnt, lane);
    if (lane == 63) s_part[tid >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - cnt;
    for (int u = 0; u < (tid >> 6); u++) before += s_part[u];
    const int64_t blk = chunk * SP_BLOCKS_PER_CHUNK + tid;
    A.rk_bits[blk] = w;
    A.rk_in_chunk[blk] = before;
    if (tid == SP_BLOCKS_PER_CHUNK - 1) A.rk_chunk[chunk] = before + cnt;
}

__global__ __launch_bounds__(1024) void k_sp_chunks(SpanArgs A) {
    __shared__ int64_t s_part[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    for (int64_t at = 0; at < A.n_chunks; at += 1024) {
        const int64_t i = at + tid;
        const int64_t v = i < A.n_chunks ? A.rk_chunk[i] : 0;
        const int64_t incl = wave_incl(v, lane);
        if (lane == 63) s_part[w] = incl;
        __syncthreads();
        int64_t before = 0, total = 0;
        for (int u = 0; u < 16; u++) {
            if (u < w) before += s_part[u];
            total += s_part[u];
        }
        if (i < A.n_chunks) A.rk_chunk[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) A.rk_chunk[A.n_chunks] = carry;
}

__device__ __forceinline__ int64_t sp_rank(const SpanArgs& A, int64_t p) {  // starts in bytes[0, p), 0 <= p <= n_bytes
    const int64_t b = p >> 6;
    return A.rk_chunk[b >> 8] + A.rk_in_chunk[b] + __popcll(A.rk_bits[b] & ((1ull << (p & 63)) - 1ull));
}

template <class S>
__global__ void k_sp_scatter(SpanArgs A) {
    const int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= A.n_chunks * SP_BLOCKS_PER_CHUNK) return;
    S* sel = static_cast<S*>(A.sel);
    uint64_t w = A.rk_bits[blk];
    int64_t r = A.rk_chunk[blk >> 8] + A.rk_in_chunk[blk];
    const int64_t pos = blk * 64;
    while (w) {
        sel[r++] = (S)(pos + __builtin_ctzll(w));
        w &= w - 1;
    }
    if (blk == 0) sel[A.rk_chunk[A.n_chunks]] = (S)A.n_bytes;
}

// select without the scattered array: the last chunk, then the last 64-byte block of it, with at most k starts in front,
// then the word's (k - those)-th set bit.  0 <= k < n_starts.
__device__ __forceinline__ int64_t sp_select_search(const SpanArgs& A, int64_t k) {
    int64_t lo = 0, hi = A.n_chunks - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (A.rk_chunk[mid] <= k) lo = mid; else hi = mid - 1;
    }
    uint32_t r = (uint32_t)(k - A.rk_chunk[lo]);
    const uint32_t* in = A.rk_in_chunk + lo * SP_BLOCKS_PER_CHUNK;
    int a = 0, b = SP_BLOCKS_PER_CHUNK - 1;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (in[mid] <= r) a = mid; else b = mid - 1;
    }
    r -= in[a];
    const int64_t blk = lo * SP_BLOCKS_PER_CHUNK + a;
    uint64_t w = A.rk_bits[blk];  // holds more than r starts: the block behind it has more than k in front
    for (; r && w; r--) w &= w - 1;
    return w ? blk * 64 + __builtin_ctzll(w) : A.n_bytes;
}

// byte position of the k-th character start of the batch; k beyond the last one: n_bytes
template <bool SEARCH>
__device__ __forceinline__ int64_t sp_select(const SpanArgs& A, int64_t k, int64_t n_starts) {
    if (k < 0) k = 0;
    if (k > n_starts) k = n_starts;
    if (SEARCH) return k == n_starts ? A.n_bytes : sp_select_search(A, k);
    return A.sel_wide ? static_cast<const int64_t*>(A.sel)[k] : (int64_t)static_cast<const uint32_t*>(A.sel)[k];
}

// ---- tokens -------------------------------------------------------------------------------------------------------
enum : uint32_t { TOK_KNOWN = 0, TOK_UNKNOWN = 1, TOK_BAD = 2 };

// the decode-table entry of a token and what kind it is; an id of -1 and an id that cannot be decoded have an empty entry
__device__ __forceinline__ uint2 sp_entry(const DecTables& T, int32_t id, bool first, uint32_t& kind) {
    kind = TOK_KNOWN;
    if (id == -1) {
        kind = TOK_UNKNOWN;
        return make_uint2(0, 0);
    }
    if (id < 0 || (int64_t)id >= T.n) {
        kind = TOK_BAD;
        return make_uint2(0, 0);
    }
    const uint2 e = (first && T.sent) ? T.sent[id] : T.ent[id];
    if ((e.x & 0xFFu) == DEC_TAG_BAD) {
        kind = TOK_BAD;
        return make_uint2(0, 0);
    }
    return e;
}
__device__ __forceinline__ uint32_t sp_len(uint2 e) { return (e.x & DEC_TAG_LONG) ? e.x >> 8 : (e.x & 0xFFu); }
__device__ __forceinline__ uint64_t sp_inline(uint2 e) { return (((uint64_t)e.y << 32) | e.x) >> 8; }

// what the scan adds up: bytes in byte-encoder mode, items (the characters of the decoded text) otherwise
template <bool BYTE>
__device__ __forceinline__ uint32_t sp_units(const DecTables& T, uint2 e, uint32_t kind) {
    if (kind == TOK_UNKNOWN) return 1u;
    const uint32_t len = sp_len(e);
    if (BYTE) return len;
    if (!(e.x & DEC_TAG_LONG)) return len - (uint32_t)__popcll(cont_bits(sp_inline(e)));
    uint32_t n = 0;
    const uint8_t* src = T.blob + e.y;
    for (uint32_t j = 0; j < len; j++) n += is_start(src[j]);
    return n;
}

// Tile p's look-back state, computed by ONE lane: what a workgroup falls back on when a tile in front of its own has not
// published for a long time (see k_dec_tiles).
template <bool BYTE>
__device__ __forceinline__ unsigned long long sp_tile_state(const DecTables& T, const SpanArgs& A, int64_t p) {
    const int64_t a = p * SP_TILE, b = (a + SP_TILE < A.n_ids) ? a + SP_TILE : A.n_ids;
    unsigned long long sum = 0;
    bool start = p == 0;
    for (int64_t i = a; i < b; i++) {
        const bool first = (A.first_bits[i >> 5] >> (i & 31)) & 1u;
        if (first) {
            sum = 0;
            start = true;
        }
        uint32_t kind;
        const uint2 e = sp_entry(T, A.ids[i], first, kind);
        sum += sp_units<BYTE>(T, e, kind);
    }
    return (start ? SP_ST_FINAL : SP_ST_PART) | sum;
}

// n <= 7 source bytes at position p (0 <= p, p + n <= n_bytes), as the low bytes of a word
__device__ __forceinline__ uint64_t sp_fetch(const SpanArgs& A, int64_t p, uint32_t n) {
    if (n == 0) return 0;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(A.bytes) + (uintptr_t)p;
    const uintptr_t a0 = addr & ~(uintptr_t)7;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(A.bytes), hi = lo + (uintptr_t)A.n_bytes;
    uint64_t v;
    if (a0 >= lo && a0 + 16 <= hi) {  // two aligned 8-byte loads inside the buffer
        const uint64_t* q = reinterpret_cast<const uint64_t*>(a0);
        const uint32_t sh = (uint32_t)(addr & 7) * 8;
        const uint64_t w0 = q[0], w1 = q[1];
        v = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
    } else {
        v = 0;
        for (uint32_t j = 0; j < n; j++) v |= (uint64_t)A.bytes[p + j] << (8 * j);
    }
    return v & ((1ull << (8 * n)) - 1ull);
}

// Does the source hold the token's decoded bytes at [p, p + n)?  n is the token's length and the range is inside the
// buffer.  starts: the character starts among those source bytes.
__device__ __forceinline__ bool sp_same(const DecTables& T, const SpanArgs& A, uint2 e, int64_t p, uint32_t n, uint32_t& starts) {
    if (!(e.x & DEC_TAG_LONG)) {
        const uint64_t v = sp_fetch(A, p, n);
        starts = n - (uint32_t)__popcll(cont_bits(v));
        return v == sp_inline(e);
    }
    const uint8_t* want = T.blob + e.y;
    bool same = true;
    starts = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t b = A.bytes[p + j];
        same = same && b == want[j];
        starts += is_start(b);
    }
    return same;
}

// the pretokenizer's item length in character mode (pretokenizer.c:14-28)
__device__ __forceinline__ uint32_t utf8_item_len(uint32_t b) {
    return (b & 0x80u) == 0 ? 1u : (b & 0xE0u) == 0xC0u ? 2u : (b & 0xF0u) == 0xE0u ? 3u : (b & 0xF8u) == 0xF0u ? 4u : 1u;
}

template <bool BYTE, int W, bool SEARCH = false>
__global__ __launch_bounds__(SP_THREADS) void k_sp_tiles(DecTables T, SpanArgs A) {
    __shared__ uint16_t s_rank[SP_TILE];     // document starts in the tile up to and including each token
    __shared__ int32_t s_doc[SP_TILE + 1];   // the r-th document that starts in the tile, counted from tile_first_doc
    __shared__ uint32_t s_wsum[SP_THREADS / 64], s_wflag[SP_THREADS / 64], s_wcnt[SP_THREADS / 64];
    __shared__ int64_t s_carry;
    if (!*A.ok) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t t0 = tile * SP_TILE;
    const int64_t i0 = t0 + (int64_t)tid * SP_PER;
    uint32_t firsts = 0;  // bit k: token i0 + k starts a document
    if (i0 < A.n_ids) firsts = (A.first_bits[i0 >> 5] >> (i0 & 31)) & ((1u << SP_PER) - 1u);
    int32_t id[SP_PER];
    if (i0 + SP_PER <= A.n_ids && (reinterpret_cast<uintptr_t>(A.ids) & 15) == 0) {  // two 16-byte loads
#pragma unroll
        for (int g = 0; g < SP_PER; g += 4) {
            const int4 a = *reinterpret_cast<const int4*>(A.ids + i0 + g);
            id[g] = a.x; id[g + 1] = a.y; id[g + 2] = a.z; id[g + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < SP_PER; k++) id[k] = (i0 + k < A.n_ids) ? A.ids[i0 + k] : 0;
    }
    uint2 ent[SP_PER];
    uint32_t units[SP_PER];
    uint32_t kinds = 0;  // two bits per token
    uint32_t mine = 0;   // units behind the thread's last document start (all of them when it has none)
    // (uint32 up to the tile's total: hutk_token_spans_device refuses a vocabulary whose longest token times SP_TILE
    // does not fit; the carry between tiles is 64-bit)
#pragma unroll
    for (int k = 0; k < SP_PER; k++) {
        ent[k] = make_uint2(0, 0);
        units[k] = 0;
        if (i0 + k < A.n_ids) {
            uint32_t kind;
            ent[k] = sp_entry(T, id[k], (firsts >> k) & 1u, kind);
            units[k] = sp_units<BYTE>(T, ent[k], kind);
            kinds |= kind << (2 * k);
        }
        if ((firsts >> k) & 1u) mine = 0;
        mine += units[k];
    }
    // Segmented scan over the threads: (has a start, units behind the last start), and the plain count of starts.
    uint32_t sf = firsts != 0, ss = mine, sc = (uint32_t)__popc(firsts);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t pf = __shfl_up(sf, off), ps = __shfl_up(ss, off), pc = __shfl_up(sc, off);
        if (lane >= off) {
            if (!sf) ss += ps;
            sf |= pf;
            sc += pc;
        }
    }
    if (lane == 63) {
        s_wflag[wave] = sf;
        s_wsum[wave] = ss;
        s_wcnt[wave] = sc;
    }
    uint32_t xf = __shfl_up(sf, 1), xs = __shfl_up(ss, 1), xc = __shfl_up(sc, 1);  // exclusive, inside the wavefront
    if (lane == 0) xf = 0, xs = 0, xc = 0;
    __syncthreads();
    uint32_t tile_f = 0, tile_s = 0;
    {
        uint32_t bf = 0, bs = 0, bc = 0;  // the wavefronts in front of this one
#pragma unroll
        for (int u = 0; u < SP_THREADS / 64; u++) {
            const uint32_t f = s_wflag[u], s = s_wsum[u];
            if (u < wave) {
                bs = f ? s : bs + s;
                bf |= f;
                bc += s_wcnt[u];
            }
            tile_s = f ? s : tile_s + s;
            tile_f |= f;
        }
        xs = xf ? xs : bs + xs;
        xf |= bf;
        xc += bc;
    }
    // The units between the document's start and the tile, by decoupled look-back (k_dec_tiles has the reasoning): a tile
    // with a document start publishes its final state at once, the others what they add, and then what they found.
    unsigned long long* st = A.tile_state;
    const bool final_now = tile_f || tile == 0;
    if (tid == 0)
        __hip_atomic_store(&st[tile], (final_now ? SP_ST_FINAL : SP_ST_PART) | (unsigned long long)tile_s, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    // meanwhile: the starts up to each token, for the list of the tile's documents
    {
        uint32_t r = xc;
#pragma unroll
        for (int k = 0; k < SP_PER; k++) {
            r += (firsts >> k) & 1u;
            s_rank[tid * SP_PER + k] = (uint16_t)r;
        }
    }
    if (tid < 64) {  // wavefront 0 looks back
        int64_t carry = 0;
        const bool head_starts = (__shfl((int)firsts, 0) & 1) != 0;  // the tile's first token starts a document: nothing to carry
        if (tile > 0 && !head_starts) {
            bool found = false;
            for (int64_t hi = tile - 1; !found; hi -= 64) {
                const int64_t p = hi - lane;
                unsigned long long v = SP_ST_FINAL;  // before tile 0: nothing
                uint32_t spins = 0;
                for (;;) {
                    if (p >= 0) v = __hip_atomic_load(&st[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (__all((v & SP_ST_MASK) != 0)) break;
                    if (++spins > A.help_after) {  // not dispatched yet, perhaps never before we leave
                        if ((v & SP_ST_MASK) == 0) v = sp_tile_state<BYTE>(T, A, p);
                        break;
                    }
                }
                const unsigned long long final_at = __ballot((v & SP_ST_MASK) == SP_ST_FINAL);
                const int stop = final_at ? __builtin_ctzll(final_at) : 63;  // the nearest tile whose state is final
                int64_t part = (lane <= stop) ? (int64_t)(v & ~SP_ST_MASK) : 0;
                for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o, 64);
                carry += part;
                found = final_at != 0;
            }
        }
        if (lane == 0) {
            if (!final_now)
                __hip_atomic_store(&st[tile], SP_ST_FINAL | (unsigned long long)(carry + tile_s), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            s_carry = carry;
        }
    }
    __syncthreads();
    const int64_t carry = s_carry;
    const int64_t tfd = A.tile_first_doc[tile];
    {
        const int64_t t1 = t0 + SP_TILE;
        for (int64_t d = tfd + tid; d < A.n_docs; d += SP_THREADS) {
            const int64_t i = A.id_offs[d];
            if (i >= t1 || i >= A.n_ids) break;
            if (A.id_offs[d + 1] > i) s_doc[s_rank[i - t0]] = (int32_t)(d - tfd);
        }
    }
    __syncthreads();
    if (i0 >= A.n_ids) return;

    // the thread's tokens, in order
    int64_t U = xf ? (int64_t)xs : carry + (int64_t)xs;  // units of the document in front of the token
    uint32_t r = xc;
    int64_t cur_d = -2, base = 0, dlen = 0, g_doc = 0;
    const int64_t n_starts = BYTE ? 0 : A.rk_chunk[A.n_chunks];
    bool chained = false;      // the running value below continues from the thread's previous token
    int64_t run = 0;           // byte mode: character starts of the document in front of the token; character mode: its byte offset
    int64_t os[SP_PER], oe[SP_PER];
    // the thread has all its SP_PER tokens and the output takes 16-byte stores
    const bool vec = i0 + SP_PER <= A.n_ids && (reinterpret_cast<uintptr_t>(A.out) & 15) == 0;
#pragma unroll
    for (int k = 0; k < SP_PER; k++) {
        os[k] = 0;
        oe[k] = 0;
        if (i0 + k >= A.n_ids) continue;
        const bool first = (firsts >> k) & 1u;
        if (first) {
            U = 0;
            r++;
        }
        const int64_t d = r == 0 ? tfd - 1 : tfd + s_doc[r];
        const uint32_t kind = (kinds >> (2 * k)) & 3u;
        const uint32_t n = units[k];
        if (d < 0 || d >= A.n_docs) {  // (offsets that passed k_sp_check name a document for every id)
            sp_raise(A.err, HUTK_E_ARG);
            U += n;
            continue;
        }
        if (d != cur_d) {
            cur_d = d;
            base = A.doc_offs[d];
            dlen = A.doc_offs[d + 1] - base;
            if (!BYTE) g_doc = sp_rank(A, base);
            chained = false;
        }
        bool good = kind != TOK_BAD;
        int64_t bs = 0, be = 0, cs = 0, ce = 0;
        if (BYTE) {
            bs = U;
            be = U + n;
            if (be > dlen) {  // the ids say more bytes than the document has
                good = false;
                be = be > dlen ? dlen : be;
                bs = bs > dlen ? dlen : bs;
            }
            const uint32_t m = (uint32_t)(be - bs);
            uint32_t starts = 0, lead0 = 0;
            if (kind == TOK_KNOWN && m == n) {
                good = sp_same(T, A, ent[k], base + bs, n, starts) && good;
                if (A.chars && n) lead0 = is_start(A.bytes[base + bs]);
            } else if (m) {  // one unknown byte
                lead0 = starts = is_start(A.bytes[base + bs]);
            }
            if (A.chars) {
                if (first) run = 0;
                else if (!chained) run = sp_rank(A, base + bs) - sp_rank(A, base);
                cs = m ? run + lead0 - 1 : run;
                ce = run + starts;
                run = ce;
            }
        } else {
            cs = U;
            ce = U + n;
            if (first || U == 0) bs = 0;
            else if (chained) bs = run;
            else bs = sp_select<SEARCH>(A, g_doc + U, n_starts) - base;
            be = sp_select<SEARCH>(A, g_doc + U + n, n_starts) - base;
            bs = bs < 0 ? 0 : bs > dlen ? dlen : bs;
            be = be < bs ? bs : be > dlen ? dlen : be;
            const int64_t m = be - bs;
            uint32_t starts = 0;
            if (kind == TOK_KNOWN) {
                good = m == (int64_t)sp_len(ent[k]) && sp_same(T, A, ent[k], base + bs, (uint32_t)m, starts);
            } else if (kind == TOK_UNKNOWN) {
                good = false;
                if (m > 0) {
                    const int64_t rule = utf8_item_len(A.bytes[base + bs]);
                    good = m == (rule < dlen - bs ? rule : dlen - bs);
                }
            }
            run = be;
        }
        chained = true;
        if (!good) {
            sp_raise(A.err, HUTK_E_UNSUPPORTED);
            if (A.status) A.status[d] = HUTK_DOC_SPAN_MISMATCH;
        }
        os[k] = A.chars ? cs : bs;
        oe[k] = A.chars ? ce : be;
        U += n;
        // written as soon as 16 bytes are complete: two tokens of int32 spans, one of int64
        if constexpr (W == 4) {
            if ((k & 1) && vec)
                *reinterpret_cast<int4*>(static_cast<int32_t*>(A.out) + 2 * (i0 + k - 1)) =
                    make_int4((int32_t)os[k - 1], (int32_t)oe[k - 1], (int32_t)os[k], (int32_t)oe[k]);
            else if (!vec) {  // (the output need only be aligned to its element)
                static_cast<int32_t*>(A.out)[2 * (i0 + k)] = (int32_t)os[k];
                static_cast<int32_t*>(A.out)[2 * (i0 + k) + 1] = (int32_t)oe[k];
            }
        } else {
            if (vec) *reinterpret_cast<longlong2*>(static_cast<int64_t*>(A.out) + 2 * (i0 + k)) = make_longlong2(os[k], oe[k]);
            else {
                static_cast<int64_t*>(A.out)[2 * (i0 + k)] = os[k];
                static_cast<int64_t*>(A.out)[2 * (i0 + k) + 1] = oe[k];
            }
        }
    }
}

}  // namespace

int64_t span_tile_ids() { return SP_TILE; }

void launch_spans(const DecTables& t, const SpanArgs& a, int out_width, hipStream_t s) {
    hipLaunchKernelGGL(k_sp_check, dim3((unsigned)((a.n_docs + 255) / 256)), dim3(256), 0, s, a, out_width == 4 ? 1 : 0);
    if (a.n_tiles == 0) return;  // documents without ids: the offsets are checked, nothing is written
    hipLaunchKernelGGL(k_sp_bits, dim3((unsigned)a.n_chunks), dim3(SP_BLOCKS_PER_CHUNK), 0, s, a);
    hipLaunchKernelGGL(k_sp_chunks, dim3(1), dim3(1024), 0, s, a);
    if (!a.byte_mode && a.sel) {
        const unsigned blocks = (unsigned)((a.n_chunks * SP_BLOCKS_PER_CHUNK + 255) / 256);
        if (a.sel_wide) hipLaunchKernelGGL(k_sp_scatter<int64_t>, dim3(blocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_sp_scatter<uint32_t>, dim3(blocks), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_sp_pre, dim3((unsigned)((a.n_tiles + 255) / 256)), dim3(256), 0, s, a);
    const dim3 grid((unsigned)a.n_tiles), block(SP_THREADS);
    if (a.byte_mode) {
        if (out_width == 4) hipLaunchKernelGGL((k_sp_tiles<true, 4>), grid, block, 0, s, t, a);
        else hipLaunchKernelGGL((k_sp_tiles<true, 8>), grid, block, 0, s, t, a);
    } else if (!a.sel) {
        if (out_width == 4) hipLaunchKernelGGL((k_sp_tiles<false, 4, true>), grid, block, 0, s, t, a);
        else hipLaunchKernelGGL((k_sp_tiles<false, 8, true>), grid, block, 0, s, t, a);
    } else {
        if (out_width == 4) hipLaunchKernelGGL((k_sp_tiles<false, 4>), grid, block, 0, s, t, a);
        else hipLaunchKernelGGL((k_sp_tiles<false, 8>), grid, block, 0, s, t, a);
    }
}

}  // namespace hutk

using namespace hutk;

extern "C" {

int hutk_debug_span_tile_ids(void) { return (int)span_tile_ids(); }
int hutk_debug_span_chunk_bytes(void) { return SPAN_CHUNK_BYTES; }

int hutk_token_spans_device(hutk_ctx* c, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                            const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_ids, int unit, int out_width,
                            void* d_spans, int32_t* d_status, int32_t* d_err, void* hip_stream) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to compute spans on");
    if (n_docs < 0 || n_bytes < 0 || n_ids < 0 || n_docs > INT32_MAX - 1 || (out_width != 4 && out_width != 8) ||
        (unit != HUTK_SPANS_BYTES && unit != HUTK_SPANS_CHARS))
        return api_set_error(HUTK_E_ARG, "hutk_token_spans_device: bad arguments");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    // contexts whose tokens do not tile the document, or whose items are not what the span kernels assume
    if (!c->pattern.empty())
        return api_set_error(HUTK_E_UNSUPPORTED, "hutk_token_spans_device: a regex pattern drops the text between its matches; "
                                           "the tokens do not tile the document");
    if (c->tab.has_multi)
        return api_set_error(HUTK_E_UNSUPPORTED, "hutk_token_spans_device: a special-character replacement of several units");
    if (!c->tab.is_byte_encoder)
        for (int b = 0x80; b < 256; b++)
            if (c->tab.item_direct[b])
                return api_set_error(HUTK_E_UNSUPPORTED, "hutk_token_spans_device: a special-character entry for a byte >= 0x80 "
                                                   "without is_byte_encoder");
    // k_sp_tiles adds a tile's units up in 32 bits
    if ((uint64_t)c->dec_max_len * (uint64_t)span_tile_ids() > 0xFFFFFFFFull)
        return api_set_error(HUTK_E_UNSUPPORTED, "hutk_token_spans_device: a token of this vocabulary is too long");
    if (n_docs == 0) {
        if (n_ids != 0) return api_set_error(HUTK_E_ARG, "hutk_token_spans_device: ids without documents");
        HUTK_HIP_TRY(hipSetDevice(c->device));
        if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, 4, hip_stream ? (hipStream_t)hip_stream : c->stream));
        return HUTK_OK;
    }
    // (documents without ids: the offsets are still checked, nothing else is read or written)
    if (!d_offsets || !d_id_offsets || (n_ids > 0 && (!d_ids || !d_spans)) || (n_bytes > 0 && !d_bytes))
        return api_set_error(HUTK_E_ARG, "hutk_token_spans_device: a buffer is NULL");
    HUTK_HIP_TRY(hipSetDevice(c->device));
    const int64_t tile = span_tile_ids();
    const int64_t n_tiles = (n_ids + tile - 1) / tile;
    const int64_t n_chunks = n_bytes / SPAN_CHUNK_BYTES + 1;
    if (n_tiles > 0x7FFFFFFFll || n_chunks > 0x7FFFFFFFll / 256) return api_set_error(HUTK_E_UNSUPPORTED, "hutk_token_spans_device: the batch is too large for one launch");
    const bool byte_mode = c->tab.is_byte_encoder;
    const bool sel_wide = n_bytes > 0xFFFFFFFFll;
    // HUTK_SPANS_SELECT=search: no scattered select array; select searches the rank structure (the slower form)
    const char* sel_form = getenv("HUTK_SPANS_SELECT");
    const bool scatter = !byte_mode && n_ids > 0 && !(sel_form && strcmp(sel_form, "search") == 0);
    HUTK_HIP_TRY(c->dw_first.reserve((size_t)(n_ids / 32 + 4)));
    HUTK_HIP_TRY(c->dw_state.reserve((size_t)n_tiles + 8));
    HUTK_HIP_TRY(c->dw_tfd.reserve((size_t)n_tiles + 1));
    HUTK_HIP_TRY(c->w_err.reserve(1));
    HUTK_HIP_TRY(c->sp_ok.reserve(4));
    HUTK_HIP_TRY(c->sp_bits.reserve((size_t)n_chunks * 256));
    HUTK_HIP_TRY(c->sp_in_chunk.reserve((size_t)n_chunks * 256));
    HUTK_HIP_TRY(c->sp_chunk.reserve((size_t)n_chunks + 1));
    if (scatter) HUTK_HIP_TRY(c->sp_sel.reserve(sel_wide ? (size_t)n_bytes + 1 : (size_t)n_bytes / 2 + 1));
    StreamScope scope(c, hip_stream, false);  // (the device was selected in front of the allocations)
    if (scope.rc) return scope.rc;
    hipStream_t s = scope.s;
    SpanArgs A{};
    A.bytes = d_bytes;
    A.doc_offs = d_offsets;
    A.n_docs = n_docs;
    A.n_bytes = n_bytes;
    A.ids = d_ids;
    A.id_offs = d_id_offsets;
    A.n_ids = n_ids;
    A.n_tiles = n_tiles;
    A.chars = unit == HUTK_SPANS_CHARS;
    A.byte_mode = byte_mode;
    A.out = d_spans;
    A.status = d_status;
    A.err = d_err ? d_err : c->w_err.p;
    A.ok = c->sp_ok.p;
    A.first_bits = c->dw_first.p;
    A.tile_state = c->dw_state.p;
    A.tile_first_doc = c->dw_tfd.p;
    A.rk_bits = c->sp_bits.p;
    A.rk_in_chunk = c->sp_in_chunk.p;
    A.rk_chunk = c->sp_chunk.p;
    A.n_chunks = n_chunks;
    A.sel = scatter ? c->sp_sel.p : nullptr;
    A.sel_wide = sel_wide;
    A.help_after = getenv("HUTK_SPANS_HELP_AFTER") ? (uint32_t)atol(getenv("HUTK_SPANS_HELP_AFTER")) : (1u << 14);  // (0: tests of the fallback)
    HUTK_HIP_TRY(hipMemsetAsync(A.err, 0, 4, s));
    HUTK_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)A.ok, 1, 1, s));
    HUTK_HIP_TRY(hipMemsetAsync(A.first_bits, 0, (size_t)(n_ids / 32 + 4) * 4, s));
    if (n_tiles) HUTK_HIP_TRY(hipMemsetAsync(A.tile_state, 0, (size_t)n_tiles * 8, s));
    if (d_status) HUTK_HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n_docs * 4, s));
    launch_spans(c->dec, A, out_width, s);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_token_spans(hutk_ctx* c, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, const int32_t* ids,
                     const int64_t* id_offsets, int unit, int out_width, void* spans, int32_t* status) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to compute spans on");
    if (n_docs < 0 || !offsets || !id_offsets || (out_width != 4 && out_width != 8))
        return api_set_error(HUTK_E_ARG, "hutk_token_spans: bad arguments");
    if (offsets[0] < 0 || id_offsets[0] != 0) return api_set_error(HUTK_E_ARG, "offsets[0] must not be negative, id_offsets[0] must be 0");
    if (int rc = check_offsets(offsets, n_docs, false, "offsets")) return rc;
    if (int rc = check_offsets(id_offsets, n_docs, false, "offsets")) return rc;  // (one text for both arrays)
    const int64_t n_bytes = offsets[n_docs], n_ids = id_offsets[n_docs];
    if ((n_bytes > 0 && !bytes) || (n_ids > 0 && (!ids || !spans))) return api_set_error(HUTK_E_ARG, "hutk_token_spans: a buffer is NULL");
    HUTK_HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HUTK_HIP_TRY(c->s_bytes.reserve((size_t)n_bytes + 16));
    HUTK_HIP_TRY(c->s_offsets.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->ds_ids.reserve((size_t)n_ids + 16));
    HUTK_HIP_TRY(c->ds_offs.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->ds_status.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->ss_spans.reserve((size_t)n_ids * 2 + 2));
    HUTK_HIP_TRY(c->w_err.reserve(1));
    if (n_bytes) HUTK_HIP_TRY(hipMemcpyAsync(c->s_bytes.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    if (n_ids) HUTK_HIP_TRY(hipMemcpyAsync(c->ds_ids.p, ids, (size_t)n_ids * 4, hipMemcpyHostToDevice, s));
    HUTK_HIP_TRY(hipMemcpyAsync(c->s_offsets.p, offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    HUTK_HIP_TRY(hipMemcpyAsync(c->ds_offs.p, id_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    int rc = hutk_token_spans_device(c, c->s_bytes.p, c->s_offsets.p, n_docs, n_bytes, c->ds_ids.p, c->ds_offs.p, n_ids, unit,
                                     out_width, c->ss_spans.p, c->ds_status.p, c->w_err.p, s);
    if (rc) return rc;
    int32_t err = 0;
    HUTK_HIP_TRY(hipMemcpyAsync(&err, c->w_err.p, 4, hipMemcpyDeviceToHost, s));
    if (n_ids) HUTK_HIP_TRY(hipMemcpyAsync(spans, c->ss_spans.p, (size_t)n_ids * 2 * out_width, hipMemcpyDeviceToHost, s));
    if (status && n_docs) HUTK_HIP_TRY(hipMemcpyAsync(status, c->ds_status.p, (size_t)n_docs * 4, hipMemcpyDeviceToHost, s));
    HUTK_HIP_TRY(hipStreamSynchronize(s));
    return err == HUTK_OK ? HUTK_OK : api_set_error(err, device_error_message(Direction::Spans, err));
}

}  // extern "C"
