// hutk_fallback.hip -- byte fallback: an item the vocabulary does not hold is encoded as the ids of its bytes (the 256
// lines "<0x00>".."<0xFF>" of a SentencePiece-shaped vocabulary), and such an id decodes to its one raw byte
// (include/hutoken_amd.h).
//
// Encode.  The plain encode (hutk_api.cpp, encode_device_impl) writes into a workspace; the span kernels of
// hutk_spans.hip (launch_spans, byte unit, 32-bit) say which bytes every id covers; the expansion here replaces every -1
// by the table's ids of the bytes of its span.  The host never learns how many ids the encode wrote (the call does not
// synchronise), so the spans run over the workspace's CAPACITY: the ids behind the last document are one more document,
// of no bytes, whose spans and status nobody reads.
//   k_fb_pad      one thread: the number of ids (-1: the encode failed), the extra document's offsets
//   k_fb_tiles    tiles of FB_TILE ids, twice: <false> counts the ids every tile becomes; k_scan_i64 (hutk_special.hip)
//                 makes them tile bases; <true> writes ids and out_offsets.  No workgroup waits for another one.
// Decode.  k_fb_remap: k_dsp_remap (hutk_special.hip) and the table's ids, in front of the decode kernels of
// hutk_decode.hip, which run unchanged over tables that fallback_rebuild_decode extended by 256 one-byte entries.
//
// The C entry points are at the end of the file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "hutk_host.h"

namespace hutk {

namespace {

constexpr int FB_THREADS = 256, FB_PER = 8, FB_TILE = FB_THREADS * FB_PER;  // ids per workgroup of the expansion
static_assert(FB_PER % 4 == 0 && 32 % FB_PER == 0, "16-byte id loads; a thread's first-token bits sit in one word");
constexpr int FB_MAX_ITEM = 4;  // bytes of the longest item: a four-byte character

struct FbArgs {
    const uint8_t* bytes;
    const int64_t* doc_offs;        // [n_docs + 2] the caller's, and the extra document's end
    int64_t n_docs;                 // the caller's
    const int32_t* ids;             // the plain encode's
    const int64_t* id_offs;         // [n_docs + 2]
    const int32_t* spans;           // [capacity][2] byte spans
    const int32_t* span_status;     // [n_docs + 1]
    const int32_t* ok;              // the spans' verdict on the offsets
    const uint32_t* first_bits;     // of the spans: bit i: id i is the first of a document
    const int64_t* tile_first_doc;  // of the spans: first document whose first id is at or after the tile's
    const int32_t* table;           // [256]
    const int64_t* hdr;             // [0]: the number of ids, -1: the plain encode failed
    int64_t* tile_base;             // [n_tiles + 1] ids a tile becomes, then in front of it
    int32_t* out_ids;
    int64_t ids_cap;
    int64_t* out_offsets;
    int32_t* err;
};

// (an error outranks the note HUTK_E_WORD_TOO_LARGE that the encode may have left)
__device__ __forceinline__ void fb_raise(int32_t* err, int32_t code) {
    if (atomicCAS(err, 0, code) == HUTK_E_WORD_TOO_LARGE) atomicCAS(err, HUTK_E_WORD_TOO_LARGE, code);
}

// inclusive prefix sum over the 64 lanes of a wavefront (DPP row shifts and broadcasts, as k_dec_tiles')
__device__ __forceinline__ uint32_t fb_wave_incl(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
// exclusive scan over the workgroup; total: the sum.  s_part: one value per wavefront, free again after the call
__device__ __forceinline__ uint32_t fb_block_excl(uint32_t v, uint32_t* s_part, uint32_t& total) {
    const int tid = threadIdx.x;
    const uint32_t incl = fb_wave_incl(v);
    if ((tid & 63) == 63) s_part[tid >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - v;
    total = 0;
#pragma unroll
    for (int u = 0; u < FB_THREADS / 64; u++) {
        const uint32_t t = s_part[u];
        if (u < (tid >> 6)) before += t;
        total += t;
    }
    __syncthreads();
    return before;
}

__global__ void k_fb_pad(int64_t* id_offs, int64_t* doc_offs, int64_t n_docs, int64_t cap, const int32_t* err, int64_t* hdr) {
    const int32_t e = *err;
    const int64_t n = id_offs[n_docs];
    hdr[0] = ((e != HUTK_OK && e != HUTK_E_WORD_TOO_LARGE) || n < 0 || n >= cap) ? -1 : n;
    id_offs[n_docs + 1] = cap;
    doc_offs[n_docs + 1] = doc_offs[n_docs];
}

// WRITE = false: tile_base[tile] = the ids the tile's ids become.  WRITE = true: tile_base holds the scan; the ids, and
// out_offsets of every document whose first id is in the tile -- empty ones and, where the last id is, those behind it
// and out_offsets[n_docs] included (the tile at n_ids has no ids when n_ids is a multiple of FB_TILE: it still runs).
template <bool WRITE>
__global__ __launch_bounds__(FB_THREADS) void k_fb_tiles(FbArgs A) {
    __shared__ uint16_t s_rank[FB_TILE];    // document starts in the tile up to and including each id
    __shared__ int32_t s_doc[FB_TILE + 1];  // the r-th document that starts in the tile, counted from tile_first_doc
    __shared__ uint16_t s_pos[WRITE ? FB_TILE : 1];  // ids of the tile's output in front of each id
    __shared__ int32_t s_tab[WRITE ? 256 : 1];
    __shared__ uint32_t s_part[FB_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t t0 = tile * FB_TILE, t1 = t0 + FB_TILE;
    const int64_t n_ids = A.hdr[0];
    const bool ok = *A.ok != 0;
    if (n_ids < 0 || !ok || t0 > n_ids) {  // a failed encode, offsets the spans refused, a tile behind the ids
        if (!WRITE && tid == 0) A.tile_base[tile] = 0;
        if (WRITE && tile == 0 && tid == 0 && n_ids >= 0 && !ok) fb_raise(A.err, HUTK_E_ARG);
        return;
    }
    if (WRITE) s_tab[tid] = A.table[tid];
    const int64_t i0 = t0 + (int64_t)tid * FB_PER;
    const int valid = i0 >= n_ids ? 0 : (n_ids - i0 < FB_PER ? (int)(n_ids - i0) : FB_PER);
    uint32_t firsts = 0;  // bit k: id i0 + k starts a document
    if (valid) firsts = (A.first_bits[i0 >> 5] >> (i0 & 31)) & ((1u << valid) - 1u);
    int32_t id[FB_PER], sp[2 * FB_PER];
    if (valid == FB_PER) {  // (the workspace is 16-byte aligned) two 16-byte loads of ids, four of spans
#pragma unroll
        for (int g = 0; g < FB_PER; g += 4) {
            const int4 a = *reinterpret_cast<const int4*>(A.ids + i0 + g);
            id[g] = a.x; id[g + 1] = a.y; id[g + 2] = a.z; id[g + 3] = a.w;
        }
#pragma unroll
        for (int g = 0; g < 2 * FB_PER; g += 4) {
            const int4 a = *reinterpret_cast<const int4*>(A.spans + 2 * i0 + g);
            sp[g] = a.x; sp[g + 1] = a.y; sp[g + 2] = a.z; sp[g + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < FB_PER; k++) {
            id[k] = k < valid ? A.ids[i0 + k] : 0;
            sp[2 * k] = k < valid ? A.spans[2 * (i0 + k)] : 0;
            sp[2 * k + 1] = k < valid ? A.spans[2 * (i0 + k) + 1] : 0;
        }
    }
    // An unknown item's count needs its document's status: the tile's documents listed in LDS, as k_sp_tiles does.
    uint32_t unknown = 0;  // bit k: id i0 + k is -1 and its span is an item's
#pragma unroll
    for (int k = 0; k < FB_PER; k++) {
        const int32_t len = sp[2 * k + 1] - sp[2 * k];
        if (k < valid && id[k] == -1 && len >= 1 && len <= FB_MAX_ITEM) unknown |= 1u << k;
    }
    const int64_t tfd = A.tile_first_doc[tile];
    uint32_t starts_total;
    const uint32_t xc = fb_block_excl((uint32_t)__popc(firsts), s_part, starts_total);
    if (__syncthreads_or(unknown != 0)) {
        uint32_t r = xc;
#pragma unroll
        for (int k = 0; k < FB_PER; k++) {
            r += (firsts >> k) & 1u;
            s_rank[tid * FB_PER + k] = (uint16_t)r;
        }
        __syncthreads();
        for (int64_t d = tfd + tid; d < A.n_docs; d += FB_THREADS) {
            const int64_t i = A.id_offs[d];
            if (i >= t1 || i >= n_ids) break;
            if (A.id_offs[d + 1] > i) s_doc[s_rank[i - t0]] = (int32_t)(d - tfd);
        }
        __syncthreads();
    }
    int64_t base[FB_PER];  // of a clean unknown item: where its bytes are
    uint32_t cnt[FB_PER], mine = 0;
    {
        uint32_t r = xc;
        int64_t cur_d = -2, cur_base = 0, cur_len = 0;
        bool cur_clean = false;
#pragma unroll
        for (int k = 0; k < FB_PER; k++) {
            r += (firsts >> k) & 1u;
            cnt[k] = k < valid ? 1u : 0u;
            base[k] = -1;
            if ((unknown >> k) & 1u) {
                const int64_t d = r == 0 ? tfd - 1 : tfd + s_doc[r];
                if (d != cur_d) {
                    cur_d = d;
                    cur_clean = d >= 0 && d < A.n_docs && A.span_status[d] == 0;  // (checked offsets name a document for every id)
                    if (cur_clean) {
                        cur_base = A.doc_offs[d];
                        cur_len = A.doc_offs[d + 1] - cur_base;
                    }
                }
                if (cur_clean && sp[2 * k] >= 0 && sp[2 * k + 1] <= cur_len) {  // (k_sp_tiles clips its spans: always)
                    cnt[k] = (uint32_t)(sp[2 * k + 1] - sp[2 * k]);
                    base[k] = cur_base + sp[2 * k];
                }
            }
            mine += cnt[k];
        }
    }
    uint32_t total;
    const uint32_t before = fb_block_excl(mine, s_part, total);
    if (!WRITE) {
        if (tid == 0) A.tile_base[tile] = total;
        return;
    }
    const int64_t g0 = A.tile_base[tile];
    {
        uint32_t pos = before;
#pragma unroll
        for (int k = 0; k < FB_PER; k++) {
            s_pos[tid * FB_PER + k] = (uint16_t)pos;  // (at most FB_TILE * FB_MAX_ITEM; behind the last id: the total)
            pos += cnt[k];
        }
    }
    __syncthreads();
    for (int64_t d = tfd + tid; d <= A.n_docs; d += FB_THREADS) {
        const int64_t i = A.id_offs[d];
        if (i >= t1) break;
        A.out_offsets[d] = g0 + s_pos[i - t0];
        if (d < A.n_docs && A.span_status[d] != 0) fb_raise(A.err, HUTK_E_UNSUPPORTED);  // the document keeps its plain ids
    }
    if (g0 + (int64_t)total > A.ids_cap) {  // (cannot happen: the capacity is a bound and the call checked ids_cap)
        if (tid == 0) fb_raise(A.err, HUTK_E_CAPACITY);
        return;
    }
    int32_t* out = A.out_ids + g0 + before;
#pragma unroll
    for (int k = 0; k < FB_PER; k++) {
        if (base[k] < 0) {
            if (k < valid) *out = id[k];
        } else {
            const uint8_t* text = A.bytes + base[k];
            for (uint32_t j = 0; j < cnt[k]; j++) out[j] = s_tab[text[j]];
        }
        out += cnt[k];
    }
}

// ---- decode: table ids become the one-byte entries behind the vocabulary's and the specials' ---------------------
constexpr int FBR_THREADS = 256, FBR_PER = 4, FBR_TILE = FBR_THREADS * FBR_PER;  // ids per workgroup of the pass

__device__ __forceinline__ int32_t fb_index(const DecFallback& F, int32_t id) {  // the byte of a table id, -1: not one
    if (id < F.id_min || id > F.id_max) return -1;
    for (uint32_t s = fb_slot((uint32_t)id);; s = (s + 1) & (FB_SLOTS - 1)) {  // (a quarter full: it ends)
        const uint2 e = F.slots[s];
        if (e.y == DSP_EMPTY) return -1;
        if ((int32_t)e.x == id) return (int32_t)e.y;
    }
}

// k_dsp_remap with one more case, asked first: out[i] = F.base + b for the table's id of byte b.  Such an id is no
// marker: it sets no first-token bit behind it, and the walk of DSP_BITS_SKIP ends on it like on any ordinary id (an id
// is never both: the call refuses such a table).  Without HUTK_FB_SPECIAL S holds no id.
__global__ __launch_bounds__(FBR_THREADS) void k_fb_remap(DecSpecial S, DecFallback F, const int32_t* ids, int32_t* out,
                                                          int64_t n_ids, uint32_t* first_bits) {
    const int64_t i0 = ((int64_t)blockIdx.x * FBR_THREADS + threadIdx.x) * FBR_PER;
    if (i0 >= n_ids) return;
    const bool full = i0 + FBR_PER <= n_ids;
    int32_t id[FBR_PER];
    if (full && (reinterpret_cast<uintptr_t>(ids) & 15) == 0) {
        const int4 a = *reinterpret_cast<const int4*>(ids + i0);
        id[0] = a.x; id[1] = a.y; id[2] = a.z; id[3] = a.w;
    } else {
#pragma unroll
        for (int k = 0; k < FBR_PER; k++) id[k] = (i0 + k < n_ids) ? ids[i0 + k] : 0;
    }
    int32_t v[FBR_PER];
#pragma unroll
    for (int k = 0; k < FBR_PER; k++) {
        const int64_t i = i0 + k;
        v[k] = id[k] >= S.n_vocab ? -1 : id[k];
        if (i >= n_ids) continue;
        const int32_t b = fb_index(F, id[k]);
        if (b >= 0) {
            v[k] = F.base + b;
            continue;
        }
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
        for (int k = 0; k < FBR_PER; k++)
            if (i0 + k < n_ids) out[i0 + k] = v[k];
    }
}

// what the spans refuse (hutk_token_spans_device), and a context without a table
int fb_refusal(const hutk_ctx* c, const char* who) {
    const std::string w(who);
    if (!c->fb.on) return api_set_error(HUTK_E_UNSUPPORTED, w + ": no byte-fallback table is installed (hutk_ctx_set_byte_fallback)");
    if (!c->pattern.empty()) return api_set_error(HUTK_E_UNSUPPORTED, w + ": a regex pattern drops the text between its matches; the tokens do not tile the document");
    if (c->presplit >= 0) return api_set_error(HUTK_E_UNSUPPORTED, w + ": a split preset is installed: a byte-level vocabulary holds all 256 bytes, there is nothing to fall back to");
    if (c->tab.has_multi) return api_set_error(HUTK_E_UNSUPPORTED, w + ": a special-character replacement of several units");
    if (!c->tab.is_byte_encoder)
        for (int b = 0x80; b < 256; b++)
            if (c->tab.item_direct[b])
                return api_set_error(HUTK_E_UNSUPPORTED, w + ": a special-character entry for a byte >= 0x80 without is_byte_encoder");
    if ((uint64_t)c->dec_max_len * (uint64_t)span_tile_ids() > 0xFFFFFFFFull)
        return api_set_error(HUTK_E_UNSUPPORTED, w + ": a token of this vocabulary is too long");
    return HUTK_OK;
}

}  // namespace

void launch_fb_remap(const DecSpecial& sp, const DecFallback& fb, const int32_t* ids, int32_t* ids_out, int64_t n_ids,
                     uint32_t* first_bits, hipStream_t s) {
    hipLaunchKernelGGL(k_fb_remap, dim3((unsigned)((n_ids + FBR_TILE - 1) / FBR_TILE)), dim3(FBR_THREADS), 0, s, sp, fb, ids,
                       ids_out, n_ids, first_bits);
}

int fallback_rebuild_decode(hutk_ctx* c) {
    hutk_ctx::Fallback& F = c->fb;
    if (!F.on) return HUTK_OK;
    const hutk_ctx::Specials& S = c->sx;
    F.clash = false;
    for (int b = 0; b < 256 && S.n; b++)
        F.clash = F.clash || std::find(S.ids.begin(), S.ids.end(), F.ids[b]) != S.ids.end();
    if (c->host_only) return HUTK_OK;
    DecExt::Host X;  // behind the entries of the special ids, when a set is installed
    std::vector<std::pair<const uint8_t*, uint32_t>> extra;
    extra.reserve(256);
    uint8_t byte[256];
    for (int b = 0; b < 256; b++) byte[b] = (uint8_t)b, extra.emplace_back(&byte[b], 1u);
    if (int rc = dec_ext_build(c->tab, S.n ? &S.dec : nullptr, extra, false,
                               "byte fallback: the vocabulary leaves no ids for the decode tables", X))
        return rc;
    F.base = c->tab.dec_n + X.n_extra - 256;
    X.slots.assign(FB_SLOTS, make_uint2(0, DSP_EMPTY));
    F.id_min = INT32_MAX;
    F.id_max = 0;
    for (int b = 0; b < 256; b++) {
        uint32_t s = fb_slot((uint32_t)F.ids[b]);
        while (X.slots[s].y != DSP_EMPTY) s = (s + 1) & (FB_SLOTS - 1);
        X.slots[s] = make_uint2((uint32_t)F.ids[b], (uint32_t)b);
        F.id_min = std::min(F.id_min, F.ids[b]);
        F.id_max = std::max(F.id_max, F.ids[b]);
    }
    HUTK_HIP_TRY(hipSetDevice(c->device));
    HUTK_HIP_TRY(hipDeviceSynchronize());  // an earlier asynchronous call may still read the tables
    if (int rc = F.dec.upload(X)) return rc;
    HUTK_HIP_TRY(F.d_tab.reserve(256));
    HUTK_HIP_TRY(hipMemcpy(F.d_tab.p, F.ids, sizeof F.ids, hipMemcpyHostToDevice));
    return HUTK_OK;
}

int encode_fallback_device_impl(hutk_ctx* c, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                                int32_t* d_ids_out, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_status, int32_t* d_err,
                                void* hip_stream) {
    if (n_docs == 0)  // nothing to expand: the plain encode writes the one offset
        return encode_device_impl(c, d_bytes, d_offsets, n_docs, n_bytes, d_ids_out, ids_cap, d_out_offsets, d_status, d_err,
                                  hip_stream, nullptr, nullptr);
    if (n_docs < 0 || n_bytes < 0 || !d_offsets || !d_out_offsets || (n_bytes > 0 && (!d_bytes || !d_ids_out)))
        return api_set_error(HUTK_E_ARG, "bad argument");
    if (n_docs > (int64_t)INT32_MAX - 2) return api_set_error(HUTK_E_ARG, "byte fallback: too many documents for one call");
    const int64_t cap = hutk_ids_capacity(c, n_bytes, n_docs);  // the bound + 1: the encode writes fewer ids than this
    if (ids_cap < cap - 1) return api_set_error(HUTK_E_CAPACITY, "ids_cap is below hutk_ids_capacity()");
    if (span_tile_ids() != FB_TILE) return api_set_error(HUTK_E_DEVICE, "byte fallback: the spans' tiles are not the expansion's");
    hutk_ctx::Fallback& F = c->fb;
    const int64_t n_tiles = (cap + FB_TILE - 1) / FB_TILE;
    const int64_t n_chunks = n_bytes / SPAN_CHUNK_BYTES + 1;
    if (n_tiles > 0x7FFFFFFFll || n_chunks > 0x7FFFFFFFll / 256) return api_set_error(HUTK_E_UNSUPPORTED, "byte fallback: the batch is too large for one launch");
    const bool byte_mode = c->tab.is_byte_encoder;
    const bool sel_wide = n_bytes > 0xFFFFFFFFll;
    const char* sel_form = getenv("HUTK_SPANS_SELECT");
    const bool scatter = !byte_mode && !(sel_form && strcmp(sel_form, "search") == 0);
    HUTK_HIP_TRY(hipSetDevice(c->device));
    HUTK_HIP_TRY(F.w_ids.reserve((size_t)cap + 16));
    HUTK_HIP_TRY(F.w_oo.reserve((size_t)n_docs + 2));
    HUTK_HIP_TRY(F.w_doff.reserve((size_t)n_docs + 2));
    HUTK_HIP_TRY(F.w_spans.reserve((size_t)cap * 2 + 16));
    HUTK_HIP_TRY(F.w_sstatus.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(F.w_serr.reserve(1));
    HUTK_HIP_TRY(F.w_tile.reserve((size_t)n_tiles + 1));
    HUTK_HIP_TRY(F.w_hdr.reserve(2));
    HUTK_HIP_TRY(c->dw_first.reserve((size_t)(cap / 32 + 4)));
    HUTK_HIP_TRY(c->dw_state.reserve((size_t)n_tiles + 8));
    HUTK_HIP_TRY(c->dw_tfd.reserve((size_t)n_tiles + 1));
    HUTK_HIP_TRY(c->w_err.reserve(1));
    HUTK_HIP_TRY(c->sp_ok.reserve(4));
    HUTK_HIP_TRY(c->sp_bits.reserve((size_t)n_chunks * 256));
    HUTK_HIP_TRY(c->sp_in_chunk.reserve((size_t)n_chunks * 256));
    HUTK_HIP_TRY(c->sp_chunk.reserve((size_t)n_chunks + 1));
    if (scatter) HUTK_HIP_TRY(c->sp_sel.reserve(sel_wide ? (size_t)n_bytes + 1 : (size_t)n_bytes / 2 + 1));
    int32_t* const err = d_err ? d_err : c->w_err.p;
    if (int rc = encode_device_impl(c, d_bytes, d_offsets, n_docs, n_bytes, F.w_ids.p, cap, F.w_oo.p, d_status, err, hip_stream,
                                    nullptr, nullptr))
        return rc;
    StreamScope scope(c, hip_stream, false);  // (the device was selected in front of the allocations)
    if (scope.rc) return scope.rc;
    hipStream_t s = scope.s;
    HUTK_HIP_TRY(hipMemcpyAsync(F.w_doff.p, d_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_fb_pad, dim3(1), dim3(1), 0, s, F.w_oo.p, F.w_doff.p, n_docs, cap, err, F.w_hdr.p);
    SpanArgs A{};
    A.bytes = d_bytes;
    A.doc_offs = F.w_doff.p;
    A.n_docs = n_docs + 1;
    A.n_bytes = n_bytes;
    A.ids = F.w_ids.p;
    A.id_offs = F.w_oo.p;
    A.n_ids = cap;
    A.n_tiles = n_tiles;
    A.chars = 0;
    A.byte_mode = byte_mode;
    A.out = F.w_spans.p;
    A.status = F.w_sstatus.p;
    A.err = F.w_serr.p;  // (the extra document's ids are nobody's text: its mismatch must not reach the caller's word)
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
    A.help_after = getenv("HUTK_SPANS_HELP_AFTER") ? (uint32_t)atol(getenv("HUTK_SPANS_HELP_AFTER")) : (1u << 14);
    HUTK_HIP_TRY(hipMemsetAsync(A.err, 0, 4, s));
    HUTK_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)A.ok, 1, 1, s));
    HUTK_HIP_TRY(hipMemsetAsync(A.first_bits, 0, (size_t)(cap / 32 + 4) * 4, s));
    HUTK_HIP_TRY(hipMemsetAsync(A.tile_state, 0, (size_t)n_tiles * 8, s));
    HUTK_HIP_TRY(hipMemsetAsync(A.status, 0, (size_t)(n_docs + 1) * 4, s));
    launch_spans(c->dec, A, 4, s);
    FbArgs X{};
    X.bytes = d_bytes;
    X.doc_offs = F.w_doff.p;
    X.n_docs = n_docs;
    X.ids = F.w_ids.p;
    X.id_offs = F.w_oo.p;
    X.spans = F.w_spans.p;
    X.span_status = F.w_sstatus.p;
    X.ok = c->sp_ok.p;
    X.first_bits = c->dw_first.p;
    X.tile_first_doc = c->dw_tfd.p;
    X.table = F.d_tab.p;
    X.hdr = F.w_hdr.p;
    X.tile_base = F.w_tile.p;
    X.out_ids = d_ids_out;
    X.ids_cap = ids_cap;
    X.out_offsets = d_out_offsets;
    X.err = err;
    hipLaunchKernelGGL(k_fb_tiles<false>, dim3((unsigned)n_tiles), dim3(FB_THREADS), 0, s, X);
    launch_scan_i64(F.w_tile.p, n_tiles, s);
    hipLaunchKernelGGL(k_fb_tiles<true>, dim3((unsigned)n_tiles), dim3(FB_THREADS), 0, s, X);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

}  // namespace hutk

using namespace hutk;

extern "C" {

int hutk_ctx_find_byte_tokens(const hutk_ctx* c, int32_t out256[256]) {
    if (!c || !out256) return 0;
    int found = 0;
    for (int b = 0; b < 256; b++) found += (out256[b] = c->tab.byte_tok[b]) >= 0;
    return found;
}

int hutk_ctx_set_byte_fallback(hutk_ctx* c, const int32_t* ids256) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    hutk_ctx::Fallback& F = c->fb;
    if (!ids256) {
        F.on = false;
        return HUTK_OK;
    }
    int32_t sorted[256];
    memcpy(sorted, ids256, sizeof sorted);
    std::sort(sorted, sorted + 256);
    if (sorted[0] < 0) return api_set_error(HUTK_E_VALUE, "byte fallback: an id must not be negative");
    if (std::adjacent_find(sorted, sorted + 256) != sorted + 256) return api_set_error(HUTK_E_VALUE, "byte fallback: two bytes have the same id");
    memcpy(F.ids, ids256, sizeof F.ids);
    F.on = true;
    const int rc = fallback_rebuild_decode(c);
    if (rc) F.on = false;  // (a device failure: the device arrays may be half replaced, no table is in force)
    return rc;
}

int hutk_ctx_byte_fallback(const hutk_ctx* c, int32_t* out256) {
    if (!c || !c->fb.on) return 0;
    if (out256) memcpy(out256, c->fb.ids, sizeof c->fb.ids);
    return 1;
}

int hutk_encode_fallback_batch_device(hutk_ctx* c, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                      int64_t n_bytes, int flags, int32_t* d_ids_out, int64_t ids_cap, int64_t* d_out_offsets,
                                      int32_t* d_status, int32_t* d_err, void* hip_stream) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (flags & ~HUTK_FB_SPECIAL) return api_set_error(HUTK_E_ARG, "hutk_encode_fallback_batch_device: unknown flags");
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to encode on");
    if (n_docs < 0 || n_bytes < 0 || !d_offsets || !d_out_offsets || (n_bytes > 0 && (!d_bytes || !d_ids_out)))
        return api_set_error(HUTK_E_ARG, "hutk_encode_fallback_batch_device: bad arguments");
    if (((uintptr_t)d_bytes & 15u) != 0) return api_set_error(HUTK_E_ARG, "d_bytes must be 16-byte aligned");
    std::lock_guard<std::recursive_mutex> lock(c->mu);  // held once around the whole call: encode, spans, expansion
    if (int rc = fb_refusal(c, "hutk_encode_fallback_batch_device")) return rc;
    if (flags & HUTK_FB_SPECIAL) {
        if (c->sx.n && c->fb.clash)
            return api_set_error(HUTK_E_VALUE, "hutk_encode_fallback_batch_device: an id is both a special token's and the byte-fallback table's");
        return encode_special_impl(c, true, d_bytes, d_offsets, n_docs, n_bytes, d_ids_out, ids_cap, d_out_offsets, d_status, d_err,
                                   hip_stream);
    }
    return encode_fallback_device_impl(c, d_bytes, d_offsets, n_docs, n_bytes, d_ids_out, ids_cap, d_out_offsets, d_status, d_err,
                                       hip_stream);
}

int hutk_encode_fallback_batch(hutk_ctx* c, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, int flags,
                               int32_t* ids_out, int64_t ids_cap, int64_t* out_offsets, int32_t* status) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (flags & ~HUTK_FB_SPECIAL) return api_set_error(HUTK_E_ARG, "hutk_encode_fallback_batch: unknown flags");
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to encode on");
    if (n_docs < 0 || !offsets || !out_offsets) return api_set_error(HUTK_E_ARG, "hutk_encode_fallback_batch: bad arguments");
    if (int rc = check_offsets(offsets, n_docs, true, "offsets")) return rc;
    const int64_t n_bytes = offsets[n_docs];
    if (n_bytes > 0 && (!bytes || !ids_out)) return api_set_error(HUTK_E_ARG, "hutk_encode_fallback_batch: a buffer is NULL");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    const int64_t cap = (flags & HUTK_FB_SPECIAL) ? hutk_special_ids_capacity(c, n_bytes, n_docs) : hutk_ids_capacity(c, n_bytes, n_docs);
    if (ids_cap < cap - 1) return api_set_error(HUTK_E_CAPACITY, "ids_cap is below the capacity of the batch");
    const auto device = [&](const uint8_t* d_bytes, const int64_t* d_offs, int32_t* d_ids, int64_t* d_oo, int32_t* d_status,
                            int32_t* d_err, hipStream_t s) {
        return hutk_encode_fallback_batch_device(c, d_bytes, d_offs, n_docs, n_bytes, flags, d_ids, cap, d_oo, d_status, d_err, s);
    };
    const auto refuse = [](int err) {
        if (err == HUTK_E_UNSUPPORTED) {  // documents whose spans did not verify kept their plain ids: the rest is exact
            api_set_error(err, "a document's text does not hold the decoded bytes of its tokens where their spans lie: it keeps its plain ids");
            return false;
        }
        api_set_error(err, err == HUTK_E_ARG ? "offsets that do not describe the text, or a document of 2^31 bytes or more"
                                             : device_error_message(Direction::Encode, err));
        return true;
    };
    return encode_host_impl(c, "hutk_encode_fallback_batch", cap, device, refuse, bytes, offsets, n_docs, n_bytes, ids_out, ids_cap,
                            out_offsets, status);
}

int hutk_decode_fallback_batch_device(hutk_ctx* c, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_docs,
                                      int64_t n_ids, int flags, uint8_t* d_bytes_out, int64_t bytes_cap, int64_t* d_out_offsets,
                                      int32_t* d_status, int32_t* d_err, void* hip_stream) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (flags & ~(HUTK_FB_SPECIAL | HUTK_FB_SKIP_SPECIAL)) return api_set_error(HUTK_E_ARG, "hutk_decode_fallback_batch_device: unknown flags");
    if ((flags & HUTK_FB_SKIP_SPECIAL) && !(flags & HUTK_FB_SPECIAL))
        return api_set_error(HUTK_E_ARG, "hutk_decode_fallback_batch_device: HUTK_FB_SKIP_SPECIAL needs HUTK_FB_SPECIAL");
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to decode on");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    const hutk_ctx::Fallback& F = c->fb;
    const hutk_ctx::Specials& S = c->sx;
    if (!F.on) return api_set_error(HUTK_E_UNSUPPORTED, "hutk_decode_fallback_batch_device: no byte-fallback table is installed (hutk_ctx_set_byte_fallback)");
    const bool special = (flags & HUTK_FB_SPECIAL) && S.n > 0;
    if (special && F.clash)
        return api_set_error(HUTK_E_VALUE, "hutk_decode_fallback_batch_device: an id is both a special token's and the byte-fallback table's");
    const bool skip = (flags & HUTK_FB_SKIP_SPECIAL) != 0;
    DecSpecial P{};
    P.slots = special ? c->sxd.dec.dx_slots.p : nullptr;
    P.id_min = special ? S.dec.id_min : 1;  // (without the set no id is in [1, 0])
    P.id_max = special ? S.dec.id_max : 0;
    P.n_vocab = (int32_t)c->dec.n;
    P.bits = (!F.dec.strip || !special) ? DSP_BITS_NONE : skip ? DSP_BITS_SKIP : DSP_BITS_AFTER;
    DecFallback B{};
    B.slots = F.dec.dx_slots.p;
    B.id_min = F.id_min;
    B.id_max = F.id_max;
    B.base = (int32_t)F.base;
    return decode_device_impl(c, F.dec.tables(skip), &P, d_ids, d_id_offsets, n_docs, n_ids, d_bytes_out, bytes_cap, d_out_offsets,
                              d_status, d_err, hip_stream, &B);
}

int hutk_decode_fallback_batch(hutk_ctx* c, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, int flags,
                               uint8_t* bytes_out, int64_t bytes_cap, int64_t* out_offsets, int32_t* status) {
    if (!c) return api_set_error(HUTK_E_ARG, "ctx is NULL");
    if (flags & ~(HUTK_FB_SPECIAL | HUTK_FB_SKIP_SPECIAL)) return api_set_error(HUTK_E_ARG, "hutk_decode_fallback_batch: unknown flags");
    if ((flags & HUTK_FB_SKIP_SPECIAL) && !(flags & HUTK_FB_SPECIAL))
        return api_set_error(HUTK_E_ARG, "hutk_decode_fallback_batch: HUTK_FB_SKIP_SPECIAL needs HUTK_FB_SPECIAL");
    const auto device = [&](const int32_t* d_ids, const int64_t* d_offs, int64_t n_ids, uint8_t* d_bytes, int64_t* d_oo,
                            int32_t* d_status, int32_t* d_err, hipStream_t s) {
        return hutk_decode_fallback_batch_device(c, d_ids, d_offs, n_docs, n_ids, flags, d_bytes, bytes_cap, d_oo, d_status, d_err, s);
    };
    return decode_host_impl(c, device, ids, id_offsets, n_docs, bytes_out, bytes_cap, out_offsets, status);
}

}  // extern "C"
