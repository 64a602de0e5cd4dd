// hutk_host.h -- what the C entry points of every direction share (hutk_api.cpp, hutk_decode.hip, hutk_spans.hip,
// hutk_special.hip, hutk_collate.hip, hutk_train.hip; DESIGN.md section 1, "Host layer").  Host code only: no kernel uses any of it.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "hutk_device.h"

// A failed HIP call ends the entry point: HUTK_E_DEVICE, and hutk_last_error() names the call.
#define HUTK_HIP_TRY(expr)                                                                                  \
    do {                                                                                                    \
        hipError_t e__ = (expr);                                                                            \
        if (e__ != hipSuccess)                                                                              \
            return hutk::api_set_error(HUTK_E_DEVICE, std::string("HIP error: ") + hipGetErrorString(e__) + \
                                                          " at " #expr);                                    \
    } while (0)

namespace hutk {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) {
            (void)hipDeviceSynchronize();  // an earlier asynchronous call may still be using the old allocation
            (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
        size_t want = n + n / 8 + 64;
        hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace hutk

using hutk::DevBuf;

struct hutk_ctx {
    hutk::Tables tab;
    int device = -1;
    bool host_only = false;
    bool timing = true;

    // device tables
    DevBuf<uint64_t> d_pair, d_char;
    DevBuf<int32_t> d_sym_id, d_prefix_alone;
    DevBuf<uint32_t> d_item_sym, d_prefix_syms, d_prefix_alone_syms, d_seam, d_seam2, d_item_units;
    DevBuf<uint8_t> d_item_direct, d_split_dfa;
    DevBuf<uint32_t> d_bytepair16;  // {symbol, merged} as 16 + 16 bits
    DevBuf<hutk::WordSlot> d_word_tab;
    int64_t n_word_entries = 0, n_wordl_entries = 0;  // whole-word table entries in all, and those of the long-word companion
    DevBuf<uint64_t> d_bytepair32;  // {symbol, merged} as 32 + 32 bits
    DevBuf<long long> w_prof;
    bool profile = false;
    // regex pre-token path: the pattern of initialize() (empty: the hand-written splitter) and the bitmaps of a batch
    std::string pattern;
    DevBuf<uint32_t> w_wbits, w_gbits, w_fbits, w_abits;
    hutk::DevTables dt{};

    // workspace
    DevBuf<uint32_t> w_run;
    DevBuf<int32_t> w_exc_tok;
    DevBuf<uint32_t> w_exc_sym, w_exc_mrg, w_tile_u32, w_doc_pos, w_counters;
    DevBuf<int64_t> w_tile_i64;
    DevBuf<hutk::ExcRec> w_exc;
    DevBuf<uint32_t> w_exc_quad, w_exc_mid, w_exc_wave;

    // decode direction: tables and workspace
    DevBuf<uint2> d_dec_ent, d_dec_sent;
    DevBuf<uint8_t> d_dec_blob;
    hutk::DecTables dec{};
    DevBuf<uint32_t> dw_first;
    DevBuf<unsigned long long> dw_state;
    DevBuf<int64_t> dw_tfd;
    DevBuf<int32_t> dw_ids;  // hutk_decode_special_batch_device: the ids with the special ones renumbered
    DevBuf<int32_t> ds_ids, ds_status;
    DevBuf<int64_t> ds_offs, ds_oo;
    DevBuf<uint8_t> ds_bytes;
    DevBuf<int32_t> w_err;
    // token spans: the rank / select structure over the batch's character starts, staging of the host-buffer form
    DevBuf<uint64_t> sp_bits;
    DevBuf<uint32_t> sp_in_chunk;
    DevBuf<int64_t> sp_chunk, sp_sel, ss_spans;
    DevBuf<int32_t> sp_ok;
    uint32_t dec_max_len = 0;  // the longest decoded token, in bytes

    // special tokens (hutk_special.hip): the set as hutk_ctx_set_special_tokens validated it, its tables on the host and
    // on the device, and the workspace of hutk_encode_special_batch_device
    struct Specials {
        int64_t n = 0;                 // pairs in the set; 0: none installed
        std::vector<uint8_t> blob;     // the strings, end to end
        std::vector<uint32_t> off;     // [n + 1] into blob
        std::vector<int32_t> ids;      // [n]
        std::vector<uint2> slots;      // open-addressed set of the strings: {hash of the bytes, index | length << 16}
        std::vector<uint32_t> filt;    // three 256-bit sets: first bytes, second bytes, lengths
        uint32_t mask = 0, max_len = 0, n_first = 0, first[4] = {0, 0, 0, 0};
        int64_t last_matches = 0;
        // decode direction (hutk_decode_special_batch_device): the context's decode tables followed by one entry per
        // DISTINCT special id, in the order of the ids' first pairs; x_sent: the same behind the first-token entries
        // (a special's entry there equals its x_ent entry; empty without a prefix); *_skip: the specials' entries have
        // length 0 (HUTK_DECODE_SKIP_SPECIAL); x_blob: the context's blob, then the strings of more than 7 bytes
        std::vector<uint2> x_ent, x_sent, x_ent_skip, x_sent_skip, x_slots;
        std::vector<uint8_t> x_blob;
        int64_t x_n = 0;  // distinct ids
        int32_t x_min = 0, x_max = 0;
        DevBuf<uint2> dx_ent, dx_sent, dx_ent_skip, dx_sent_skip, dx_slots;
        DevBuf<uint8_t> dx_blob;
        DevBuf<uint8_t> d_blob, w_mlen, w_sel;
        DevBuf<uint32_t> d_off, d_filt;
        DevBuf<uint2> d_slots;
        DevBuf<int32_t> d_ids, w_pspecial, w_pstatus, w_pids;
        DevBuf<int64_t> w_tile, w_mstart, w_poff, w_first, w_poo, w_blk, w_dst;
        void release() {
            d_blob.release(); w_mlen.release(); w_sel.release(); d_off.release(); d_filt.release(); d_slots.release();
            d_ids.release(); w_pspecial.release(); w_pstatus.release(); w_pids.release(); w_tile.release();
            w_mstart.release(); w_poff.release(); w_first.release(); w_poo.release(); w_blk.release(); w_dst.release();
            dx_ent.release(); dx_sent.release(); dx_ent_skip.release(); dx_sent_skip.release(); dx_slots.release();
            dx_blob.release();
        }
    } sx;

    // byte fallback (hutk_fallback.hip): the table of hutk_ctx_set_byte_fallback, the decode tables extended by it, and
    // the workspace of hutk_encode_fallback_batch_device
    struct Fallback {
        bool on = false;
        int32_t ids[256] = {0};
        bool clash = false;            // an id of the table is a special id too (HUTK_FB_SPECIAL refuses)
        // decode: [vocabulary lines][the distinct special ids, when a set is installed][256 one-byte entries]
        int64_t base = 0;              // entries in front of the 256
        bool strip = false;            // the context strips a prefix: dx_sent* are in use
        int32_t id_min = 0, id_max = 0;
        DevBuf<uint2> dx_ent, dx_sent, dx_ent_skip, dx_sent_skip, dx_slots;
        DevBuf<uint8_t> dx_blob;
        // encode: the table, the plain encode's outputs (offsets with one more entry: the unused ids behind the batch
        // as a document), their byte spans and the spans' status, per-tile counts
        DevBuf<int32_t> d_tab, w_ids, w_spans, w_sstatus, w_serr;
        DevBuf<int64_t> w_oo, w_doff, w_tile, w_hdr;
        void release() {
            dx_ent.release(); dx_sent.release(); dx_ent_skip.release(); dx_sent_skip.release(); dx_slots.release();
            dx_blob.release(); d_tab.release(); w_ids.release(); w_spans.release(); w_sstatus.release(); w_serr.release();
            w_oo.release(); w_doff.release(); w_tile.release(); w_hdr.release();
        }
    } fb;

    // staging for the host-buffer entry point
    DevBuf<uint8_t> s_bytes;
    DevBuf<int64_t> s_offsets, s_out_offsets;
    DevBuf<int32_t> s_ids, s_status;
    // small batches: one page-locked host buffer, one device buffer each way
    DevBuf<uint8_t> s_small_in, s_small_out;
    void* small_host = nullptr;
    // pipelined host path (hutk_encode_batch on large batches): two sets of chunk buffers, copy streams,
    // pinned staging for the rebased offsets and the small per-chunk results
    struct Pipe {
        // THREE sets of chunk buffers: the copy up of chunk c is enqueued while chunk c - 2's copy down is still under way
        // (with two sets the host had to see that copy end first: a host round trip in the pipeline's critical path)
        static constexpr int NB = 3;
        DevBuf<uint8_t> bytes[NB];
        DevBuf<int64_t> offs[NB], offs_abs[NB], oo[NB], base;  // base: ids of the chunks already encoded
        DevBuf<int32_t> ids[NB], status[NB], err[NB];
        hipStream_t s_in = nullptr, s_out = nullptr;
        hipEvent_t ev_in[NB] = {}, ev_comp[NB] = {}, ev_out[NB] = {};
        // page-locked landing place of a chunk's error word and id total: a copy to PAGEABLE memory (a stack variable)
        // waits for the copy engine's whole queue -- the next chunk's copy up included -- and the two directions then
        // take turns instead of overlapping (tools/pipe_trace.py)
        int64_t* h_small = nullptr;
        bool ready = false;
    } pipe;

    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    // One workspace per context: calls on a context are SERIALISED.  The mutex orders the host side (calls from several
    // threads), the event orders the device side: every asynchronous call records it when its last kernel is enqueued,
    // and the next call's stream waits for it before its first kernel -- whatever streams the two calls run on (StreamScope).
    std::recursive_mutex mu;
    hipEvent_t ev_busy = nullptr;
    bool busy_valid = false;

    // Single-process multi-device dispatch (hutk_ctx_add_device): further contexts with the same tables on other
    // devices; hutk_encode_batch cuts a large batch into byte-balanced runs of whole documents, one per device, and
    // every run is encoded by its device's context on a host thread of its own.  peer_ids: page-locked landing area
    // of a peer's ids (they are copied to their place once the runs before them are counted).
    std::vector<hutk_ctx*> peers;
    struct PeerBuf { int32_t* p = nullptr; size_t cap = 0; };
    std::vector<PeerBuf> peer_ids;
};

namespace hutk {

// The stretch of one call in which it owns the context's workspace (the caller holds c->mu).  Opening it selects the
// context's device, takes the caller's stream (or the context's own) and makes that stream wait for ev_busy: the previous
// call on the context, on whatever stream, still owns the workspace.  Closing it records ev_busy on the stream: on every
// way out, behind whatever the call has queued.  rc != HUTK_OK: it did not open, the entry point returns rc and nothing is
// recorded.  An entry point opens it where its wait belongs; one that returns earlier has queued nothing.
// select_device = false: the caller has selected the device already (it allocates before it waits).
struct StreamScope {
    hutk_ctx* const c;
    hipStream_t s = nullptr;
    int rc;
    StreamScope(hutk_ctx* ctx, void* hip_stream, bool select_device = true) : c(ctx) { rc = open(hip_stream, select_device); }
    ~StreamScope() { if (rc == HUTK_OK && hipEventRecord(c->ev_busy, s) == hipSuccess) c->busy_valid = true; }
    StreamScope(const StreamScope&) = delete;

private:
    int open(void* hip_stream, bool select_device) {
        if (select_device) HUTK_HIP_TRY(hipSetDevice(c->device));
        s = hip_stream ? (hipStream_t)hip_stream : c->stream;
        if (c->busy_valid) HUTK_HIP_TRY(hipStreamWaitEvent(s, c->ev_busy, 0));
        return HUTK_OK;
    }
};

// Host offsets of n_docs documents: (optionally) the first is 0, none is below the one before it.  `what` names the
// array in the message: "<what>[0] must be 0", "<what> must not decrease".
inline int check_offsets(const int64_t* offsets, int64_t n_docs, bool first_must_be_zero, const char* what) {
    if (first_must_be_zero && offsets[0] != 0) return api_set_error(HUTK_E_ARG, std::string(what) + "[0] must be 0");
    for (int64_t i = 0; i < n_docs; i++)
        if (offsets[i + 1] < offsets[i]) return api_set_error(HUTK_E_ARG, std::string(what) + " must not decrease");
    return HUTK_OK;
}

// The bitmaps of the regex pre-token path (hutk_api.cpp, regex_bitmaps) into the context's buffers, on stream s; f and a
// (the first matches: a context with a prefix) may be null.  d: the device pointers of w, g, f, a (null where none).
// The vectors are the copies' sources: they outlive the stream's work.
inline int upload_regex_bitmaps(hutk_ctx* c, hipStream_t s, const std::vector<uint32_t>& w, const std::vector<uint32_t>& g,
                                const std::vector<uint32_t>* f, const std::vector<uint32_t>* a, const uint32_t* (&d)[4]) {
    HUTK_HIP_TRY(c->w_wbits.reserve(w.size()));
    HUTK_HIP_TRY(c->w_gbits.reserve(g.size()));
    HUTK_HIP_TRY(hipMemcpyAsync(c->w_wbits.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, s));
    HUTK_HIP_TRY(hipMemcpyAsync(c->w_gbits.p, g.data(), g.size() * 4, hipMemcpyHostToDevice, s));
    d[0] = c->w_wbits.p, d[1] = c->w_gbits.p, d[2] = d[3] = nullptr;
    if (f) {
        HUTK_HIP_TRY(c->w_fbits.reserve(f->size()));
        HUTK_HIP_TRY(c->w_abits.reserve(a->size()));
        HUTK_HIP_TRY(hipMemcpyAsync(c->w_fbits.p, f->data(), f->size() * 4, hipMemcpyHostToDevice, s));
        HUTK_HIP_TRY(hipMemcpyAsync(c->w_abits.p, a->data(), a->size() * 4, hipMemcpyHostToDevice, s));
        d[2] = c->w_fbits.p, d[3] = c->w_abits.p;
    }
    return HUTK_OK;
}

// The decode tables of a context as the kernels read them (DecTables): one entry per vocabulary line in `ent`, and in
// `sent` (a context with a prefix; empty otherwise) the entry of the same token at the front of a document.
// max_len: the longest decoded token.  hutk_api.cpp uploads them; hutk_special.hip extends them by the special ids.
inline uint2 dec_pack_entry(const uint8_t* bytes, uint32_t off, uint32_t len, bool bad) {
    if (bad) return make_uint2(DEC_TAG_BAD, 0u);
    if (len > DEC_INLINE_MAX) return make_uint2(DEC_TAG_LONG | (len << 8), off);
    uint64_t v = len;
    for (uint32_t j = 0; j < len; j++) v |= (uint64_t)bytes[off + j] << (8 * (j + 1));
    return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
inline void dec_pack_tables(const Tables& T, std::vector<uint2>& ent, std::vector<uint2>& sent, uint32_t& max_len) {
    const size_t N = (size_t)T.dec_n;
    ent.assign(N ? N : 1, make_uint2(0, 0));
    sent.clear();
    max_len = 0;
    auto pack = [&](uint32_t off, uint32_t len, bool bad) {
        if (!bad && len > max_len) max_len = len;
        return dec_pack_entry(T.dec_blob.data(), off, len, bad);
    };
    // DEC_F_PFX_PARTIAL only matters at the front of a document
    for (size_t i = 0; i < N; i++)
        ent[i] = pack(T.dec_off[i], T.dec_len[i], T.dec_len[i] == DEC_BAD || (T.dec_flag[i] & ~DEC_F_PFX_PARTIAL));
    if (T.dec_slen.empty()) return;
    sent.assign(N ? N : 1, make_uint2(0, 0));
    for (size_t i = 0; i < N; i++) {
        const bool strip = T.dec_slen[i] != DEC_NOSTRIP;
        const uint32_t len = strip ? T.dec_slen[i] : T.dec_len[i];
        sent[i] = pack(strip ? T.dec_soff[i] : T.dec_off[i], len, len == DEC_BAD || T.dec_flag[i]);
    }
}

// hutk_decode.hip: the decode behind hutk_decode_batch_device (the caller has checked c and holds no lock yet): its
// checks, its workspace, every kernel of the direction, with the tables `t`.  sp != nullptr: the ids are renumbered by
// launch_dec_remap first (hutk_special.hip), and t are the extended tables.
// fb != nullptr (with sp): the pass is launch_fb_remap (hutk_fallback.hip), t has the one-byte entries too.
int decode_device_impl(hutk_ctx* c, const DecTables& t, const DecSpecial* sp, const int32_t* d_ids, const int64_t* d_id_offsets,
                       int64_t n_docs, int64_t n_ids, uint8_t* d_bytes_out, int64_t bytes_cap, int64_t* d_out_offsets,
                       int32_t* d_status, int32_t* d_err, void* hip_stream, const DecFallback* fb = nullptr);
// ... and the staging of hutk_decode_batch around it.  special_flags < 0: the plain decode; otherwise
// hutk_decode_special_batch_device with these flags.  fallback_flags >= 0: hutk_decode_fallback_batch_device with those.
int decode_host_impl(hutk_ctx* c, int special_flags, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs,
                     uint8_t* bytes_out, int64_t bytes_cap, int64_t* out_offsets, int32_t* status, int fallback_flags = -1);

// hutk_special.hip: the encode behind hutk_encode_special_batch_device; fallback: the text pieces go through
// encode_fallback_device_impl instead of encode_device_impl (hutk_encode_fallback_batch_device with HUTK_FB_SPECIAL).
int encode_special_impl(hutk_ctx* c, bool fallback, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                        int64_t n_bytes, int32_t* d_ids_out, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_status,
                        int32_t* d_err, void* hip_stream);
// hutk_fallback.hip: encode_device_impl's arguments (without the regex bitmaps); plain encode, byte spans, expansion.
// The caller holds c->mu and has checked that a table is installed and that the spans take the context.
int encode_fallback_device_impl(hutk_ctx* c, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                                int32_t* d_ids_out, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_status, int32_t* d_err,
                                void* hip_stream);
// ... and the decode tables of the byte-fallback decode, built again from the context's and the special set's whenever
// either changes (no table installed: nothing to do).  The caller holds c->mu.
int fallback_rebuild_decode(hutk_ctx* c);

// What the host-buffer entry points say about the error word a direction's kernels left (err != HUTK_OK).
enum class Direction { Encode, Decode, Spans };
inline const char* device_error_message(Direction dir, int err) {
    static const struct { Direction dir; int err; const char* text; } texts[] = {
        {Direction::Encode, HUTK_E_NUL_BYTE, "a document contains a 0x00 byte"},
        {Direction::Encode, HUTK_E_INVALID_UTF8, "text is not valid UTF-8 (non-byte-encoder mode)"},
        {Direction::Encode, HUTK_E_CAPACITY, "ids_cap too small"},
        {Direction::Decode, HUTK_E_VALUE, "Element must be non-negative and less than vocab size."},
        {Direction::Decode, HUTK_E_UNSUPPORTED, "a token cannot be decoded on its own (id without a unique key, or a token that ends "
                                                "inside a special value or a character)"},
        {Direction::Decode, HUTK_E_CAPACITY, "bytes_cap too small"},
        {Direction::Spans, HUTK_E_ARG, "offsets that do not describe the buffers, or a document of 2^31 bytes or more with 32-bit spans"},
        {Direction::Spans, HUTK_E_UNSUPPORTED, "the source text does not hold a token's decoded bytes where its span lies (see status: "
                                               "HUTK_DOC_SPAN_MISMATCH)"}};
    for (const auto& t : texts)
        if (t.dir == dir && t.err == err) return t.text;
    return "device-side failure";
}

}  // namespace hutk
