// hutk_host.h -- what the C entry points of every direction share (hutk_api.cpp, hutk_decode.hip, hutk_spans.hip,
// hutk_special.hip, hutk_collate.hip, hutk_train.hip; DESIGN.md section 1, "Host layer").  Host code only: no kernel uses any of it.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <utility>
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

// A host vector into a device buffer (one element more than it holds, so that an empty one has an address); the device is
// selected and idle.
template <class V, class D>
int upload_vec(D& d, const V& v) {
    HUTK_HIP_TRY(d.reserve(v.size() + 1));
    if (!v.empty()) HUTK_HIP_TRY(hipMemcpy(d.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
    return HUTK_OK;
}

// Extended decode tables: the context's entries followed by further ones (the special ids, the 256 bytes of the
// byte-fallback table), as dec_ext_build makes them on the host and upload() puts them on the device.
struct DecExt {
    struct Host {
        // ent: one entry per vocabulary line, then the further ones; sent: the same behind the first-token entries (a
        // further entry there equals its ent entry; empty without a prefix); *_skip: the forms for "skip the special
        // tokens"; slots: the open-addressed map of the caller's ids to the further entries; blob: the context's, then
        // the further strings of more than DEC_INLINE_MAX bytes on 4-byte boundaries, then 16 bytes
        std::vector<uint2> ent, sent, ent_skip, sent_skip, slots;
        std::vector<uint8_t> blob;
        int64_t n_extra = 0;               // further entries behind the vocabulary's
        int32_t id_min = 0, id_max = 0;    // the range of the ids in slots
        bool strip = false;                // the context strips a prefix: sent* are in use
    };
    DevBuf<uint2> dx_ent, dx_sent, dx_ent_skip, dx_sent_skip, dx_slots;
    DevBuf<uint8_t> dx_blob;
    int64_t n = 0;       // entries of the tables on the device
    bool strip = false;
    int upload(const Host& h) {
        if (int rc = upload_vec(dx_ent, h.ent)) return rc;
        if (int rc = upload_vec(dx_ent_skip, h.ent_skip)) return rc;
        if (int rc = upload_vec(dx_sent, h.sent)) return rc;
        if (int rc = upload_vec(dx_sent_skip, h.sent_skip)) return rc;
        if (int rc = upload_vec(dx_slots, h.slots)) return rc;
        if (int rc = upload_vec(dx_blob, h.blob)) return rc;
        n = (int64_t)h.ent.size();
        strip = h.strip;
        return HUTK_OK;
    }
    DecTables tables(bool skip) const {
        DecTables t{};
        t.ent = skip ? dx_ent_skip.p : dx_ent.p;
        t.sent = !strip ? nullptr : skip ? dx_sent_skip.p : dx_sent.p;
        t.blob = dx_blob.p;
        t.n = n;
        return t;
    }
    void release() {
        dx_ent.release(); dx_sent.release(); dx_ent_skip.release(); dx_sent_skip.release(); dx_slots.release();
        dx_blob.release();
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
    // word cache (hutk_wcache.h): slots, their tag words, the control words, and the candidate list of a batch (allocated
    // by the first batch that learns); wc_list_cap == 0: the context has no table
    DevBuf<uint4> d_wc_tab, d_wc_list;
    DevBuf<uint32_t> d_wc_tags, d_wc_ctl;
    uint32_t wc_list_cap = 0;
    DevBuf<uint64_t> d_bytepair32;  // {symbol, merged} as 32 + 32 bits
    DevBuf<long long> w_prof;
    bool profile = false;
    // regex pre-token path: the pattern of initialize() (empty: the hand-written splitter) and the bitmaps of a batch
    std::string pattern;
    DevBuf<uint32_t> w_wbits, w_gbits, w_fbits, w_abits;
    // a split preset (hutk_ctx_set_pretokenizer, HUTK_PRESPLIT_*; -1: none): encode_device_impl has pretok write w_wbits on
    // the device in front of its kernels.  presplit_blob: the tables, for the devices hutk_ctx_add_device adds later
    int presplit = -1;
    struct hutk_pretokenizer* pretok = nullptr;
    std::vector<uint8_t> presplit_blob;
    hutk::DevTables dt{};

    // workspace
    DevBuf<uint32_t> w_run;
    DevBuf<int32_t> w_exc_tok;
    DevBuf<uint32_t> w_exc_sym, w_exc_mrg, w_tile_u32, w_doc_pos, w_counters;
    DevBuf<int64_t> w_tile_i64;
    DevBuf<hutk::ExcRec> w_exc;
    DevBuf<uint32_t> w_exc_quad, w_exc_mid, w_exc_wave;
    int last_tail = -1;  // the tail enqueued last: 0 k_exc_a .. k_finish, 1 k_tail_small (encode_device_impl); 2 none, 3 k_tail_small behind the one-launch k_tiles (encode_one_shot); -1 none yet (hutk_debug_exc_counts)

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

    // special tokens (hutk_special.hip).  sx: the set as hutk_ctx_set_special_tokens validated it and its tables, on the
    // host only: default-movable, a fresh one is built aside and moved in.  sxd: the tables on the device and the
    // workspace of hutk_encode_special_batch_device, which stay where they are when the set changes.
    struct Specials {
        int64_t n = 0;                 // pairs in the set; 0: none installed
        std::vector<uint8_t> blob;     // the strings, end to end
        std::vector<uint32_t> off;     // [n + 1] into blob
        std::vector<int32_t> ids;      // [n]
        std::vector<uint2> slots;      // open-addressed set of the strings: {hash of the bytes, index | length << 16}
        std::vector<uint32_t> filt;    // three 256-bit sets: first bytes, second bytes, lengths
        uint32_t mask = 0, max_len = 0, n_first = 0, first[4] = {0, 0, 0, 0};
        // decode direction (hutk_decode_special_batch_device): the context's decode tables followed by one entry per
        // DISTINCT special id, in the order of the ids' first pairs; *_skip: those entries have length 0
        // (HUTK_DECODE_SKIP_SPECIAL); slots: id -> index among the distinct ids
        hutk::DecExt::Host dec;
    } sx;
    struct SpecialsDev {
        hutk::DecExt dec;
        int64_t last_matches = 0;
        DevBuf<uint8_t> d_blob, w_mlen, w_sel;
        DevBuf<uint32_t> d_off, d_filt;
        DevBuf<uint2> d_slots;
        DevBuf<int32_t> d_ids, w_pspecial, w_pstatus, w_pids;
        DevBuf<int64_t> w_tile, w_mstart, w_poff, w_first, w_poo, w_blk, w_dst;
        void release() {
            dec.release();
            d_blob.release(); w_mlen.release(); w_sel.release(); d_off.release(); d_filt.release(); d_slots.release();
            d_ids.release(); w_pspecial.release(); w_pstatus.release(); w_pids.release(); w_tile.release();
            w_mstart.release(); w_poff.release(); w_first.release(); w_poo.release(); w_blk.release(); w_dst.release();
        }
    } sxd;

    // byte fallback (hutk_fallback.hip): the table of hutk_ctx_set_byte_fallback, the decode tables extended by it, and
    // the workspace of hutk_encode_fallback_batch_device
    struct Fallback {
        bool on = false;
        int32_t ids[256] = {0};
        bool clash = false;            // an id of the table is a special id too (HUTK_FB_SPECIAL refuses)
        // decode: [vocabulary lines][the distinct special ids, when a set is installed][256 one-byte entries];
        // dec's slots: table id -> byte
        int64_t base = 0;              // entries in front of the 256
        int32_t id_min = 0, id_max = 0;
        hutk::DecExt dec;
        // encode: the table, the plain encode's outputs (offsets with one more entry: the unused ids behind the batch
        // as a document), their byte spans and the spans' status, per-tile counts
        DevBuf<int32_t> d_tab, w_ids, w_spans, w_sstatus, w_serr;
        DevBuf<int64_t> w_oo, w_doff, w_tile, w_hdr;
        void release() {
            dec.release(); d_tab.release(); w_ids.release(); w_spans.release(); w_sstatus.release(); w_serr.release();
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

// The tables of DecExt on the host: the context's packed tables trimmed to its vocabulary (under == nullptr) or the
// tables `under` made from them, followed by one entry per string of `extra` ({bytes, length}).  A string of more than
// DEC_INLINE_MAX bytes goes to the blob, on a 4-byte boundary as the loader's entries; the blob ends on one, plus 16 bytes.
// skip_empties: the *_skip forms hold entries of length 0 for the strings (they are what "skip" deletes); otherwise the
// same entries.  More than INT32_MAX entries: HUTK_E_UNSUPPORTED with `refusal`.  out.slots, id_min and id_max are the
// caller's to fill: only it knows its ids.
inline int dec_ext_build(const Tables& T, const DecExt::Host* under, const std::vector<std::pair<const uint8_t*, uint32_t>>& extra,
                         bool skip_empties, const char* refusal, DecExt::Host& out) {
    int64_t before = 0;
    if (under) {
        out.ent = under->ent, out.sent = under->sent, out.ent_skip = under->ent_skip, out.sent_skip = under->sent_skip;
        out.blob = under->blob;
        out.blob.resize(out.blob.size() - 16);  // (its tail: put back below)
        before = under->n_extra;
    } else {
        uint32_t max_len = 0;
        dec_pack_tables(T, out.ent, out.sent, max_len);
        out.ent.resize((size_t)T.dec_n);  // (an empty vocabulary has one unused entry)
        if (!out.sent.empty()) out.sent.resize((size_t)T.dec_n);
        out.ent_skip = out.ent, out.sent_skip = out.sent, out.blob = T.dec_blob;
    }
    out.n_extra = before + (int64_t)extra.size();
    if (T.dec_n + out.n_extra > (int64_t)INT32_MAX) return api_set_error(HUTK_E_UNSUPPORTED, refusal);
    out.strip = !out.sent.empty();
    for (const auto& x : extra) {
        const uint8_t* from = x.first;
        uint32_t at = 0;
        if (x.second > DEC_INLINE_MAX) {
            out.blob.resize((out.blob.size() + 3) & ~(size_t)3, 0);
            at = (uint32_t)out.blob.size();
            out.blob.insert(out.blob.end(), from, from + x.second);
        }
        const uint2 e = dec_pack_entry(from, at, x.second, false), e_skip = skip_empties ? make_uint2(0, 0) : e;
        out.ent.push_back(e);
        out.ent_skip.push_back(e_skip);
        if (out.strip) out.sent.push_back(e), out.sent_skip.push_back(e_skip);  // never stripped of a prefix
    }
    out.blob.resize(((out.blob.size() + 3) & ~(size_t)3) + 16, 0);
    return HUTK_OK;
}

// hutk_decode.hip: the decode behind hutk_decode_batch_device (the caller has checked c and holds no lock yet): its
// checks, its workspace, every kernel of the direction, with the tables `t`.  sp != nullptr: the ids are renumbered by
// launch_dec_remap first (hutk_special.hip), and t are the extended tables.
// fb != nullptr (with sp): the pass is launch_fb_remap (hutk_fallback.hip), t has the one-byte entries too.
int decode_device_impl(hutk_ctx* c, const DecTables& t, const DecSpecial* sp, const int32_t* d_ids, const int64_t* d_id_offsets,
                       int64_t n_docs, int64_t n_ids, uint8_t* d_bytes_out, int64_t bytes_cap, int64_t* d_out_offsets,
                       int32_t* d_status, int32_t* d_err, void* hip_stream, const DecFallback* fb = nullptr);
// ... and the staging of hutk_decode_batch and its special and fallback forms around it (the caller has checked c and its
// flags).  device(d_ids, d_id_offsets, n_ids, d_bytes_out, d_out_offsets, d_status, d_err, stream): the variant's device
// entry point on the staged batch.
template <class Device>
int decode_host_impl(hutk_ctx* c, Device device, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, uint8_t* bytes_out,
                     int64_t bytes_cap, int64_t* out_offsets, int32_t* status) {
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (c->host_only) return api_set_error(HUTK_E_DEVICE, "host-only context: no device to decode on");
    if (n_docs < 0 || !id_offsets || !out_offsets) return api_set_error(HUTK_E_ARG, "bad argument");
    if (int rc = check_offsets(id_offsets, n_docs, true, "id_offsets")) return rc;
    const int64_t n_ids = id_offsets[n_docs];
    if (n_ids > 0 && !ids) return api_set_error(HUTK_E_ARG, "bad argument");
    HUTK_HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HUTK_HIP_TRY(c->ds_ids.reserve((size_t)n_ids + 16));
    HUTK_HIP_TRY(c->ds_offs.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->ds_oo.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->ds_status.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->w_err.reserve(1));
    if (bytes_out && bytes_cap > 0) HUTK_HIP_TRY(c->ds_bytes.reserve((size_t)bytes_cap + 16));
    if (n_ids) HUTK_HIP_TRY(hipMemcpyAsync(c->ds_ids.p, ids, (size_t)n_ids * 4, hipMemcpyHostToDevice, s));
    HUTK_HIP_TRY(hipMemcpyAsync(c->ds_offs.p, id_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    if (int rc = device(c->ds_ids.p, c->ds_offs.p, n_ids, bytes_out ? c->ds_bytes.p : nullptr, c->ds_oo.p, c->ds_status.p,
                        c->w_err.p, s))
        return rc;
    int32_t err = 0;
    HUTK_HIP_TRY(hipMemcpyAsync(out_offsets, c->ds_oo.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
    HUTK_HIP_TRY(hipMemcpyAsync(&err, c->w_err.p, 4, hipMemcpyDeviceToHost, s));
    if (status && n_docs) HUTK_HIP_TRY(hipMemcpyAsync(status, c->ds_status.p, (size_t)n_docs * 4, hipMemcpyDeviceToHost, s));
    HUTK_HIP_TRY(hipStreamSynchronize(s));
    if (bytes_out && err == HUTK_OK && out_offsets[n_docs] > 0)
        HUTK_HIP_TRY(hipMemcpy(bytes_out, c->ds_bytes.p, (size_t)out_offsets[n_docs], hipMemcpyDeviceToHost));
    return err == HUTK_OK ? HUTK_OK : api_set_error(err, device_error_message(Direction::Decode, err));
}

// The staging of hutk_encode_special_batch and hutk_encode_fallback_batch (`who` in the messages) around their device
// entry points.  The caller has checked its arguments (n_bytes = offsets[n_docs]), holds c->mu and has computed `cap`, the
// capacity of the batch (ids_cap >= cap - 1).  device(d_bytes, d_offsets, d_ids, d_out_offsets, d_status, d_err, stream):
// the entry point on the staged batch.  refuse(err): the error word is neither HUTK_OK nor HUTK_E_WORD_TOO_LARGE; it sets
// the message and says whether the call ends there (false: a note, the ids are copied down and err is returned).
template <class Device, class Refuse>
int encode_host_impl(hutk_ctx* c, const char* who, int64_t cap, Device device, Refuse refuse, const uint8_t* bytes,
                     const int64_t* offsets, int64_t n_docs, int64_t n_bytes, int32_t* ids_out, int64_t ids_cap,
                     int64_t* out_offsets, int32_t* status) {
    HUTK_HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HUTK_HIP_TRY(c->s_bytes.reserve((size_t)n_bytes + 16));
    HUTK_HIP_TRY(c->s_offsets.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->s_ids.reserve((size_t)cap + 16));
    HUTK_HIP_TRY(c->s_out_offsets.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->s_status.reserve((size_t)n_docs + 1));
    HUTK_HIP_TRY(c->w_err.reserve(1));
    if (c->busy_valid) HUTK_HIP_TRY(hipStreamWaitEvent(s, c->ev_busy, 0));  // (the staging buffers are the context's)
    if (n_bytes) HUTK_HIP_TRY(hipMemcpyAsync(c->s_bytes.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HUTK_HIP_TRY(hipMemcpyAsync(c->s_offsets.p, offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    if (int rc = device(c->s_bytes.p, c->s_offsets.p, c->s_ids.p, c->s_out_offsets.p, c->s_status.p, c->w_err.p, s)) return rc;
    int32_t err = 0;
    HUTK_HIP_TRY(hipMemcpyAsync(&err, c->w_err.p, 4, hipMemcpyDeviceToHost, s));
    HUTK_HIP_TRY(hipMemcpyAsync(out_offsets, c->s_out_offsets.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
    if (status && n_docs) HUTK_HIP_TRY(hipMemcpyAsync(status, c->s_status.p, (size_t)n_docs * 4, hipMemcpyDeviceToHost, s));
    HUTK_HIP_TRY(hipStreamSynchronize(s));
    if (err != HUTK_OK && err != HUTK_E_WORD_TOO_LARGE && refuse(err)) return err;
    const int64_t n_ids = out_offsets[n_docs];
    if (n_ids < 0 || n_ids > ids_cap) return api_set_error(HUTK_E_DEVICE, std::string(who) + ": bad id count");
    if (n_ids) HUTK_HIP_TRY(hipMemcpy(ids_out, c->s_ids.p, (size_t)n_ids * 4, hipMemcpyDeviceToHost));
    return err;  // HUTK_OK, the note HUTK_E_WORD_TOO_LARGE (see status), or what refuse() let pass
}

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

}  // namespace hutk
