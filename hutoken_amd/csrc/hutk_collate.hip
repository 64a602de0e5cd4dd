// hutk_collate.hip -- collation of encoded batches on the GPU: the ragged (ids, offsets) pair that hutk_encode_batch_device
// writes becomes what a model reads.  Two families of layouts (include/hutoken_amd.h):
//
//   rows     a row of max_len elements is [bos] A' sep.. B' [eos], padded left or right, with the attention mask and the
//            lengths.  ONE writer (write_rows) turns a planned row into elements; a kernel is a planner that says which
//            item a row belongs to, where its ids start and how many stay, and then calls the writer:
//              padded   row i is document i, truncated on either side                   (k_collate_padded)
//              windows  a document longer than max_len - s is cut into overlapping windows, with a map from rows back to
//                       documents                                                       (k_collate_windows)
//              pairs    document i of two ragged pairs in one row, cut by one of three strategies, with token type ids;
//                       or the named side in windows, the other side whole in every row (k_collate_pairs)
//            The rows' places in the two windows forms come from ONE count, scan, write over the items first
//            (k_rows_count, k_rows_write over "rows of item i": DocRows, PairRows).
//   packed   the sequences of all documents laid end to end and cut into rows of seq_len, with position and segment
//            ids; the unfinished row is carried over to the next call                  (k_collate_packed, k_collate_flush)
// and what makes the per-token information of a row arrive in the row's shape: the geometry of
// the rows as a device array, the row plan, written by a planner per row layout that places a row with the device
// functions its collate kernel places it with (k_plan_padded, k_plan_windows, k_plan_pairs); the gather of any
// per-token array into the rows' shape by a plan (k_rows_gather); the columns of an answer in every row
// (k_rows_answers); and the last stage before a training batch: the masked-LM corruption of
// rows with its labels (k_rows_mlm, drawing from hutk_philox.h), the loss labels of rows (k_rows_labels), and the span
// corruption of rows into corrupted rows and target rows, a wavefront scanning and compacting its row
// (k_rows_span_corrupt).  In front of the layouts stands the chat render:
// the turns of conversations, one encoded document each, become one sequence per conversation with role headers,
// end-of-turn markers, loss labels, turn ids and source indices -- a ragged pair again, which every layout above takes
// (ChatTurns through the rows scan, k_chat_offsets, k_chat_render: the packed layout's shape).  Beside it stands the
// fill-in-the-middle render (the rule is hutk_fim.h): a document is cut into prefix / middle /
// suffix, at tokens or -- on the packed text, before the encode -- at characters, and re-ordered behind three sentinels,
// a ragged pair again (k_fim_cut, FimDocs through the rows scan, k_fim_plan, k_fim_render).  Behind the packed layout
// stand the packed rows for training: per-token channels that the packer moves along with the ids
// (k_collate_packed_ch, k_collate_flush_ch: siblings that share the packed kernels' body), cu_seqlens from the segment
// ids (CuStarts through the rows count and scan, k_cu_write, k_cu_gaps) and the loss labels of packed rows
// (k_packed_labels).
//
// All are one pass: every id is read once, every output element is written once, with 16-byte stores where the row
// length allows.  No element searches the offsets.  A workgroup of the row layouts stages the plan of its rows in LDS
// once; one of the packed layout owns a contiguous span of output, finds the span's first document with one search by a
// wavefront, marks the sequence starts of its span in LDS and turns the marks into "document of this position", "where
// its sequence starts" and "starts since the row began" with one workgroup scan.
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>

#include "hutk_fim.h"
#include "hutk_host.h"
#include "hutk_philox.h"
#include "hutk_wave.h"

namespace {

constexpr int TB = 256;          // threads per workgroup
constexpr int SPAN = 2048;       // packed: stream positions per workgroup (8 per thread)
constexpr int PER = SPAN / TB;   // packed: positions a thread scans
constexpr int PAD_TILE = 4096;   // rows: output elements per workgroup
constexpr int PAD_ROWS = 256;    // rows: most rows per workgroup

__device__ __forceinline__ void note_error(int32_t* err, int code) {
    if (err) atomicCAS(err, 0, code);
}

// four consecutive output elements of width W bytes, at element index i (16-byte aligned by the caller's choice of path)
template <int W>
__device__ __forceinline__ void store4(void* base, int64_t i, const int32_t (&v)[4]) {
    if constexpr (W == 4) {
        *reinterpret_cast<int4*>(static_cast<int32_t*>(base) + i) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
        longlong2* p = reinterpret_cast<longlong2*>(static_cast<int64_t*>(base) + i);
        p[0] = make_longlong2(v[0], v[1]);  // widened in registers
        p[1] = make_longlong2(v[2], v[3]);
    }
}
template <int W>
__device__ __forceinline__ void store1(void* base, int64_t i, int32_t v) {
    if constexpr (W == 4) static_cast<int32_t*>(base)[i] = v;
    else static_cast<int64_t*>(base)[i] = v;
}

// ---- rows: the tile and the writer ----------------------------------------------------------------------------------
// What the writer reads, the same for every row layout.  Padded and windows have one side, A; what only pairs have
// stays unset there and is never read (write_rows<.., PAIR = false>).
struct RowArgs {
    const int32_t *ids_a, *ids_b;
    int64_t cap_a, cap_b;  // elements of ids_a / ids_b: no id is read from outside them
    int32_t L, s;          // row length; bos, separators and eos together
    int32_t bos, eos, pad;
    int32_t sep0, sep1, sep2, sep3;  // (no array: a kernel argument indexed at run time lives in scratch)
    int32_t has_bos, n_sep, pad_left;
    void* out;
    uint8_t* mask;
    uint8_t* types;
    int32_t* lengths;
    int64_t* row_map;  // NULL: none (padded, pairs without windows)
    int32_t* err;
    int32_t rows_per_block;  // > 1 only when rows_per_block * L <= PAD_TILE
    int32_t col_chunks;      // pieces of PAD_TILE columns a row is cut into (1 unless rows_per_block == 1)
};

// A workgroup writes `rows_per_block` whole rows, or PAD_TILE columns of one long row: rows row0 .. row0 + nrows - 1,
// of each the columns c0 .. c0 + ncols - 1.  nrows <= 0: the workgroup has nothing to write.
struct RowTile {
    int64_t row0;
    int32_t nrows, c0, ncols, total;
    bool one_row;
};

__device__ __forceinline__ RowTile row_tile(const RowArgs& a, int64_t n_rows) {
    RowTile t;
    const int64_t blk = blockIdx.x;
    const int64_t rg = blk / a.col_chunks;
    const int32_t cc = (int32_t)(blk - rg * a.col_chunks);
    t.row0 = rg * a.rows_per_block;
    const int64_t left = n_rows - t.row0;
    t.nrows = left < a.rows_per_block ? (int32_t)left : a.rows_per_block;
    t.one_row = a.rows_per_block == 1;
    t.c0 = cc * PAD_TILE;
    t.ncols = t.one_row ? ((a.L - t.c0) < PAD_TILE ? (a.L - t.c0) : PAD_TILE) : a.L;
    t.total = t.nrows * t.ncols;
    return t;
}

// One planned row: ka ids of A and kb ids of B stay (kb: pairs only).  Element q of the unpadded row that is an id of A
// is ids_a[srca + q], one of B ids_b[srcb + q].  (item, start) is the row's entry of row_map.
struct RowPlan {
    int32_t ka, kb;
    int64_t srca, srcb;
    int64_t item, start;
};

// The elements of a tile, V neighbours per thread (VEC: the row length is a multiple of 4 and the outputs are aligned).
// plan(r) gives the plan of the tile's row r from wherever the calling kernel keeps it; an element is then a few
// comparisons against the row's boundaries and at most one dword read.  PAIR = false compiles the separators, the B side
// and the token types away.  Whatever a plan holds, no id is read from outside ids_a[0, cap_a) and ids_b[0, cap_b).
template <int W, bool VEC, bool PAIR, class Plan>
__device__ __forceinline__ void write_rows(const RowArgs& a, const RowTile& t, Plan plan) {
    constexpr int V = VEC ? 4 : 1;
    for (int32_t i = threadIdx.x * V; i < t.total; i += TB * V) {
        const int32_t rl = t.one_row ? 0 : i / a.L;
        const int32_t c = t.one_row ? t.c0 + i : i - rl * a.L;
        const RowPlan p = plan(rl);
        const int32_t end_a = a.has_bos + p.ka;
        const int32_t end_sep = PAIR ? end_a + a.n_sep : end_a, end_b = PAIR ? end_sep + p.kb : end_a;
        const int32_t sl = p.ka + (PAIR ? p.kb : 0) + a.s;
        const int32_t shift = a.pad_left ? a.L - sl : 0;
        int32_t v[V];
        uint8_t m[V], ty[V];
#pragma unroll
        for (int e = 0; e < V; e++) {
            const int32_t q = c + e - shift;
            v[e] = a.pad;
            m[e] = 0;
            ty[e] = 0;
            if (q >= 0 && q < sl) {
                m[e] = 1;
                if (q < a.has_bos) v[e] = a.bos;
                else if (q < end_a) {
                    const int64_t idx = p.srca + q;
                    if (idx >= 0 && idx < a.cap_a) v[e] = a.ids_a[idx];
                    else note_error(a.err, HUTK_E_ARG);
                } else if (PAIR && q < end_sep) {
                    const int32_t u = q - end_a;
                    v[e] = u == 0 ? a.sep0 : u == 1 ? a.sep1 : u == 2 ? a.sep2 : a.sep3;
                } else if (PAIR && q < end_b) {
                    ty[e] = 1;
                    const int64_t idx = p.srcb + q;
                    if (idx >= 0 && idx < a.cap_b) v[e] = a.ids_b[idx];
                    else note_error(a.err, HUTK_E_ARG);
                } else {
                    ty[e] = 1;
                    v[e] = a.eos;
                }
            }
        }
        const int64_t at = (t.row0 + rl) * (int64_t)a.L + c;
        if constexpr (VEC) {
            store4<W>(a.out, at, v);
            if (a.mask) *reinterpret_cast<uchar4*>(a.mask + at) = make_uchar4(m[0], m[1], m[2], m[3]);
            if (PAIR && a.types) *reinterpret_cast<uchar4*>(a.types + at) = make_uchar4(ty[0], ty[1], ty[2], ty[3]);
        } else {
            store1<W>(a.out, at, v[0]);
            if (a.mask) a.mask[at] = m[0];
            if (PAIR && a.types) a.types[at] = ty[0];
        }
        if (c == 0) {
            if (a.lengths) a.lengths[t.row0 + rl] = sl;
            if (a.row_map) {
                int64_t* rm = a.row_map + 2 * (t.row0 + rl);
                if constexpr (VEC) *reinterpret_cast<longlong2*>(rm) = make_longlong2(p.item, p.start);
                else rm[0] = p.item, rm[1] = p.start;
            }
        }
    }
}

// ---- padded -------------------------------------------------------------------------------------------------------
struct PadArgs {
    RowArgs r;  // (ids_a, cap_a: the ids and their number)
    const int64_t* offs;
    int64_t n_docs;
    int32_t trunc_left;
};

// Row i is document i.  The offsets of the tile's rows are staged in LDS once and ARE the plan: what stays of a
// document follows from its two offsets in a few integer operations.
template <int W, bool VEC>
__global__ __launch_bounds__(TB) void k_collate_padded(const PadArgs a) {
    __shared__ int64_t s_off[PAD_ROWS + 1];
    if (a.offs[0] != 0 || a.offs[a.n_docs] != a.r.cap_a) {  // nothing is read through offsets that do not fit the ids
        if (blockIdx.x == 0 && threadIdx.x == 0) note_error(a.r.err, HUTK_E_ARG);
        return;
    }
    const RowTile t = row_tile(a.r, a.n_docs);
    for (int32_t i = threadIdx.x; i <= t.nrows; i += TB) s_off[i] = a.offs[t.row0 + i];
    __syncthreads();
    const int32_t room = a.r.L - a.r.s;
    write_rows<W, VEC, false>(a.r, t, [&](int32_t rl) {
        const int64_t o0 = s_off[rl], o1 = s_off[rl + 1];
        int64_t dl = o1 - o0;
        if (dl < 0) {
            dl = 0;
            note_error(a.r.err, HUTK_E_ARG);
        }
        RowPlan p{};
        p.ka = dl > room ? room : (int32_t)dl;  // the document's own ids that stay
        p.srca = (a.trunc_left ? o1 - p.ka : o0) - a.r.has_bos;
        return p;
    });
}

// ---- packed -------------------------------------------------------------------------------------------------------
// Stream positions of one add call: 0 .. P-1 are the tokens carried over (they end at a document end, so their position
// and segment values are final), sequence j of the call begins at b_j = P + offsets[j] + j * s.  Rows are the stream cut
// every L positions, so the flat index of an output element IS its stream position; what lies behind the last whole row
// goes to the new carry instead.
struct PackArgs {
    const int32_t* ids;
    const int64_t* offs;
    int64_t n_docs, n_ids;
    int64_t L, P, total, rows;
    int32_t s, has_bos, has_eos;
    int32_t bos, eos;
    const int32_t *c_ids, *c_pos, *c_seg;  // the carry this call consumes (P entries)
    int32_t *n_ids_out, *n_pos, *n_seg;    // the carry it leaves (total - rows * L entries)
    void* out;
    int32_t* pos;
    int32_t* seg;
    int32_t* err;
    int32_t rows_per_block;  // L < SPAN: whole rows per workgroup
    int32_t spans_per_row;   // L >= SPAN: workgroups per row
};

// last document whose sequence begins at or before stream position x; -1 when none does.  All 64 lanes of a wavefront
// must call it; all get the answer.
__device__ __forceinline__ int64_t last_doc_le(const PackArgs& a, int64_t x) {
    return hutk::wave_count_leading(a.n_docs, [&](int64_t j) { return a.P + a.offs[j] + j * a.s <= x; }) - 1;
}

// A channel: a per-token array that lies along the offsets like the ids, records of 1 or 2 elements of 4 or 8 bytes, so
// 1, 2 or 4 dwords (include/hutoken_amd.h, PACKED CHANNELS).  The kernels move records as dwords
// and know the element width only for the alignment of a read from the caller's array; the packer's own carry is
// aligned to the record.
struct PackChan {
    const void* values;  // [n_ids] records, read at the index the id is read at
    void* rows;          // [rows][L] records
    const void* c_car;   // the carry this call consumes (P records)
    void* n_car;         // the carry it leaves
    int32_t f0, f1, f2, f3;  // the fill record (no array: PackArgs' note)
    int32_t words;       // dwords per record: 1, 2, 4
    int32_t w8;          // elements of 8 bytes (words 2: one of them; words 4: two)
};
struct PackChans {
    int32_t n;
    PackChan c[HUTK_PACKER_MAX_CHANNELS];
};

// A record in registers is an int4 of which the first WORDS components count.  Record i of a caller's array (aligned
// to its elements only) and of the packer's carry (aligned to the record):
template <int WORDS>
__device__ __forceinline__ int4 chan_load(const void* base, int64_t i, bool w8) {
    int4 r = make_int4(0, 0, 0, 0);
    const int32_t* p = static_cast<const int32_t*>(base) + i * WORDS;
    if constexpr (WORDS == 1) r.x = p[0];
    else if (w8) {
        const int2 x = reinterpret_cast<const int2*>(p)[0];
        r.x = x.x, r.y = x.y;
        if constexpr (WORDS == 4) {
            const int2 y = reinterpret_cast<const int2*>(p)[1];
            r.z = y.x, r.w = y.y;
        }
    } else {
        r.x = p[0], r.y = p[1];
        if constexpr (WORDS == 4) r.z = p[2], r.w = p[3];
    }
    return r;
}
template <int WORDS>
__device__ __forceinline__ void chan_store(void* base, int64_t i, bool w8, int4 r) {
    int32_t* p = static_cast<int32_t*>(base) + i * WORDS;
    if constexpr (WORDS == 1) p[0] = r.x;
    else if (w8) {
        reinterpret_cast<int2*>(p)[0] = make_int2(r.x, r.y);
        if constexpr (WORDS == 4) reinterpret_cast<int2*>(p)[1] = make_int2(r.z, r.w);
    } else {
        p[0] = r.x, p[1] = r.y;
        if constexpr (WORDS == 4) p[2] = r.z, p[3] = r.w;
    }
}
template <int WORDS>
__device__ __forceinline__ int4 carry_load(const void* base, int64_t i) {
    if constexpr (WORDS == 1) return make_int4(static_cast<const int32_t*>(base)[i], 0, 0, 0);
    else if constexpr (WORDS == 2) {
        const int2 x = static_cast<const int2*>(base)[i];
        return make_int4(x.x, x.y, 0, 0);
    } else return static_cast<const int4*>(base)[i];
}
template <int WORDS>
__device__ __forceinline__ void carry_store(void* base, int64_t i, int4 r) {
    if constexpr (WORDS == 1) static_cast<int32_t*>(base)[i] = r.x;
    else if constexpr (WORDS == 2) static_cast<int2*>(base)[i] = make_int2(r.x, r.y);
    else static_cast<int4*>(base)[i] = r;
}

// where a record comes from: src >= 0 the index the id was read at, -1 the fill (bos, eos, behind the stream's end,
// offsets that do not describe the ids), <= -2 slot -2 - src of the consumed carry
template <int WORDS>
__device__ __forceinline__ int4 chan_record(const PackChan& c, int64_t src) {
    if (src >= 0) return chan_load<WORDS>(c.values, src, c.w8 != 0);
    if (src < -1) return carry_load<WORDS>(c.c_car, -2 - src);
    return make_int4(c.f0, c.f1, c.f2, c.f3);
}

// The records of one channel behind the elements a thread has just placed.  They go where the ids went: to the rows at
// element `at` (four of them as WORDS 16-byte stores) or, behind the last whole row, to the new carry.
template <int WORDS>
__device__ __forceinline__ void chan_emit4(const PackChan& c, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t at,
                                           int64_t out_end, int64_t total) {
    const int4 r0 = chan_record<WORDS>(c, s0), r1 = chan_record<WORDS>(c, s1), r2 = chan_record<WORDS>(c, s2),
               r3 = chan_record<WORDS>(c, s3);
    if (at < out_end) {
        int4* o = static_cast<int4*>(c.rows) + (at >> 2) * WORDS;  // (at is a multiple of 4 on this path)
        if constexpr (WORDS == 1) o[0] = make_int4(r0.x, r1.x, r2.x, r3.x);
        else if constexpr (WORDS == 2) {
            o[0] = make_int4(r0.x, r0.y, r1.x, r1.y);
            o[1] = make_int4(r2.x, r2.y, r3.x, r3.y);
        } else o[0] = r0, o[1] = r1, o[2] = r2, o[3] = r3;
    } else {
        const int64_t t = at - out_end;
        if (at < total) carry_store<WORDS>(c.n_car, t, r0);
        if (at + 1 < total) carry_store<WORDS>(c.n_car, t + 1, r1);
        if (at + 2 < total) carry_store<WORDS>(c.n_car, t + 2, r2);
        if (at + 3 < total) carry_store<WORDS>(c.n_car, t + 3, r3);
    }
}
template <int WORDS>
__device__ __forceinline__ void chan_emit1(const PackChan& c, int64_t s0, int64_t at, int64_t out_end, int64_t total) {
    const int4 r = chan_record<WORDS>(c, s0);
    if (at < out_end) chan_store<WORDS>(c.rows, at, c.w8 != 0, r);
    else if (at < total) carry_store<WORDS>(c.n_car, at - out_end, r);
}
template <int WORDS, bool VEC>
__device__ __forceinline__ void chan_emit(const PackChan& c, const int64_t (&src)[VEC ? 4 : 1], int64_t at, int64_t out_end,
                                          int64_t total) {
    if constexpr (VEC) chan_emit4<WORDS>(c, src[0], src[1], src[2], src[3], at, out_end, total);
    else chan_emit1<WORDS>(c, src[0], at, out_end, total);
}

// k_collate_packed and its sibling with channels, k_collate_packed_ch, share this body: CH = false compiles every line
// about channels away, so the kernel that the plain add call launches is what it was.
template <int W, bool VEC, bool CH>
__device__ __forceinline__ void collate_packed_body(const PackArgs& a, const PackChans* ch) {
    __shared__ __attribute__((aligned(16))) int32_t s_d[SPAN + 4];  // marks (document - j0 at its sequence start), then their running maximum
    __shared__ __attribute__((aligned(16))) int32_t s_c[SPAN];  // (1 + where the position's sequence starts in the span) << 16 | starts so far
    __shared__ int32_t s_wmax[TB / 64], s_wcnt[TB / 64], s_wpos[TB / 64];
    __shared__ int32_t s_pre;
    __shared__ int64_t s_j[2];
    if (a.offs[0] != 0 || a.offs[a.n_docs] != a.n_ids) {
        if (blockIdx.x == 0 && threadIdx.x == 0) note_error(a.err, HUTK_E_ARG);
        return;
    }
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    if constexpr (CH) {
        // Offsets that decrease describe no ids either.  The ids' rows come out of the range-checked reads whatever the
        // offsets say, but a channel row is only as good as its offsets: every workgroup looks at its share of them.
        for (int64_t j = blk * TB + tid; j < a.n_docs; j += (int64_t)gridDim.x * TB)
            if (a.offs[j + 1] < a.offs[j]) note_error(a.err, HUTK_E_ARG);
    }
    int64_t k0, x0, x1;  // first row, first and one-past-last stream position of this workgroup
    if (a.spans_per_row > 1) {
        k0 = blk / a.spans_per_row;
        x0 = k0 * a.L + (blk - k0 * a.spans_per_row) * SPAN;
        x1 = x0 + SPAN < (k0 + 1) * a.L ? x0 + SPAN : (k0 + 1) * a.L;
    } else {
        k0 = blk * a.rows_per_block;
        x0 = k0 * a.L;
        x1 = x0 + a.rows_per_block * a.L;
    }
    if (x1 > a.total) x1 = a.total;
    if (x0 >= x1) return;
    const int32_t n = (int32_t)(x1 - x0);
    const int64_t row_start0 = k0 * a.L;

    for (int i = tid; i < SPAN + 4; i += TB) s_d[i] = 0;
    if (tid == 0) s_pre = 0;
    // the documents that hold the span's start and (when that is another place) the row's: a wavefront each, side by side
    if (tid < 64) {
        const int64_t j = last_doc_le(a, x0);
        if (tid == 0) s_j[0] = j;
    } else if (tid < 128 && x0 > row_start0) {
        const int64_t j = last_doc_le(a, row_start0);
        if (tid == 64) s_j[1] = j;
    }
    __syncthreads();
    const int64_t j0 = s_j[0];
    const int64_t b_j0 = j0 >= 0 ? a.P + a.offs[j0] + j0 * a.s : 0;

    // the sequence starts inside the span.  Empty sequences (s == 0, no ids) start nothing, so several empty documents at
    // one place cannot collide and the segment numbers stay dense.
    for (int64_t j = j0 + 1 + tid; j < a.n_docs; j += TB) {
        const int64_t o = a.offs[j];
        const int64_t b = a.P + o + j * a.s;
        if (b >= x1) break;
        if (b > x0 && (a.s > 0 || a.offs[j + 1] > o)) s_d[b - x0] = (int32_t)(j - j0);
    }
    // starts between the row's start and the span's: in the carry, and in the documents up to j0
    int32_t pre = 0;
    if (k0 == 0 && a.P > 0) pre = a.c_seg[a.P - 1] - 1;
    if (x0 > row_start0) {
        const int64_t jk = s_j[1];
        if (a.s > 0) pre += (int32_t)(j0 - jk);
        else {
            int32_t mine = 0;
            for (int64_t j = jk + 1 + tid; j <= j0; j += TB) mine += a.offs[j + 1] > a.offs[j];
            if (mine) atomicAdd(&s_pre, mine);
        }
    }
    __syncthreads();
    pre += s_pre;

    // workgroup scan over the marks: the running maximum of the marks (they grow along the span) and of the places they
    // stand at, and the running count
    {
        int32_t d[PER], c[PER];
        const int4 lo = *reinterpret_cast<const int4*>(&s_d[tid * PER]);
        const int4 hi = *reinterpret_cast<const int4*>(&s_d[tid * PER + 4]);
        d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w;
        d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
        int32_t m = 0, cnt = 0, at = 0;  // at: 1 + the place of the last mark, 0 when there is none yet
#pragma unroll
        for (int e = 0; e < PER; e++) {
            if (d[e] != 0) {
                m = d[e];
                at = tid * PER + e + 1;
                cnt++;
            }
            d[e] = m;
            c[e] = at << 16 | cnt;
        }
        const int lane = tid & 63, w = tid >> 6;
        int32_t tm = m, tc = cnt, tp = at;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t pm = __shfl_up(tm, off), pc = __shfl_up(tc, off), pp = __shfl_up(tp, off);
            if (lane >= off) {
                tm = pm > tm ? pm : tm;
                tp = pp > tp ? pp : tp;
                tc += pc;
            }
        }
        if (lane == 63) {
            s_wmax[w] = tm;
            s_wcnt[w] = tc;
            s_wpos[w] = tp;
        }
        int32_t em = __shfl_up(tm, 1), ec = __shfl_up(tc, 1), ep = __shfl_up(tp, 1);
        if (lane == 0) em = 0, ec = 0, ep = 0;
        __syncthreads();
        for (int u = 0; u < w; u++) {
            em = s_wmax[u] > em ? s_wmax[u] : em;
            ep = s_wpos[u] > ep ? s_wpos[u] : ep;
            ec += s_wcnt[u];
        }
#pragma unroll
        for (int e = 0; e < PER; e++) {
            d[e] = d[e] > em ? d[e] : em;
            const int32_t here = c[e] >> 16;
            c[e] = (here > ep ? here : ep) << 16 | ((c[e] & 0xFFFF) + ec);
        }
        *reinterpret_cast<int4*>(&s_d[tid * PER]) = make_int4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<int4*>(&s_d[tid * PER + 4]) = make_int4(d[4], d[5], d[6], d[7]);
        *reinterpret_cast<int4*>(&s_c[tid * PER]) = make_int4(c[0], c[1], c[2], c[3]);
        *reinterpret_cast<int4*>(&s_c[tid * PER + 4]) = make_int4(c[4], c[5], c[6], c[7]);
    }
    __syncthreads();

    // the elements, V neighbours per thread and consecutive threads on consecutive groups (full-width coalesced stores)
    constexpr int V = VEC ? 4 : 1;
    const bool multi = a.spans_per_row <= 1 && a.rows_per_block > 1;
    const int32_t Li = multi ? (int32_t)a.L : 0;
    const int64_t out_end = a.rows * a.L;
    for (int32_t i = tid * V; i < n; i += TB * V) {
        const int32_t rl = multi ? i / Li : 0;  // row inside the workgroup (V neighbours share it: L % 4 == 0 on that path)
        const int64_t row_start = row_start0 + (int64_t)rl * a.L;
        const int32_t seg_base = rl == 0 ? 1 + pre : 1 - (s_c[rl * Li] & 0xFFFF);
        int32_t vi[V], vp[V], vs[V];
        int64_t src[V];  // (CH only) where the element's channel records come from: chan_emit
#pragma unroll
        for (int e = 0; e < V; e++) {
            const int64_t gp = x0 + i + e;
            vi[e] = 0;
            vp[e] = 0;
            vs[e] = 0;
            if constexpr (CH) src[e] = -1;
            if (gp >= x1) continue;  // (only behind the stream's end: whole rows are multiples of V)
            if (gp < a.P) {
                vi[e] = a.c_ids[gp];
                vp[e] = a.c_pos[gp];
                vs[e] = a.c_seg[gp];
                if constexpr (CH) src[e] = -2 - gp;
                continue;
            }
            // No offsets are read here: the sequence's start is where its mark stood (or b_j0 for the one that reaches into
            // the span), it ends where the next mark stands, and the id's place follows from the stream position.
            const int32_t dd = s_d[i + e], cc = s_c[i + e];
            const int64_t j = j0 + dd;
            if (j < 0) {  // (offsets that do not describe the ids)
                note_error(a.err, HUTK_E_ARG);
                continue;
            }
            const int64_t b = dd ? x0 + (cc >> 16) - 1 : b_j0;
            bool last = false;  // of its sequence (asked only with an eos, when every document is a sequence)
            if (a.has_eos) {
                if (i + e + 1 < n) last = s_d[i + e + 1] != dd;
                else last = gp + 1 == (j + 1 < a.n_docs ? a.P + a.offs[j + 1] + (j + 1) * a.s : a.total);
            }
            if (a.has_bos && gp == b) vi[e] = a.bos;
            else if (last) vi[e] = a.eos;
            else {
                const int64_t idx = gp - a.P - j * a.s - a.has_bos;
                if (idx >= 0 && idx < a.n_ids) {
                    vi[e] = a.ids[idx];
                    if constexpr (CH) src[e] = idx;
                } else note_error(a.err, HUTK_E_ARG);
            }
            vp[e] = (int32_t)(gp - (b > row_start ? b : row_start));
            vs[e] = seg_base + (cc & 0xFFFF);
        }
        const int64_t at = x0 + i;
        if (at < out_end) {
            if constexpr (VEC) {
                store4<W>(a.out, at, vi);
                if (a.pos) *reinterpret_cast<int4*>(a.pos + at) = make_int4(vp[0], vp[1], vp[2], vp[3]);
                if (a.seg) *reinterpret_cast<int4*>(a.seg + at) = make_int4(vs[0], vs[1], vs[2], vs[3]);
            } else {
                store1<W>(a.out, at, vi[0]);
                if (a.pos) a.pos[at] = vp[0];
                if (a.seg) a.seg[at] = vs[0];
            }
        } else {  // behind the last whole row: the next call's carry
#pragma unroll
            for (int e = 0; e < V; e++) {
                const int64_t t = at + e - out_end;
                if (at + e < a.total) {
                    a.n_ids_out[t] = vi[e];
                    a.n_pos[t] = vp[e];
                    a.n_seg[t] = vs[e];
                }
            }
        }
        if constexpr (CH) {
#pragma unroll
            for (int k = 0; k < HUTK_PACKER_MAX_CHANNELS; k++) {
                if (k < ch->n) {
                    const PackChan c = ch->c[k];
                    if (c.words == 1) chan_emit<1, VEC>(c, src, at, out_end, a.total);
                    else if (c.words == 2) chan_emit<2, VEC>(c, src, at, out_end, a.total);
                    else chan_emit<4, VEC>(c, src, at, out_end, a.total);
                }
            }
        }
    }
}

template <int W, bool VEC>
__global__ __launch_bounds__(TB) void k_collate_packed(const PackArgs a) {
    collate_packed_body<W, VEC, false>(a, nullptr);
}

template <int W, bool VEC>
__global__ __launch_bounds__(TB) void k_collate_packed_ch(const PackArgs a, const PackChans ch) {
    collate_packed_body<W, VEC, true>(a, &ch);
}

// the carry as one padded row
template <int W>
__global__ __launch_bounds__(TB) void k_collate_flush(const int32_t* c_ids, const int32_t* c_pos, const int32_t* c_seg,
                                                      int64_t P, int64_t L, int32_t pad, void* out, int32_t* pos, int32_t* seg) {
    for (int64_t c = (int64_t)blockIdx.x * TB + threadIdx.x; c < L; c += (int64_t)gridDim.x * TB) {
        const bool in = c < P;
        store1<W>(out, c, in ? c_ids[c] : pad);
        if (pos) pos[c] = in ? c_pos[c] : 0;
        if (seg) seg[c] = in ? c_seg[c] : 0;
    }
}

// and its channels: carry first, then fill
template <int WORDS>
__device__ __forceinline__ void chan_flush(const PackChan& ch, int64_t c, bool in) {
    chan_store<WORDS>(ch.rows, c, ch.w8 != 0, in ? carry_load<WORDS>(ch.c_car, c) : make_int4(ch.f0, ch.f1, ch.f2, ch.f3));
}

__global__ __launch_bounds__(TB) void k_collate_flush_ch(const PackChans ch, int64_t P, int64_t L) {
    for (int64_t c = (int64_t)blockIdx.x * TB + threadIdx.x; c < L; c += (int64_t)gridDim.x * TB) {
#pragma unroll
        for (int k = 0; k < HUTK_PACKER_MAX_CHANNELS; k++) {
            if (k < ch.n) {
                const PackChan h = ch.c[k];
                if (h.words == 1) chan_flush<1>(h, c, c < P);
                else if (h.words == 2) chan_flush<2>(h, c, c < P);
                else chan_flush<4>(h, c, c < P);
            }
        }
    }
}

// ---- the rows scan --------------------------------------------------------------------------------------------------
// In the two windows forms item i (a document, a pair) gives rows(i) >= 1 rows, and row_offsets is the exclusive scan
// of rows: a count per workgroup, one k_scan_i64 launch over the workgroups' sums, and the write.  `Rows` is "rows of
// item i": rows(i, err) reports what is wrong with the item to err (NULL in the write: it was reported in the count).
constexpr int WIN_BLOCKS = 4096;  // most workgroups of the count: one k_scan_i64 launch scans their sums

struct ScanArgs {
    int64_t n;          // items
    int64_t per_block;  // items per workgroup, a multiple of TB
    int64_t* sums;      // [gridDim.x + 1]: the workgroups' row counts, then (launch_scan_i64) their exclusive scan and the sum
    int64_t* row_offs;
    int32_t* err;
};

template <class Rows>
__global__ __launch_bounds__(TB) void k_rows_count(const ScanArgs a, const Rows rows) {
    __shared__ int64_t s_part[TB / 64];
    const int64_t lo = (int64_t)blockIdx.x * a.per_block;
    const int64_t hi = lo + a.per_block < a.n ? lo + a.per_block : a.n;
    int64_t mine = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += TB) mine += rows(i, a.err);
    int64_t total;
    (void)hutk::block_excl(mine, s_part, total);
    if (threadIdx.x == 0) a.sums[blockIdx.x] = total;
}

template <class Rows>
__global__ __launch_bounds__(TB) void k_rows_write(const ScanArgs a, const Rows rows) {
    __shared__ int64_t s_part[TB / 64];
    const int64_t lo = (int64_t)blockIdx.x * a.per_block;
    const int64_t hi = lo + a.per_block < a.n ? lo + a.per_block : a.n;
    int64_t base = a.sums[blockIdx.x];
    for (int64_t at = lo; at < hi; at += TB) {  // (uniform: every thread meets the barriers of the scan)
        const int64_t i = at + threadIdx.x;
        const int64_t w = i < hi ? rows(i, nullptr) : 0;
        int64_t total;
        const int64_t before = hutk::block_excl(w, s_part, total);
        if (i < hi) a.row_offs[i] = base + before;
        base += total;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.row_offs[a.n] = a.sums[gridDim.x];
}

// The items of a tile's rows in the windows forms.  They are at most as many consecutive items as the tile has rows
// (row_offsets grows strictly), beginning with the last one whose first row is at or before the tile's first, which a
// wavefront finds.  Returns that item (at least 0) and stages row_offsets of it and the nd - 1 behind it, and of the one
// behind those, in s_ro; the caller's barrier makes them visible.  Every thread of the workgroup must call it.
__device__ __forceinline__ int64_t stage_items(const int64_t* row_offs, int64_t n, const RowTile& t, int64_t* s_ro,
                                               int64_t* s_d0, int32_t& nd) {
    if (threadIdx.x < 64) {
        const int64_t d = hutk::wave_count_leading(n, [&](int64_t i) { return row_offs[i] <= t.row0; }) - 1;
        if (threadIdx.x == 0) *s_d0 = d < 0 ? 0 : d;
    }
    __syncthreads();
    const int64_t d0 = *s_d0;
    nd = n - d0 < t.nrows ? (int32_t)(n - d0) : t.nrows;  // staged items, at least one
    for (int32_t i = threadIdx.x; i <= nd; i += TB) s_ro[i] = row_offs[d0 + i];
    return d0;
}

// the last of the nd staged items whose first row is at or before `row`
__device__ __forceinline__ int32_t staged_item_of_row(const int64_t* s_ro, int32_t nd, int64_t row) {
    int32_t lo = 0, hi = nd;
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (s_ro[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- chat ---------------------------------------------------------------------------------------------------------
// A render step between encode and collation (include/hutoken_amd.h): the turns of n_conv
// conversations, one encoded document each, become one sequence per conversation,
//     [bos]  prefix[role_t] content_t suffix[role_t]  (every turn t of the conversation)  tail
// with the loss labels, the turn index and the source index of every token.  T, the exclusive scan of the turns' rendered
// lengths, is one more instantiation of the rows scan (ChatTurns); the sequences' offsets follow from it in closed form,
// out_offsets[i] = T[conv[i]] + i * fixed with fixed = [bos] + |tail| (k_chat_offsets).  So turn t of conversation i
// begins at output position T[t] + i * fixed + [bos], and the fill has the packed layout's shape: a workgroup owns
// CHAT_SPAN output positions, one wavefront finds the span's first conversation on out_offsets and then, among that
// conversation's turns, the span's first turn on T; the starts of the sequences and of the turns inside the span are
// marked in LDS (empty ones mark nothing, so that several at one place cannot collide) and one workgroup scan turns the
// marks into "conversation of this position" and "turn of this position".
constexpr int CHAT_SPAN = 2048;           // output positions per workgroup (8 per thread in the scan, 4 in the stores)
constexpr int CHAT_PER = CHAT_SPAN / TB;

// The template as the kernels read it: in global memory behind a handle, staged into LDS by every workgroup of the fill
// (a kernel-argument array indexed at run time would live in scratch).  Words of 4 bytes throughout.
struct ChatTable {
    int32_t n_roles, bos, eos, max_part;  // bos / eos: HUTK_NO_TOKEN = absent; max_part: the largest |prefix| + |suffix|
    int32_t plen[HUTK_CHAT_MAX_ROLES], slen[HUTK_CHAT_MAX_ROLES], sloss[HUTK_CHAT_MAX_ROLES];
    int32_t prefix[HUTK_CHAT_MAX_ROLES][HUTK_CHAT_MAX_PART], suffix[HUTK_CHAT_MAX_ROLES][HUTK_CHAT_MAX_PART];
};
constexpr int CHAT_TABLE_WORDS = (int)(sizeof(ChatTable) / sizeof(int32_t));

// "rendered length of turn t" for the rows scan.  A role outside the template or a length that cannot be is reported and
// counts as 0: the turn is left out.
struct ChatTurns {
    const ChatTable* tab;
    const int64_t* offs;
    const int32_t* roles;
    int64_t n_turns, n_ids;
    __device__ int64_t operator()(int64_t t, int32_t* err) const {
        if (t == 0 && (offs[0] != 0 || offs[n_turns] != n_ids)) note_error(err, HUTK_E_ARG);
        const int32_t r = roles[t];
        const int64_t n = offs[t + 1] - offs[t];
        if (r < 0 || r >= tab->n_roles || n < 0 || n > n_ids) {
            note_error(err, HUTK_E_ARG);
            return 0;
        }
        return tab->plen[r] + n + tab->slen[r];
    }
};

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

struct ChatOffArgs {
    const int64_t* conv;  // [n_conv + 1] into the turns
    const int64_t* T;     // [n_turns + 1]
    int64_t n_conv, n_turns, fixed;
    int64_t* oo;          // [n_conv + 1]
    int32_t* err;
};

// One thread per entry of out_offsets.  conv must rise from 0 to n_turns; an entry that does not is reported and read
// as the nearest turn there is.
__global__ __launch_bounds__(TB) void k_chat_offsets(const ChatOffArgs a) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i > a.n_conv) return;
    const int64_t c = a.conv[i];
    if (c < 0 || c > a.n_turns || (i == 0 && c != 0) || (i == a.n_conv && c != a.n_turns) || (i < a.n_conv && a.conv[i + 1] < c))
        note_error(a.err, HUTK_E_ARG);
    a.oo[i] = a.T[clamp_i64(c, 0, a.n_turns)] + i * a.fixed;
}

struct ChatArgs {
    const ChatTable* tab;
    const int32_t* ids;
    const int64_t* offs;   // [n_turns + 1] into ids
    const int32_t* roles;  // [n_turns]
    const int64_t* conv;   // [n_conv + 1] into the turns
    const int64_t* T;      // [n_turns + 1]: turn_offsets
    const int64_t* oo;     // [n_conv + 1]: out_offsets
    int64_t n_conv, n_turns, n_ids, out_cap;
    int32_t gen_role, has_bos, tail_len, fixed;
    uint32_t loss_roles;
    int32_t ignore;
    int32_t *out_ids, *labels, *turn_ids;  // turn_ids: may be NULL
    int64_t* src;                          // may be NULL
    int32_t* err;
    int32_t wide;  // bit 0 out_ids, 1 labels, 2 turn_ids, 3 src: the pointer is 16-byte aligned
};

// up to four neighbouring elements at element index `at` (a multiple of 4): one 16-byte store where the array allows
__device__ __forceinline__ void chat_store(int32_t* base, bool wide, int64_t at, int cnt, const int32_t (&v)[4]) {
    if (wide && cnt == 4) *reinterpret_cast<int4*>(base + at) = make_int4(v[0], v[1], v[2], v[3]);
    else
        for (int e = 0; e < cnt; e++) base[at + e] = v[e];
}
__device__ __forceinline__ void chat_store(int64_t* base, bool wide, int64_t at, int cnt, const int64_t (&v)[4]) {
    if (wide && cnt == 4) {
        longlong2* p = reinterpret_cast<longlong2*>(base + at);
        p[0] = make_longlong2(v[0], v[1]);
        p[1] = make_longlong2(v[2], v[3]);
    } else
        for (int e = 0; e < cnt; e++) base[at + e] = v[e];
}

// Nothing is trusted: every index into conv, T, offs, roles, ids and the table is checked before it is used, the marks
// lie inside the span by construction, and a position is written only below min(n_out, out_cap).  What does not fit is
// reported with HUTK_E_ARG and leaves id 0, ignore_index, -1, -1 at its place.
__global__ __launch_bounds__(TB) void k_chat_render(const ChatArgs a) {
    __shared__ __attribute__((aligned(16))) int32_t s_t[CHAT_SPAN];  // marks (turn - t0 at its start), then their running maximum
    __shared__ __attribute__((aligned(16))) int32_t s_c[CHAT_SPAN];  // the same for the conversations (conversation - i0)
    __shared__ ChatTable s_tab;
    __shared__ int32_t s_wt[TB / 64], s_wc[TB / 64];
    __shared__ int64_t s_first[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (a.offs[0] != 0 || a.offs[a.n_turns] != a.n_ids) {  // nothing is read through offsets that do not fit the ids
        if (blockIdx.x == 0 && tid == 0) note_error(a.err, HUTK_E_ARG);
        return;
    }
    const int64_t n_out = a.oo[a.n_conv];
    if (blockIdx.x == 0 && tid == 0) {
        if (a.oo[0] != 0 || a.T[0] != 0 || n_out != a.T[a.n_turns] + a.n_conv * (int64_t)a.fixed) note_error(a.err, HUTK_E_ARG);
        if (n_out > a.out_cap) note_error(a.err, HUTK_E_CAPACITY);
    }
    const int64_t x0 = (int64_t)blockIdx.x * CHAT_SPAN;
    int64_t x1 = x0 + CHAT_SPAN;
    if (x1 > n_out) x1 = n_out;
    if (x1 > a.out_cap) x1 = a.out_cap;
    if (x0 >= x1) return;
    const int32_t n = (int32_t)(x1 - x0);

    for (int i = tid; i < CHAT_TABLE_WORDS; i += TB) reinterpret_cast<int32_t*>(&s_tab)[i] = reinterpret_cast<const int32_t*>(a.tab)[i];
    for (int i = tid; i < CHAT_SPAN; i += TB) s_t[i] = 0, s_c[i] = 0;
    // The last conversation that begins at or before the span's start -- of several at one place (empty ones, without
    // bos and tail) the last, the one the position belongs to -- and then the last of ITS turns that begins at or before
    // it (the turn before its first when none does: the span starts on its bos).  The second search needs the first
    // one's answer, so one wavefront does both.
    if (tid < 64) {
        int64_t i0 = hutk::wave_count_leading(a.n_conv, [&](int64_t i) { return a.oo[i] <= x0; }) - 1;
        if (i0 < 0) i0 = 0;  // (out_offsets[0] != 0: reported above)
        const int64_t c0 = clamp_i64(a.conv[i0], 0, a.n_turns), c1 = clamp_i64(a.conv[i0 + 1], c0, a.n_turns);
        const int64_t y = x0 - i0 * a.fixed - a.has_bos;
        const int64_t k = hutk::wave_count_leading(c1 - c0, [&](int64_t k) { return a.T[c0 + k] <= y; });
        if (tid == 0) s_first[0] = i0, s_first[1] = c0 + k - 1;
    }
    __syncthreads();
    const int64_t i0 = s_first[0], t0 = s_first[1];

    // The starts inside the span: a wavefront per conversation, its lanes over the conversation's turns.  Empty turns
    // and empty sequences mark nothing.
    for (int64_t i = i0 + w; i < a.n_conv; i += TB / 64) {
        const int64_t o = a.oo[i];
        if (i > i0 && o >= x1) break;
        const int64_t c0 = clamp_i64(a.conv[i], 0, a.n_turns), c1 = clamp_i64(a.conv[i + 1], c0, a.n_turns);
        if (i > i0 && o > x0 && lane == 0 && a.oo[i + 1] > o) s_c[o - x0] = (int32_t)(i - i0);
        const int64_t shift = i * a.fixed + a.has_bos;
        for (int64_t t = (i == i0 ? t0 + 1 : c0) + lane; t < c1; t += 64) {
            const int64_t Tt = a.T[t], S = Tt + shift;
            if (S >= x1) break;
            if (S > x0 && a.T[t + 1] > Tt) s_t[S - x0] = (int32_t)(t - t0);
        }
    }
    __syncthreads();

    // workgroup scan over the marks: the running maximum of both (they grow along the span)
    {
        int32_t dt[CHAT_PER], dc[CHAT_PER];
        const int4 tl = *reinterpret_cast<const int4*>(&s_t[tid * CHAT_PER]), th = *reinterpret_cast<const int4*>(&s_t[tid * CHAT_PER + 4]);
        const int4 cl = *reinterpret_cast<const int4*>(&s_c[tid * CHAT_PER]), ch = *reinterpret_cast<const int4*>(&s_c[tid * CHAT_PER + 4]);
        dt[0] = tl.x; dt[1] = tl.y; dt[2] = tl.z; dt[3] = tl.w; dt[4] = th.x; dt[5] = th.y; dt[6] = th.z; dt[7] = th.w;
        dc[0] = cl.x; dc[1] = cl.y; dc[2] = cl.z; dc[3] = cl.w; dc[4] = ch.x; dc[5] = ch.y; dc[6] = ch.z; dc[7] = ch.w;
        int32_t mt = 0, mc = 0;
#pragma unroll
        for (int e = 0; e < CHAT_PER; e++) {
            mt = dt[e] > mt ? dt[e] : mt;
            mc = dc[e] > mc ? dc[e] : mc;
            dt[e] = mt;
            dc[e] = mc;
        }
        const int32_t tt = hutk::wave_incl_max(mt, lane), tc = hutk::wave_incl_max(mc, lane);
        if (lane == 63) s_wt[w] = tt, s_wc[w] = tc;
        int32_t et = __shfl_up(tt, 1), ec = __shfl_up(tc, 1);
        if (lane == 0) et = 0, ec = 0;
        __syncthreads();
        for (int u = 0; u < w; u++) {
            et = s_wt[u] > et ? s_wt[u] : et;
            ec = s_wc[u] > ec ? s_wc[u] : ec;
        }
#pragma unroll
        for (int e = 0; e < CHAT_PER; e++) {
            dt[e] = dt[e] > et ? dt[e] : et;
            dc[e] = dc[e] > ec ? dc[e] : ec;
        }
        *reinterpret_cast<int4*>(&s_t[tid * CHAT_PER]) = make_int4(dt[0], dt[1], dt[2], dt[3]);
        *reinterpret_cast<int4*>(&s_t[tid * CHAT_PER + 4]) = make_int4(dt[4], dt[5], dt[6], dt[7]);
        *reinterpret_cast<int4*>(&s_c[tid * CHAT_PER]) = make_int4(dc[0], dc[1], dc[2], dc[3]);
        *reinterpret_cast<int4*>(&s_c[tid * CHAT_PER + 4]) = make_int4(dc[4], dc[5], dc[6], dc[7]);
    }
    __syncthreads();

    // The elements, four neighbours per thread and consecutive threads on consecutive groups.  A thread reads what it
    // needs of a conversation (five words) and of a turn (five words) when it meets another one, which among four
    // neighbours is rare; a position is then a few comparisons against them and at most one id.
    const int32_t n_roles = s_tab.n_roles;
    for (int32_t p = tid * 4; p < n; p += TB * 4) {
        int32_t vi[4], vl[4], vt[4];
        int64_t vs[4];
        int64_t ci = -1, ct = -2;           // the conversation and the turn held in registers
        int64_t o = 0, c0 = 0, c1 = 0, A = 0, R = 0;            // conversation: its start, its turns, T at its first turn, its turns' length
        int64_t ts = 0, tlen = 0, off0 = 0, nt = 0;             // turn: its start behind A, its rendered length, its ids
        int32_t role = -1, pl = 0, sl = 0, sloss = 0;
        bool loss = false;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            vi[e] = 0;
            vl[e] = a.ignore;
            vt[e] = -1;
            vs[e] = -1;
            if (p + e >= n) continue;
            const int64_t x = x0 + p + e;
            const int64_t i = i0 + s_c[p + e];
            if (i != ci) {
                ci = i;
                o = a.oo[i];
                c0 = clamp_i64(a.conv[i], 0, a.n_turns);
                c1 = clamp_i64(a.conv[i + 1], c0, a.n_turns);
                A = a.T[c0];
                R = a.T[c1] - A;
            }
            const int64_t q = x - o;
            if (q < 0) {
                note_error(a.err, HUTK_E_ARG);
                continue;
            }
            if (a.has_bos && q == 0) {
                vi[e] = s_tab.bos;
                continue;
            }
            const int64_t yy = q - a.has_bos;  // behind the bos: the turns, then the tail
            if (yy >= R) {
                const int64_t k = yy - R;
                if (k < a.tail_len) vi[e] = a.gen_role >= 0 ? s_tab.prefix[a.gen_role][k] : s_tab.eos;
                else note_error(a.err, HUTK_E_ARG);
                continue;
            }
            const int64_t t = t0 + s_t[p + e];
            if (t < c0 || t >= c1) {
                note_error(a.err, HUTK_E_ARG);
                continue;
            }
            if (t != ct) {
                ct = t;
                const int64_t Tt = a.T[t];
                ts = Tt - A;
                tlen = a.T[t + 1] - Tt;
                off0 = a.offs[t];
                nt = a.offs[t + 1] - off0;
                role = a.roles[t];
                if (role < 0 || role >= n_roles) role = -1;
                else {
                    pl = s_tab.plen[role];
                    sl = s_tab.slen[role];
                    sloss = s_tab.sloss[role];
                    loss = (a.loss_roles >> role) & 1u;
                }
            }
            const int64_t u = yy - ts;  // inside the turn: prefix, content, suffix
            if (role < 0 || u < 0 || u >= tlen) {
                note_error(a.err, HUTK_E_ARG);
                continue;
            }
            vt[e] = (int32_t)(t - c0);
            if (u < pl) vi[e] = s_tab.prefix[role][u];
            else if (u - pl < nt) {
                const int64_t idx = off0 + u - pl;
                if (idx >= 0 && idx < a.n_ids) {
                    vi[e] = a.ids[idx];
                    vs[e] = idx;
                    if (loss) vl[e] = vi[e];
                } else note_error(a.err, HUTK_E_ARG);
            } else {
                const int64_t v = u - pl - nt;
                if (v >= 0 && v < sl) {
                    vi[e] = s_tab.suffix[role][v];
                    if (loss && v < sloss) vl[e] = vi[e];
                } else note_error(a.err, HUTK_E_ARG);
            }
        }
        const int64_t at = x0 + p;
        const int cnt = n - p < 4 ? n - p : 4;
        chat_store(a.out_ids, a.wide & 1, at, cnt, vi);
        chat_store(a.labels, a.wide & 2, at, cnt, vl);
        if (a.turn_ids) chat_store(a.turn_ids, a.wide & 4, at, cnt, vt);
        if (a.src) chat_store(a.src, a.wide & 8, at, cnt, vs);
    }
}

// ---- fill-in-the-middle ---------------------------------------------------------------------------------------------
// A render step between encode and collation, like the chat render (include/hutoken_amd.h): a
// document is cut into prefix / middle / suffix and re-ordered behind three sentinels (hutk_fim.h holds the rule).  The
// cuts are drawn per document at token level (FimDocs with kinds_in == NULL), or were drawn on the packed text before
// the encode (k_fim_cut) and are read back from the offsets of the 3 n_docs encoded pieces (kinds_in given).
// out_offsets, the exclusive scan of the rendered lengths, is one more instantiation of the rows scan (FimDocs); the
// plan row (src0, n, lo, hi) and the kind of every document are written by one thread each (k_fim_plan); the fill has
// the chat render's shape with ONE level of search: a workgroup owns FIM_SPAN output positions, one wavefront finds the
// span's first document on out_offsets, the documents that start inside the span are marked in LDS (empty ones mark
// nothing) and one workgroup scan turns the marks into "document of this position".
constexpr int FIM_SPAN = 2048;  // output positions per workgroup (8 per thread in the scan, 4 in the stores)
constexpr int FIM_PER = FIM_SPAN / TB;

struct FimDoc {
    int32_t kind;
    int64_t src0, n, lo, hi;
};

// Document i as the plan sees it, and "rendered length of document i" for the rows scan.  What cannot be (offsets that
// decrease or leave the ids, a kind outside 0 .. 2) is reported and gives a plain document of no ids: it is left out.
struct FimDocs {
    const int64_t* offs;      // tokens: [n_docs + 1] into the ids; pieces: [3 n_docs + 1]
    const int32_t* kinds_in;  // NULL: token level, the cuts are drawn here
    int64_t n_docs, n_ids, first_doc;
    uint64_t seed, fim_below, spm_below;
    int32_t E;
    __device__ FimDoc doc(int64_t i, int32_t* err) const {
        FimDoc d{hutk::FIM_PLAIN, 0, 0, 0, 0};
        if (!kinds_in) {
            if (i == 0 && (offs[0] != 0 || offs[n_docs] != n_ids)) note_error(err, HUTK_E_ARG);
            const int64_t a = offs[i], n = offs[i + 1] - a;
            if (a < 0 || n < 0 || a > n_ids || n > n_ids - a) {
                note_error(err, HUTK_E_ARG);
                return d;
            }
            const hutk::FimCut c = hutk::fim_decide(seed, first_doc + i, n, fim_below, spm_below);
            return FimDoc{c.kind, a, n, c.lo, c.hi};
        }
        if (i == 0 && (offs[0] != 0 || offs[3 * n_docs] != n_ids)) note_error(err, HUTK_E_ARG);
        const int64_t a = offs[3 * i], b = offs[3 * i + 1], c = offs[3 * i + 2], e = offs[3 * i + 3];
        const int32_t kind = kinds_in[i];
        if (a < 0 || b < a || c < b || e < c || e > n_ids || kind < hutk::FIM_PLAIN || kind > hutk::FIM_SPM) {
            note_error(err, HUTK_E_ARG);
            return d;
        }
        return FimDoc{kind, a, e - a, b - a, c - a};
    }
    __device__ int64_t operator()(int64_t i, int32_t* err) const {
        const FimDoc d = doc(i, err);
        return hutk::fim_length(d.n, d.kind, E);
    }
};

// One thread per document: its plan row and, at token level, its kind.  (The scan in front of it has reported what is
// wrong with a document.)
__global__ __launch_bounds__(TB) void k_fim_plan(const FimDocs docs, int64_t* plan, int32_t* kinds_out) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= docs.n_docs) return;
    const FimDoc d = docs.doc(i, nullptr);
    plan[4 * i] = d.src0;
    plan[4 * i + 1] = d.n;
    plan[4 * i + 2] = d.lo;
    plan[4 * i + 3] = d.hi;
    if (kinds_out) kinds_out[i] = d.kind;
}

struct FimCutArgs {
    const uint8_t* bytes;
    const int64_t* offs;  // [n_docs + 1] into the bytes
    int64_t n_docs, n_bytes, first_doc;
    uint64_t seed, fim_below, spm_below;
    int64_t* pieces;  // [3 n_docs + 1]
    int32_t* kinds;   // [n_docs]
    int32_t* err;
};

// a cut of a document of `len` bytes at `base`, moved back to the start of its UTF-8 character: at most three steps
__device__ __forceinline__ int64_t fim_char_start(const uint8_t* base, int64_t len, int64_t pos) {
#pragma unroll
    for (int step = 0; step < 3; step++) {
        if (pos <= 0 || pos >= len || (base[pos] & 0xC0) != 0x80) break;
        pos--;
    }
    return pos;
}

// The text cut, one thread per document: the draw, at most six byte reads, four stores.  A document whose offsets cannot
// be is reported and counted as plain with length 0.
__global__ __launch_bounds__(TB) void k_fim_cut(const FimCutArgs a) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= a.n_docs) return;
    if (i == 0) {
        if (a.offs[0] != 0 || a.offs[a.n_docs] != a.n_bytes) note_error(a.err, HUTK_E_ARG);
        a.pieces[3 * a.n_docs] = a.n_bytes;
    }
    int64_t s = a.offs[i], len = a.offs[i + 1] - s;
    if (s < 0 || len < 0 || s > a.n_bytes || len > a.n_bytes - s) {
        note_error(a.err, HUTK_E_ARG);
        s = clamp_i64(s, 0, a.n_bytes);
        len = 0;
    }
    const hutk::FimCut c = hutk::fim_decide(a.seed, a.first_doc + i, len, a.fim_below, a.spm_below);
    int64_t lo = c.lo, hi = c.hi;
    if (c.kind != hutk::FIM_PLAIN) {
        lo = fim_char_start(a.bytes + s, len, lo);
        hi = fim_char_start(a.bytes + s, len, hi);
    }
    a.pieces[3 * i] = s;
    a.pieces[3 * i + 1] = s + lo;
    a.pieces[3 * i + 2] = s + hi;
    a.kinds[i] = c.kind;
}

struct FimArgs {
    const int32_t* ids;
    const int64_t* plan;   // [n_docs][4]: src0, n, lo, hi
    const int32_t* kinds;  // [n_docs]
    const int64_t* oo;     // [n_docs + 1]: out_offsets
    int64_t n_docs, n_ids, out_cap;
    int32_t pre, suf, mid, end, E;
    uint32_t loss_parts;
    int32_t ignore;
    int32_t *out_ids, *labels, *parts;  // labels, parts: may be NULL
    int64_t* src;                       // may be NULL
    int32_t* err;
    int32_t wide;  // bit 0 out_ids, 1 labels, 2 parts, 3 src: the pointer is 16-byte aligned
};

// A plan row and a kind that fit the ids: 0 <= lo <= hi <= n, the document inside ids[0, n_ids), a kind of 0 .. 2.
__device__ __forceinline__ bool fim_doc_fits(const FimDoc& d, int64_t n_ids) {
    return d.kind >= hutk::FIM_PLAIN && d.kind <= hutk::FIM_SPM && d.lo >= 0 && d.lo <= d.hi && d.hi <= d.n && d.src0 >= 0 &&
           d.src0 <= n_ids && d.n <= n_ids - d.src0;
}

// Nothing is trusted: every index into out_offsets, the plan, the kinds and the ids is checked before it is used, the
// marks lie inside the span by construction, and a position is written only below min(n_out, out_cap).  What does not
// fit is reported with HUTK_E_ARG and leaves id 0, ignore_index, part -1, source -1 at its place.
__global__ __launch_bounds__(TB) void k_fim_render(const FimArgs a) {
    __shared__ __attribute__((aligned(16))) int32_t s_d[FIM_SPAN];  // marks (document - i0 at its start), then their running maximum
    __shared__ int32_t s_w[TB / 64];
    __shared__ int64_t s_first;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t n_out = a.oo[a.n_docs];
    if (blockIdx.x == 0 && tid == 0) {
        if (a.oo[0] != 0) note_error(a.err, HUTK_E_ARG);
        if (n_out > a.out_cap) note_error(a.err, HUTK_E_CAPACITY);
    }
    const int64_t x0 = (int64_t)blockIdx.x * FIM_SPAN;
    int64_t x1 = x0 + FIM_SPAN;
    if (x1 > n_out) x1 = n_out;
    if (x1 > a.out_cap) x1 = a.out_cap;
    if (x0 >= x1) return;
    const int32_t n = (int32_t)(x1 - x0);

    for (int i = tid; i < FIM_SPAN; i += TB) s_d[i] = 0;
    // the last document that begins at or before the span's start: of several at one place (empty ones) the last, the
    // one the position belongs to
    if (tid < 64) {
        const int64_t i0 = hutk::wave_count_leading(a.n_docs, [&](int64_t i) { return a.oo[i] <= x0; }) - 1;
        if (tid == 0) s_first = i0 < 0 ? 0 : i0;  // (out_offsets[0] != 0: reported above)
    }
    __syncthreads();
    const int64_t i0 = s_first;

    // The starts inside the span, a thread per document.  Empty sequences mark nothing.  Here every document that starts
    // in (x0, x1] is also held against out_offsets: its rendered length must be the distance to the next start.
    for (int64_t i = i0 + 1 + tid; i < a.n_docs; i += TB) {
        const int64_t o = a.oo[i];
        if (o > x1) break;
        const int64_t len = a.oo[i + 1] - o;
        const int32_t kind = a.kinds[i];
        if (kind < hutk::FIM_PLAIN || kind > hutk::FIM_SPM || len != hutk::fim_length(a.plan[4 * i + 1], kind, a.E)) note_error(a.err, HUTK_E_ARG);
        if (o > x0 && o < x1 && len > 0) s_d[o - x0] = (int32_t)(i - i0);
    }
    __syncthreads();

    // workgroup scan over the marks: their running maximum (they grow along the span)
    {
        int32_t d[FIM_PER];
        const int4 dl = *reinterpret_cast<const int4*>(&s_d[tid * FIM_PER]), dh = *reinterpret_cast<const int4*>(&s_d[tid * FIM_PER + 4]);
        d[0] = dl.x; d[1] = dl.y; d[2] = dl.z; d[3] = dl.w; d[4] = dh.x; d[5] = dh.y; d[6] = dh.z; d[7] = dh.w;
        int32_t m = 0;
#pragma unroll
        for (int e = 0; e < FIM_PER; e++) {
            m = d[e] > m ? d[e] : m;
            d[e] = m;
        }
        const int32_t t = hutk::wave_incl_max(m, lane);
        if (lane == 63) s_w[w] = t;
        int32_t before = __shfl_up(t, 1);
        if (lane == 0) before = 0;
        __syncthreads();
        for (int u = 0; u < w; u++) before = s_w[u] > before ? s_w[u] : before;
#pragma unroll
        for (int e = 0; e < FIM_PER; e++) d[e] = d[e] > before ? d[e] : before;
        *reinterpret_cast<int4*>(&s_d[tid * FIM_PER]) = make_int4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<int4*>(&s_d[tid * FIM_PER + 4]) = make_int4(d[4], d[5], d[6], d[7]);
    }
    __syncthreads();

    // The elements, four neighbours per thread and consecutive threads on consecutive groups.  A thread reads a
    // document's two offsets, plan row and kind when it meets another document, which among four neighbours is rare; a
    // position is then a few comparisons (fim_locate) and at most one id.
    for (int32_t p = tid * 4; p < n; p += TB * 4) {
        int32_t vi[4], vl[4], vp[4];
        int64_t vs[4];
        int64_t ci = -1, o = 0, len = 0;  // the document held in registers: its start and its rendered length
        FimDoc d{0, 0, 0, 0, 0};
        bool fits = false;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            vi[e] = 0;
            vl[e] = a.ignore;
            vp[e] = -1;
            vs[e] = -1;
            if (p + e >= n) continue;
            const int64_t i = i0 + s_d[p + e];
            if (i != ci) {
                ci = i;
                fits = i >= 0 && i < a.n_docs;
                if (fits) {
                    o = a.oo[i];
                    d = FimDoc{a.kinds[i], a.plan[4 * i], a.plan[4 * i + 1], a.plan[4 * i + 2], a.plan[4 * i + 3]};
                    fits = fim_doc_fits(d, a.n_ids);
                    len = fits ? hutk::fim_length(d.n, d.kind, a.E) : 0;
                    if (fits && a.oo[i + 1] - o != len) note_error(a.err, HUTK_E_ARG);  // (out_offsets is not the scan)
                }
            }
            const int64_t q = x0 + p + e - o;
            const hutk::FimPlace at = fits ? hutk::fim_locate(d.n, d.lo, d.hi, d.kind, a.E, q) : hutk::FimPlace{-1, -1};
            if (at.part < 0) {
                note_error(a.err, HUTK_E_ARG);
                continue;
            }
            if (at.part == hutk::FIM_PART_SENTINEL) {
                vi[e] = at.v == hutk::FIM_PRE ? a.pre : at.v == hutk::FIM_SUF ? a.suf : at.v == hutk::FIM_MID ? a.mid : a.end;
            } else {
                const int64_t idx = d.src0 + at.v;  // (inside the ids: the document is, and v < n)
                vi[e] = a.ids[idx];
                vs[e] = idx;
            }
            vp[e] = at.part;
            const bool end_loss = at.part == hutk::FIM_PART_SENTINEL && at.v == hutk::FIM_END && (a.loss_parts & HUTK_FIM_LOSS_END);
            if (((a.loss_parts >> at.part) & 1u) || end_loss) vl[e] = vi[e];
        }
        const int64_t at = x0 + p;
        const int cnt = n - p < 4 ? n - p : 4;
        chat_store(a.out_ids, a.wide & 1, at, cnt, vi);
        if (a.labels) chat_store(a.labels, a.wide & 2, at, cnt, vl);
        if (a.parts) chat_store(a.parts, a.wide & 4, at, cnt, vp);
        if (a.src) chat_store(a.src, a.wide & 8, at, cnt, vs);
    }
}

// ---- windows ------------------------------------------------------------------------------------------------------
// Document i of n ids gives w(n) rows: one when n <= C (C = L - s ids fit a row), else 1 + ceil((n - C) / step) with
// step = C - stride; row k of it holds the document's ids [k * step, min(k * step + C, n)).  A length that cannot be
// (negative, above n_ids) is reported and counted as the nearest that can.
__device__ __forceinline__ int64_t window_count(int64_t dl, int64_t n_ids, int64_t C, int64_t step, int32_t* err) {
    if (dl < 0 || dl > n_ids) {
        note_error(err, HUTK_E_ARG);
        dl = dl < 0 ? 0 : n_ids;
    }
    return dl <= C ? 1 : 1 + (dl - C + step - 1) / step;
}

struct DocRows {
    const int64_t* offs;
    int64_t n_docs, n_ids;
    int64_t C, step;
    __device__ int64_t operator()(int64_t i, int32_t* err) const {
        if (i == 0 && (offs[0] != 0 || offs[n_docs] != n_ids)) note_error(err, HUTK_E_ARG);
        return window_count(offs[i + 1] - offs[i], n_ids, C, step, err);
    }
};

// Row `row` among the nd staged documents (stage_items; s_off: their offsets): which one (behind the first staged),
// where its window starts inside the document and how many ids it holds.  A length or a row_offsets that cannot be is
// reported and gives an empty row.  What k_collate_windows and k_plan_windows both place a row with.
__device__ __forceinline__ int32_t window_row(const int64_t* s_ro, const int64_t* s_off, int32_t nd, int64_t row, int64_t cap,
                                              int32_t C, int32_t step, int32_t* err, int64_t& start, int32_t& n) {
    const int32_t lo = staged_item_of_row(s_ro, nd, row);
    int64_t dl = s_off[lo + 1] - s_off[lo];
    const int64_t k = row - s_ro[lo];
    bool bad = dl < 0 || dl > cap;
    if (bad) dl = 0;
    if (k < 0 || k >= window_count(dl, cap, C, step, nullptr)) bad = true;  // (a row_offsets that is not the scan of w)
    start = 0;
    n = 0;
    if (bad) note_error(err, HUTK_E_ARG);
    else {
        start = k * step;  // < dl: no overflow
        n = dl - start < C ? (int32_t)(dl - start) : C;
    }
    return lo;
}

struct WinArgs {
    RowArgs r;  // (ids_a, cap_a: the ids and their number)
    const int64_t* offs;
    const int64_t* rows;  // row_offsets
    int64_t n_docs, n_rows;
    int32_t C, step;
};

// The planner: the tile's documents are found and staged (stage_items) with their offsets, and thread r places row r
// among them once.  Whatever row_offsets and offsets hold, every index stays inside the staged entries and d_ids.
template <int W, bool VEC>
__global__ __launch_bounds__(TB) void k_collate_windows(const WinArgs a) {
    __shared__ int64_t s_ro[PAD_ROWS + 1], s_off[PAD_ROWS + 1];
    __shared__ int64_t s_start[PAD_ROWS];  // of the row's window inside its document
    __shared__ int32_t s_j[PAD_ROWS], s_n[PAD_ROWS];  // the row's document (behind the first staged one), its window's ids
    __shared__ int64_t s_d0;
    if (a.offs[0] != 0 || a.offs[a.n_docs] != a.r.cap_a || a.rows[0] != 0 || a.rows[a.n_docs] != a.n_rows) {
        if (blockIdx.x == 0 && threadIdx.x == 0) note_error(a.r.err, HUTK_E_ARG);
        return;
    }
    const int tid = threadIdx.x;
    const RowTile t = row_tile(a.r, a.n_rows);
    if (t.nrows <= 0) return;
    int32_t nd;
    const int64_t d0 = stage_items(a.rows, a.n_docs, t, s_ro, &s_d0, nd);
    for (int32_t i = tid; i <= nd; i += TB) s_off[i] = a.offs[d0 + i];
    __syncthreads();
    if (tid < t.nrows) {
        int64_t start;
        int32_t n;
        s_j[tid] = window_row(s_ro, s_off, nd, t.row0 + tid, a.r.cap_a, a.C, a.step, a.r.err, start, n);
        s_start[tid] = start;
        s_n[tid] = n;
    }
    __syncthreads();
    write_rows<W, VEC, false>(a.r, t, [&](int32_t rl) {
        const int32_t j = s_j[rl];
        RowPlan p{};
        p.ka = s_n[rl];
        p.start = s_start[rl];
        p.srca = s_off[j] + p.start - a.r.has_bos;
        p.item = d0 + j;
        return p;
    });
}

// ---- pairs --------------------------------------------------------------------------------------------------------
// Row i is [bos] A' sep.. B' [eos] of document i of two ragged pairs.  With R = L - s ids of room
// (s: bos, the separators, eos) the kept lengths (ka, kb) follow the truncation strategy; in the windows form the named
// side is cut into windows of C = R - (ids kept of the other side) and row_offsets is the exclusive scan of the pairs'
// window counts.  Either side's offsets may begin anywhere in its ids: document i of side X is valid when
// 0 <= offsets_x[i] <= offsets_x[i + 1] <= cap_x; any other is reported and counts as empty.
__device__ __forceinline__ int64_t side_len(int64_t o0, int64_t o1, int64_t cap, int32_t* err) {
    if (o0 < 0 || o1 < o0 || o1 > cap) {
        note_error(err, HUTK_E_ARG);
        return 0;
    }
    return o1 - o0;
}

// the ids of A and B that stay in one row of R; longest_first is the closed form, not a loop
__device__ __forceinline__ void pair_lengths(int64_t na, int64_t nb, int64_t R, int strategy, int32_t& ka, int32_t& kb) {
    if (na + nb > R) {
        if (strategy == HUTK_PAIR_ONLY_FIRST) {
            nb = nb < R ? nb : R;
            na = na < R - nb ? na : R - nb;
        } else if (strategy == HUTK_PAIR_ONLY_SECOND) {
            na = na < R ? na : R;
            nb = nb < R - na ? nb : R - na;
        } else {
            const bool swap = na > nb;
            int64_t n1 = swap ? nb : na, n2;  // the shorter and the longer side
            n2 = n1 > R ? n1 : n1 > R - n1 ? n1 : R - n1;
            if (n1 + n2 > R) {
                n1 = R / 2;
                n2 = n1 + R % 2;  // the longer side gets the odd id; on a tie that is B
            }
            na = swap ? n2 : n1;
            nb = swap ? n1 : n2;
        }
    }
    ka = (int32_t)na;
    kb = (int32_t)nb;
}

// rows of one pair in the windows form: the cut side has n ids, the other one no.  C: the cut side's room per row
__device__ __forceinline__ int64_t pair_window_count(int64_t n, int64_t no, int64_t R, int64_t stride, int64_t& C, int64_t& step) {
    C = R - (no < R ? no : R);
    step = C - stride > 1 ? C - stride : 1;
    return n <= C || C == 0 ? 1 : 1 + (n - C + step - 1) / step;
}

struct PairRows {
    const int64_t *offs_a, *offs_b;
    int64_t cap_a, cap_b;
    int64_t R, stride;
    int32_t cut_b;  // only_second: B is the side in windows
    __device__ int64_t operator()(int64_t i, int32_t* err) const {
        const int64_t na = side_len(offs_a[i], offs_a[i + 1], cap_a, err);
        const int64_t nb = side_len(offs_b[i], offs_b[i + 1], cap_b, err);
        int64_t C, step;
        return cut_b ? pair_window_count(nb, na, R, stride, C, step) : pair_window_count(na, nb, R, stride, C, step);
    }
};

struct PairArgs {
    RowArgs r;
    const int64_t *offs_a, *offs_b;
    const int64_t* rows;  // row_offsets: the windows form; NULL: row i is pair i
    int64_t n_pairs, n_rows;
    int32_t R, stride, strategy;
};

// One placed row of pairs: its pair (behind the first of the workgroup), the ids kept of both sides, the window's start
// inside the cut side, and the index of the first id of either side that the row holds.
struct PairRow {
    int32_t lo, ka, kb;
    int64_t start, a0, b0;
};

// Row tid of the workgroup's rows (the first is row0), both forms: the pair is the row itself, or is found among the nd
// staged row_offsets.  What k_collate_pairs and k_plan_pairs both place a row with.
__device__ __forceinline__ PairRow pair_row(const PairArgs& a, const int64_t* s_ro, int64_t d0, int32_t nd, int64_t row0, int tid) {
    const bool win = a.rows != nullptr;
    PairRow r;
    r.lo = tid;
    int64_t k = 0;
    if (win) {
        r.lo = staged_item_of_row(s_ro, nd, row0 + tid);
        k = row0 + tid - s_ro[r.lo];
    }
    const int64_t p = d0 + r.lo;
    const int64_t a0 = a.offs_a[p], b0 = a.offs_b[p];
    const int64_t na = side_len(a0, a.offs_a[p + 1], a.r.cap_a, a.r.err);
    const int64_t nb = side_len(b0, a.offs_b[p + 1], a.r.cap_b, a.r.err);
    r.ka = 0, r.kb = 0;
    r.start = 0;
    const bool cut_b = a.strategy == HUTK_PAIR_ONLY_SECOND;
    if (!win) pair_lengths(na, nb, a.R, a.strategy, r.ka, r.kb);
    else {
        int64_t C, step;
        const int64_t n = cut_b ? nb : na;
        const int64_t w = pair_window_count(n, cut_b ? na : nb, a.R, a.stride, C, step);
        if (k < 0 || k >= w) note_error(a.r.err, HUTK_E_ARG);  // (a row_offsets that is not the scan of the counts)
        else {
            r.start = k * step;  // < n, or 0
            const int32_t kn = n - r.start < C ? (int32_t)(n - r.start) : (int32_t)C;
            const int32_t ko = a.R - (int32_t)C;
            r.ka = cut_b ? ko : kn;
            r.kb = cut_b ? kn : ko;
        }
    }
    r.a0 = a0 + (cut_b ? 0 : r.start);
    r.b0 = b0 + (cut_b ? r.start : 0);
    return r;
}

// The planner, both forms.  Thread r places row r once: its pair (itself, or in the windows form found among the staged
// row_offsets as k_collate_windows finds a document), both sides' offsets, ka, kb and the window's start go to LDS.
// Whatever the offsets hold, every index stays inside the offsets arrays and the two id buffers.
template <int W, bool VEC>
__global__ __launch_bounds__(TB) void k_collate_pairs(const PairArgs a) {
    __shared__ int64_t s_ro[PAD_ROWS + 1];
    __shared__ int64_t s_srca[PAD_ROWS], s_srcb[PAD_ROWS];  // index of element q in ids_a / ids_b, less q
    __shared__ int64_t s_start[PAD_ROWS];                   // of the row's window inside the cut side
    __shared__ int32_t s_ka[PAD_ROWS], s_kb[PAD_ROWS], s_j[PAD_ROWS];
    __shared__ int64_t s_d0;
    const bool win = a.rows != nullptr;
    if (win && (a.rows[0] != 0 || a.rows[a.n_pairs] != a.n_rows)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) note_error(a.r.err, HUTK_E_ARG);
        return;
    }
    const int tid = threadIdx.x;
    const RowTile t = row_tile(a.r, a.n_rows);
    if (t.nrows <= 0) return;
    int64_t d0 = t.row0;  // the first pair of this workgroup's rows
    int32_t nd = t.nrows;
    if (win) {
        d0 = stage_items(a.rows, a.n_pairs, t, s_ro, &s_d0, nd);
        __syncthreads();
    }
    if (tid < t.nrows) {
        const PairRow r = pair_row(a, s_ro, d0, nd, t.row0, tid);
        s_j[tid] = r.lo;
        s_start[tid] = r.start;
        s_ka[tid] = r.ka;
        s_kb[tid] = r.kb;
        s_srca[tid] = r.a0 - a.r.has_bos;
        s_srcb[tid] = r.b0 - (a.r.has_bos + r.ka + a.r.n_sep);
    }
    __syncthreads();
    write_rows<W, VEC, true>(a.r, t, [&](int32_t rl) {
        return RowPlan{s_ka[rl], s_kb[rl], s_srca[rl], s_srcb[rl], d0 + s_j[rl], s_start[rl]};
    });
}

// ---- row plans --------------------------------------------------------------------------------------------------------
// The geometry of a row as data: plan[r] = (item, start, src_a, ka, col_a, src_b, kb, col_b), eight int64.
// Columns col_a .. col_a + ka - 1 of row r hold ids_a[src_a ..], columns col_b .. col_b + kb - 1 ids_b[src_b ..]; every
// other column is bos, a separator, eos or padding.  A planner is the placement of its collate kernel, one thread per
// row, with the row written as a plan instead of as elements.
struct PlanOut {
    int64_t* plan;
    int32_t vec;  // plan is 16-byte aligned
};

// The plan of row `row` from what write_rows takes: the kept lengths, the first id of either side, (item, start)
template <bool PAIR>
__device__ __forceinline__ void store_plan(const PlanOut& o, const RowArgs& a, int64_t row, int64_t item, int64_t start,
                                           int64_t src_a, int32_t ka, int64_t src_b, int32_t kb) {
    const int32_t sl = ka + (PAIR ? kb : 0) + a.s;
    const int64_t col_a = (a.pad_left ? a.L - sl : 0) + a.has_bos;
    const int64_t col_b = col_a + ka + (PAIR ? a.n_sep : 0);
    int64_t* p = o.plan + 8 * row;
    if (!PAIR) src_b = 0, kb = 0;
    if (o.vec) {
        longlong2* q = reinterpret_cast<longlong2*>(p);
        q[0] = make_longlong2(item, start);
        q[1] = make_longlong2(src_a, ka);
        q[2] = make_longlong2(col_a, src_b);
        q[3] = make_longlong2(kb, col_b);
    } else {
        p[0] = item, p[1] = start, p[2] = src_a, p[3] = ka, p[4] = col_a, p[5] = src_b, p[6] = kb, p[7] = col_b;
    }
}

// the 256 rows a workgroup of a planner places, as the tile that stage_items takes
__device__ __forceinline__ RowTile plan_tile(int64_t n_rows) {
    RowTile t{};
    t.row0 = (int64_t)blockIdx.x * TB;
    const int64_t left = n_rows - t.row0;
    t.nrows = left < TB ? (int32_t)left : TB;
    return t;
}

__global__ __launch_bounds__(TB) void k_plan_padded(const PadArgs a, const PlanOut o) {
    const int64_t row = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (row >= a.n_docs) return;
    if (a.offs[0] != 0 || a.offs[a.n_docs] != a.r.cap_a) {  // the rows of offsets that do not fit the ids are empty
        note_error(a.r.err, HUTK_E_ARG);
        store_plan<false>(o, a.r, row, row, 0, 0, 0, 0, 0);
        return;
    }
    const int64_t o0 = a.offs[row], o1 = a.offs[row + 1];
    int64_t dl = o1 - o0;
    if (dl < 0 || dl > a.r.cap_a) {
        note_error(a.r.err, HUTK_E_ARG);
        store_plan<false>(o, a.r, row, row, 0, 0, 0, 0, 0);
        return;
    }
    const int32_t room = a.r.L - a.r.s;
    const int32_t ka = dl > room ? room : (int32_t)dl;
    const int64_t start = a.trunc_left ? dl - ka : 0;
    store_plan<false>(o, a.r, row, row, start, o0 + start, ka, 0, 0);
}

__global__ __launch_bounds__(TB) void k_plan_windows(const WinArgs a, const PlanOut o) {
    __shared__ int64_t s_ro[PAD_ROWS + 1], s_off[PAD_ROWS + 1];
    __shared__ int64_t s_d0;
    const int tid = threadIdx.x;
    const RowTile t = plan_tile(a.n_rows);
    if (t.nrows <= 0) return;
    if (a.offs[0] != 0 || a.offs[a.n_docs] != a.r.cap_a || a.rows[0] != 0 || a.rows[a.n_docs] != a.n_rows) {
        note_error(a.r.err, HUTK_E_ARG);
        if (tid < t.nrows) store_plan<false>(o, a.r, t.row0 + tid, 0, 0, 0, 0, 0, 0);
        return;
    }
    int32_t nd;
    const int64_t d0 = stage_items(a.rows, a.n_docs, t, s_ro, &s_d0, nd);
    for (int32_t i = tid; i <= nd; i += TB) s_off[i] = a.offs[d0 + i];
    __syncthreads();
    if (tid < t.nrows) {
        int64_t start;
        int32_t n;
        const int32_t lo = window_row(s_ro, s_off, nd, t.row0 + tid, a.r.cap_a, a.C, a.step, a.r.err, start, n);
        store_plan<false>(o, a.r, t.row0 + tid, d0 + lo, start, s_off[lo] + start, n, 0, 0);
    }
}

__global__ __launch_bounds__(TB) void k_plan_pairs(const PairArgs a, const PlanOut o) {
    __shared__ int64_t s_ro[PAD_ROWS + 1];
    __shared__ int64_t s_d0;
    const bool win = a.rows != nullptr;
    const int tid = threadIdx.x;
    const RowTile t = plan_tile(a.n_rows);
    if (t.nrows <= 0) return;
    if (win && (a.rows[0] != 0 || a.rows[a.n_pairs] != a.n_rows)) {
        note_error(a.r.err, HUTK_E_ARG);
        if (tid < t.nrows) store_plan<true>(o, a.r, t.row0 + tid, 0, 0, 0, 0, 0, 0);
        return;
    }
    int64_t d0 = t.row0;
    int32_t nd = t.nrows;
    if (win) {
        d0 = stage_items(a.rows, a.n_pairs, t, s_ro, &s_d0, nd);
        __syncthreads();
    }
    if (tid < t.nrows) {
        const PairRow r = pair_row(a, s_ro, d0, nd, t.row0, tid);
        store_plan<true>(o, a.r, t.row0 + tid, d0 + r.lo, r.start, r.a0, r.ka, r.b0, r.kb);
    }
}

// ---- the gather -------------------------------------------------------------------------------------------------------
// out[r][c] = the record of the token that a planned row holds at column c, `fill` where it holds none: any per-token
// array (spans, word ids, labels) in the rows' shape.  The tiling is that of the row writers (row_tile); the plans of a
// workgroup's rows are staged in LDS once, clipped to the row, so that an element is four comparisons and at most one
// load of REC bytes.  The plan is a caller's tensor: whatever it holds, a column outside [0, L) is never written and a
// record outside values_a[0, n_a) / values_b[0, n_b) is never read.
struct GatherArgs {
    RowArgs r;  // (L, rows_per_block, col_chunks, err: what row_tile reads)
    const int64_t* plan;
    int64_t n_rows;
    const void *va, *vb;
    int64_t n_a, n_b;
    int32_t f0, f1, f2, f3;  // the fill record (no array: a kernel argument indexed at run time lives in scratch)
    void* out;
};

// one side of one plan, clipped: columns [lo, hi) of the row hold records src + (c - col); lo == hi: none
__device__ __forceinline__ void clip_side(int64_t col, int64_t k, int32_t L, int32_t* err, int32_t& lo, int32_t& hi, int32_t& c0) {
    lo = hi = c0 = 0;
    if (k < 0) note_error(err, HUTK_E_ARG);
    if (k <= 0) return;
    if (col < 0 || col >= L || k > L - col) note_error(err, HUTK_E_ARG);  // (a planner never writes a side that leaves the row)
    if (col >= L || col <= -(int64_t)L) return;
    if (k > L) k = L;
    const int64_t end = col + k;  // no overflow: |col| < L, k <= L
    if (end <= 0) return;
    lo = col < 0 ? 0 : (int32_t)col;
    hi = end > L ? L : (int32_t)end;
    c0 = (int32_t)col;
}

template <int REC>
struct RecWord;  // the type a record is moved as on the wide path
template <> struct RecWord<4> { using T = int32_t; };
template <> struct RecWord<8> { using T = int2; };
template <> struct RecWord<16> { using T = int4; };

// WIDE: L * REC is a multiple of 16, out is 16-byte aligned and both value arrays are aligned to REC: a thread moves
// 16 / REC records and stores 16 bytes.  Otherwise a thread moves one record dword by dword.
template <int REC, bool WIDE>
__global__ __launch_bounds__(TB) void k_rows_gather(const GatherArgs a) {
    __shared__ int64_t s_srca[PAD_ROWS], s_srcb[PAD_ROWS];
    __shared__ int32_t s_loa[PAD_ROWS], s_hia[PAD_ROWS], s_ca[PAD_ROWS], s_lob[PAD_ROWS], s_hib[PAD_ROWS], s_cb[PAD_ROWS];
    const RowTile t = row_tile(a.r, a.n_rows);
    if (t.nrows <= 0) return;
    if (threadIdx.x < t.nrows) {
        const int tid = threadIdx.x;
        const int64_t* p = a.plan + 8 * (t.row0 + tid);
        const bool first = t.c0 == 0;  // (of the workgroups of one long row, the first reports what is wrong with its plan)
        int32_t lo, hi, c0;
        clip_side(p[4], p[3], a.r.L, first ? a.r.err : nullptr, lo, hi, c0);
        s_srca[tid] = p[2], s_loa[tid] = lo, s_hia[tid] = hi, s_ca[tid] = c0;
        const int32_t lo_a = lo, hi_a = hi;
        clip_side(p[7], p[6], a.r.L, first ? a.r.err : nullptr, lo, hi, c0);
        s_srcb[tid] = p[5], s_lob[tid] = lo, s_hib[tid] = hi, s_cb[tid] = c0;
        if (first && lo_a < hi_a && lo < hi && lo < hi_a && lo_a < hi) note_error(a.r.err, HUTK_E_ARG);  // (sides that overlap: A wins)
    }
    __syncthreads();
    constexpr int V = WIDE ? 16 / REC : 1;  // records per thread
    constexpr int D = REC / 4;              // dwords per record
    const int32_t fill[4] = {a.f0, a.f1, a.f2, a.f3};  // (indexed by constants only)
    for (int32_t i = threadIdx.x * V; i < t.total; i += TB * V) {
        const int32_t rl = t.one_row ? 0 : i / a.r.L;
        const int32_t c = t.one_row ? t.c0 + i : i - rl * a.r.L;
        const int32_t lo_a = s_loa[rl], hi_a = s_hia[rl], lo_b = s_lob[rl], hi_b = s_hib[rl];
        int32_t v[V * D];
#pragma unroll
        for (int e = 0; e < V; e++) {
#pragma unroll
            for (int w = 0; w < D; w++) v[e * D + w] = fill[w];
            const int32_t col = c + e;
            const bool in_a = col >= lo_a && col < hi_a;
            if (!in_a && !(col >= lo_b && col < hi_b)) continue;
            const int64_t src = in_a ? s_srca[rl] : s_srcb[rl], n = in_a ? a.n_a : a.n_b;
            const int64_t d = col - (in_a ? s_ca[rl] : s_cb[rl]);  // >= 0: col >= lo >= the side's first column
            if (src >= n || src + d < 0 || src + d >= n) {  // (no overflow: src < n and 0 <= d < L)
                note_error(a.r.err, HUTK_E_ARG);
                continue;
            }
            const void* base = in_a ? a.va : a.vb;
            if constexpr (WIDE) {
                using T = typename RecWord<REC>::T;
                const T x = static_cast<const T*>(base)[src + d];
                if constexpr (REC == 4) v[e] = x;
                else if constexpr (REC == 8) v[2 * e] = x.x, v[2 * e + 1] = x.y;
                else v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
            } else {
                const int32_t* x = static_cast<const int32_t*>(base) + (src + d) * D;
#pragma unroll
                for (int w = 0; w < D; w++) v[w] = x[w];
            }
        }
        const int64_t at = (t.row0 + rl) * (int64_t)a.r.L + c;  // in records
        if constexpr (WIDE) {
            *reinterpret_cast<int4*>(static_cast<char*>(a.out) + at * REC) = make_int4(v[0], v[1], v[2], v[3]);
        } else {
            int32_t* q = static_cast<int32_t*>(a.out) + at * D;
#pragma unroll
            for (int w = 0; w < D; w++) q[w] = v[w];
        }
    }
}

// ---- targets: masked-LM corruption and loss labels ----------------------------------------------------------
// Both read rows that exist already, [n_rows][L] elements of W bytes, with the rows' plan, and write rectangles of the
// same shape at the same positions: an element is read and written by one thread.  The tiling is row_tile's, the plans
// of a workgroup's rows are staged clipped as k_rows_gather stages them, and a plan is trusted as little as there.
struct SidePlans {
    int64_t srca[PAD_ROWS], srcb[PAD_ROWS];
    int32_t loa[PAD_ROWS], hia[PAD_ROWS], ca[PAD_ROWS], lob[PAD_ROWS], hib[PAD_ROWS], cb[PAD_ROWS];
    int32_t endb[PAD_ROWS];  // col_b + kb inside [0, L]: the template's columns in front of it are bos and separators
};

// Every thread of the workgroup must call it; the plans are visible when it returns.
__device__ __forceinline__ void stage_plans(SidePlans& s, const int64_t* plan, const RowTile& t, int32_t L, int32_t* err) {
    if (threadIdx.x < t.nrows) {
        const int tid = threadIdx.x;
        const int64_t* p = plan + 8 * (t.row0 + tid);
        int32_t* e = t.c0 == 0 ? err : nullptr;  // (of the workgroups of one long row, the first reports what is wrong with its plan)
        int32_t lo, hi, c0;
        clip_side(p[4], p[3], L, e, lo, hi, c0);
        s.srca[tid] = p[2], s.loa[tid] = lo, s.hia[tid] = hi, s.ca[tid] = c0;
        const int32_t lo_a = lo, hi_a = hi;
        clip_side(p[7], p[6], L, e, lo, hi, c0);
        s.srcb[tid] = p[5], s.lob[tid] = lo, s.hib[tid] = hi, s.cb[tid] = c0;
        if (lo_a < hi_a && lo < hi && lo < hi_a && lo_a < hi) note_error(e, HUTK_E_ARG);  // (sides that overlap: A wins)
        const int64_t col = p[7] < -(int64_t)L ? -(int64_t)L : p[7] > L ? L : p[7];
        const int64_t k = p[6] < 0 ? 0 : p[6] > 2 * (int64_t)L ? 2 * (int64_t)L : p[6];
        const int64_t end = col + k;  // (what a planner writes is left as it is: 0 <= col_b, col_b + kb <= L)
        s.endb[tid] = end < 0 ? 0 : end > L ? L : (int32_t)end;
    }
    __syncthreads();
}

template <int W>
using elem_t = std::conditional_t<W == 4, int32_t, int64_t>;  // an element of the rows: ids of either width are moved whole

template <int W>
__device__ __forceinline__ void load4(const void* base, int64_t i, elem_t<W> (&v)[4]) {
    if constexpr (W == 4) {
        const int4 x = *reinterpret_cast<const int4*>(static_cast<const int32_t*>(base) + i);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
        const longlong2* p = reinterpret_cast<const longlong2*>(static_cast<const int64_t*>(base) + i);
        const longlong2 x = p[0], y = p[1];
        v[0] = x.x, v[1] = x.y, v[2] = y.x, v[3] = y.y;
    }
}
template <int W>
__device__ __forceinline__ void put4(void* base, int64_t i, const elem_t<W> (&v)[4]) {
    if constexpr (W == 4) store4<4>(base, i, v);
    else {  // (store4<8> widens int32: a label or an id of 64 bits goes as it is)
        longlong2* p = reinterpret_cast<longlong2*>(static_cast<int64_t*>(base) + i);
        p[0] = make_longlong2(v[0], v[1]);
        p[1] = make_longlong2(v[2], v[3]);
    }
}
template <int W>
__device__ __forceinline__ void put1(void* base, int64_t i, elem_t<W> v) {
    if constexpr (W == 4) store1<4>(base, i, v);
    else static_cast<int64_t*>(base)[i] = v;
}

struct MlmArgs {
    RowArgs r;  // (L, rows_per_block, col_chunks, err: what row_tile reads)
    const int64_t* plan;
    int64_t n_rows;
    const void* ids;
    void *out, *labels;
    const int32_t *wa, *wb;  // whole-word mode: the word of every token of either side
    int64_t n_a, n_b;
    uint64_t seed;
    uint64_t select_below, mask_below, random_below;  // 0 .. 2^32, against draws of 32 bits
    uint64_t vocab;
    int64_t ignore;
    int32_t mask_id, sides;
};

// out[r][c] = the id, mask_id or a random id; labels[r][c] = the id where the column was selected, ignore elsewhere.
// Only a column of a side named in `sides` draws (hutk_philox.h: the draw is a function of seed, row and column, or of
// seed, row, side and word; never of the tile, W, VEC or the batch).  WORDS: the word of the column's token is selected,
// and a selected column then draws its kind and id; a word id below 0 protects its token.
template <int W, bool VEC, bool WORDS>
__global__ __launch_bounds__(TB) void k_rows_mlm(const MlmArgs a) {
    __shared__ SidePlans s;
    const RowTile t = row_tile(a.r, a.n_rows);
    if (t.nrows <= 0) return;
    stage_plans(s, a.plan, t, a.r.L, a.r.err);
    constexpr int V = VEC ? 4 : 1;
    using T = elem_t<W>;
    for (int32_t i = threadIdx.x * V; i < t.total; i += TB * V) {
        const int32_t rl = t.one_row ? 0 : i / a.r.L;
        const int32_t c = t.one_row ? t.c0 + i : i - rl * a.r.L;
        const int64_t row = t.row0 + rl;
        const int64_t at = row * (int64_t)a.r.L + c;
        T v[V], lab[V];
        if constexpr (VEC) load4<W>(a.ids, at, v);
        else v[0] = static_cast<const T*>(a.ids)[at];
        const int32_t lo_a = s.loa[rl], hi_a = s.hia[rl], lo_b = s.lob[rl], hi_b = s.hib[rl];
#pragma unroll
        for (int e = 0; e < V; e++) {
            lab[e] = (T)a.ignore;
            const int32_t col = c + e;
            const bool in_a = col >= lo_a && col < hi_a;
            const bool in_b = !in_a && col >= lo_b && col < hi_b;
            if (!((in_a && (a.sides & HUTK_MLM_SIDE_A)) || (in_b && (a.sides & HUTK_MLM_SIDE_B)))) continue;
            hutk::Philox4 d;
            if constexpr (WORDS) {
                const int64_t src = in_a ? s.srca[rl] : s.srcb[rl], n = in_a ? a.n_a : a.n_b;
                const int64_t k = col - (in_a ? s.ca[rl] : s.cb[rl]);  // >= 0: col >= lo >= the side's first column
                if (src >= n || src + k < 0 || src + k >= n) {  // (no overflow: src < n and 0 <= k < L)
                    note_error(a.r.err, HUTK_E_ARG);
                    continue;
                }
                const int32_t word = (in_a ? a.wa : a.wb)[src + k];
                if (word < 0) continue;
                if (hutk::draw(a.seed, row, (uint32_t)word, in_a ? hutk::DRAW_WORD_A : hutk::DRAW_WORD_B).x >= a.select_below) continue;
                d = hutk::draw(a.seed, row, (uint32_t)col, hutk::DRAW_COLUMN);
            } else {
                d = hutk::draw(a.seed, row, (uint32_t)col, hutk::DRAW_COLUMN);
                if (d.x >= a.select_below) continue;
            }
            lab[e] = v[e];
            if (d.y < a.mask_below) v[e] = a.mask_id;
            else if (d.y < a.random_below) v[e] = hutk::draw_id(d.z, a.vocab);
        }
        if constexpr (VEC) {
            put4<W>(a.out, at, v);
            put4<W>(a.labels, at, lab);
        } else {
            put1<W>(a.out, at, v[0]);
            put1<W>(a.labels, at, lab[0]);
        }
    }
}

struct LabelArgs {
    RowArgs r;  // (L, rows_per_block, col_chunks, err: what row_tile reads)
    const int64_t* plan;
    int64_t n_rows;
    const void* ids;
    const uint8_t* mask;
    void* labels;
    int64_t ignore;
    int32_t flags;
};

// labels[r][c] = ids[r][c] on a loss column, ignore elsewhere; with HUTK_LABELS_SHIFT the id and the question move one
// column to the right: what column c predicts.  A loss column is a real one (mask != 0) of a kind named in flags: A, B,
// the template in front of col_b + kb (bos, separators) or at and behind it (eos).  The neighbour behind a thread's
// elements is read from global memory, so the end of a workgroup's columns is no special place.
template <int W, bool VEC>
__global__ __launch_bounds__(TB) void k_rows_labels(const LabelArgs a) {
    __shared__ SidePlans s;
    const RowTile t = row_tile(a.r, a.n_rows);
    if (t.nrows <= 0) return;
    stage_plans(s, a.plan, t, a.r.L, a.r.err);
    constexpr int V = VEC ? 4 : 1;
    using T = elem_t<W>;
    const bool shift = (a.flags & HUTK_LABELS_SHIFT) != 0;
    for (int32_t i = threadIdx.x * V; i < t.total; i += TB * V) {
        const int32_t rl = t.one_row ? 0 : i / a.r.L;
        const int32_t c = t.one_row ? t.c0 + i : i - rl * a.r.L;
        const int64_t at = (t.row0 + rl) * (int64_t)a.r.L + c;
        T v[V + 1], lab[V];
        uint8_t m[V + 1];
        if constexpr (VEC) {
            T q[4];
            load4<W>(a.ids, at, q);
            const uchar4 x = *reinterpret_cast<const uchar4*>(a.mask + at);
            v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
            m[0] = x.x, m[1] = x.y, m[2] = x.z, m[3] = x.w;
        } else {
            v[0] = static_cast<const T*>(a.ids)[at];
            m[0] = a.mask[at];
        }
        v[V] = 0;
        m[V] = shift && c + V < a.r.L ? a.mask[at + V] : 0;  // (the row ends at L: its last column predicts nothing)
        const int32_t lo_a = s.loa[rl], hi_a = s.hia[rl], lo_b = s.lob[rl], hi_b = s.hib[rl], end_b = s.endb[rl];
        bool loss[V + 1];
#pragma unroll
        for (int e = 0; e <= V; e++) {
            const int32_t col = c + e;
            const bool in_a = col >= lo_a && col < hi_a;
            const bool in_b = !in_a && col >= lo_b && col < hi_b;
            const int kind = in_a ? HUTK_LABELS_A : in_b ? HUTK_LABELS_B : col < end_b ? HUTK_LABELS_TEMPLATE : HUTK_LABELS_END;
            loss[e] = m[e] != 0 && (a.flags & kind) != 0;
        }
        if (loss[V]) v[V] = static_cast<const T*>(a.ids)[at + V];  // (shift only: m[V] is 0 without)
#pragma unroll
        for (int e = 0; e < V; e++) {
            if (shift) lab[e] = m[e] != 0 && loss[e + 1] ? v[e + 1] : (T)a.ignore;
            else lab[e] = loss[e] ? v[e] : (T)a.ignore;
        }
        if constexpr (VEC) put4<W>(a.labels, at, lab);
        else put1<W>(a.labels, at, lab[0]);
    }
}

// ---- packed rows for training ---------------------------------------------------------------------------
// cu_seqlens is a stream compaction of the flat elements that start a sequence: the rows scan with "element" as the
// item counts them per workgroup (k_rows_count<CuStarts>) and scans the workgroups' counts; the write differs, since
// what is kept is the element's index at its rank, not a rank per element (k_cu_write).  The gaps between neighbouring
// entries of what was written give max_seqlen (k_cu_gaps: a maximum per workgroup, one atomic each).
constexpr int CU_TILE = 2048;  // elements per workgroup of the count (times a whole number above WIN_BLOCKS * CU_TILE elements)

struct CuStarts {
    const int32_t* seg;
    int64_t L;
    __device__ __forceinline__ int64_t operator()(int64_t f, int32_t*) const {
        return f % L == 0 || seg[f] != seg[f - 1];
    }
};

struct CuArgs {
    int32_t* cu;    // [cap + 1]; NULL: count only
    int32_t* info;  // (n_seq, max_seqlen)
    int64_t cap, total;
};

__global__ __launch_bounds__(TB) void k_cu_write(const ScanArgs a, const CuStarts starts, const CuArgs o) {
    __shared__ int64_t s_part[TB / 64];
    const int64_t lo = (int64_t)blockIdx.x * a.per_block;
    const int64_t hi = lo + a.per_block < a.n ? lo + a.per_block : a.n;
    const int64_t n_seq = a.sums[gridDim.x];
    int64_t base = a.sums[blockIdx.x];
    for (int64_t at = lo; at < hi; at += TB) {  // (uniform: every thread meets the barriers of the scan)
        const int64_t i = at + threadIdx.x;
        const int64_t w = i < hi ? starts(i, nullptr) : 0;
        int64_t total;
        const int64_t k = base + hutk::block_excl(w, s_part, total);
        if (w && o.cu && k < o.cap) o.cu[k] = (int32_t)i;
        base += total;
    }
    // behind the starts: the total in every slot up to and including slot cap
    if (o.cu)
        for (int64_t k = (n_seq < o.cap ? n_seq : o.cap) + (int64_t)blockIdx.x * TB + threadIdx.x; k <= o.cap; k += (int64_t)gridDim.x * TB)
            o.cu[k] = (int32_t)o.total;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        o.info[0] = (int32_t)n_seq;
        o.info[1] = 0;
        if (o.cu && n_seq > o.cap) note_error(a.err, HUTK_E_CAPACITY);
    }
}

// info[1] = the largest cu[k + 1] - cu[k] over the sequences written, k < min(n_seq, cap)
__global__ __launch_bounds__(TB) void k_cu_gaps(const CuArgs o) {
    __shared__ int32_t s_max[TB / 64];
    const int64_t n_seq = o.info[0];
    const int64_t m = n_seq < o.cap ? n_seq : o.cap;
    int32_t mine = 0;
    for (int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x; k < m; k += (int64_t)gridDim.x * TB) {
        const int32_t g = o.cu[k + 1] - o.cu[k];
        mine = g > mine ? g : mine;
    }
    const int lane = threadIdx.x & 63;
    mine = __shfl(hutk::wave_incl_max(mine, lane), 63);
    if (lane == 0) s_max[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int u = 1; u < TB / 64; u++) mine = s_max[u] > mine ? s_max[u] : mine;
        if (mine > 0) atomicMax(&o.info[1], mine);
    }
}

struct PackedLabelArgs {
    const void* values;
    const int32_t* seg;
    void* labels;
    int64_t n, L;  // elements, row length
    int64_t ignore;
    int32_t shift;
};

// labels[f] = values[f] on a real column (segment != 0), or with shift what the column predicts: values[f + 1] when that
// column is in the same row and of the same, real segment.  One elementwise pass; the neighbour behind a thread's V
// elements is read from global memory, so the end of a workgroup's elements is no special place.
template <int W, bool VEC>
__global__ __launch_bounds__(TB) void k_packed_labels(const PackedLabelArgs a) {
    constexpr int V = VEC ? 4 : 1;
    using T = elem_t<W>;
    const int64_t at = ((int64_t)blockIdx.x * TB + threadIdx.x) * V;
    if (at >= a.n) return;
    const int64_t c = at % a.L;  // (VEC: L % 4 == 0, the V elements share a row)
    T v[V + 1], lab[V];
    int32_t sg[V + 1];
    if constexpr (VEC) {
        T q[4];
        load4<W>(a.values, at, q);
        const int4 x = *reinterpret_cast<const int4*>(a.seg + at);
        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
        sg[0] = x.x, sg[1] = x.y, sg[2] = x.z, sg[3] = x.w;
    } else {
        v[0] = static_cast<const T*>(a.values)[at];
        sg[0] = a.seg[at];
    }
    const bool next = a.shift && c + V < a.L;  // (the row ends at L: its last column predicts nothing)
    sg[V] = next ? a.seg[at + V] : 0;
    v[V] = next && sg[V] != 0 ? static_cast<const T*>(a.values)[at + V] : 0;
#pragma unroll
    for (int e = 0; e < V; e++) {
        if (a.shift) lab[e] = sg[e] != 0 && sg[e + 1] == sg[e] ? v[e + 1] : (T)a.ignore;
        else lab[e] = sg[e] != 0 ? v[e] : (T)a.ignore;
    }
    if constexpr (VEC) put4<W>(a.labels, at, lab);
    else put1<W>(a.labels, at, lab[0]);
}

// ---- targets: span corruption ---------------------------------------------------------------------------------
// The first row pass whose outputs are of another length than its input: every noise span of a row becomes one
// sentinel in the corrupted row, and the spans move, each behind its sentinel, into a target row.  One wavefront per
// row, four rows per workgroup, no LDS and no barrier: the wavefront walks its row in chunks of 256 columns, four
// consecutive ones per lane, and carries four values from chunk to chunk -- the prefix maximum of the reaches, whether
// the last column was noise, the count of run beginnings and the packed counts of kept columns and target elements.
// Every __shfl is executed by all 64 lanes: the trip count depends on L alone and a row behind the last one leaves as a
// whole wavefront.
constexpr int SPAN_LEN_MAX = 32;                // lengths a span can be drawn with
constexpr int SPAN_CHUNK = 64 * 4;              // columns a wavefront takes per trip

struct SpanArgs {
    const int64_t* plan;
    int64_t n_rows;
    const void* ids;
    const uint8_t* mask;
    void *out, *labels, *dec;  // dec: NULL without decoder_start_id
    uint8_t* out_mask;
    int32_t *in_len, *tgt_len, *err;
    uint64_t seed;
    uint64_t start_below;  // 0 .. 2^32, against a draw of 32 bits
    int64_t sentinel_first, pad, ignore;
    int32_t L, L_tgt;
    int32_t n_cmp;   // the thresholds below 2^32 among len_below[0 .. n_len - 2]: the others no draw reaches
    int32_t step, n_sent, eos, dec_start, sides;
    uint32_t len_below[SPAN_LEN_MAX - 1];  // (indexed by constants only: the loop over it is unrolled)
};

__device__ __forceinline__ uint4 splat16(uint8_t v) {
    const uint32_t x = v * 0x01010101u;
    return make_uint4(x, x, x, x);
}
__device__ __forceinline__ uint4 splat16(int32_t v) { return make_uint4((uint32_t)v, (uint32_t)v, (uint32_t)v, (uint32_t)v); }
__device__ __forceinline__ uint4 splat16(int64_t v) {
    const uint32_t lo = (uint32_t)(uint64_t)v, hi = (uint32_t)((uint64_t)v >> 32);
    return make_uint4(lo, hi, lo, hi);
}

// p[from .. to) = v by one wavefront: single elements up to the first 16-byte boundary, 16-byte stores, single elements
// behind the last one.  p is aligned to its elements.
template <class T>
__device__ __forceinline__ void wave_fill(T* p, int64_t from, int64_t to, T v, int lane) {
    if (from >= to) return;
    constexpr int PER = 16 / (int)sizeof(T);
    T* b = p + from;
    const int64_t n = to - from;
    int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(b) & 15)) & 15) / (int64_t)sizeof(T);  // < PER <= 16
    if (head > n) head = n;
    if (lane < head) b[lane] = v;
    const int64_t nvec = (n - head) / PER;
    const uint4 x = splat16(v);
    for (int64_t i = lane; i < nvec; i += 64) *reinterpret_cast<uint4*>(b + head + i * PER) = x;
    const int64_t done = head + nvec * PER;  // n - done < PER
    if (lane < n - done) b[done + lane] = v;
}

// See include/hutoken_amd.h for the rule.  VEC: L % 4 == 0, ids 16-byte and mask 4-byte aligned: a lane loads its four
// columns at once.  Sums: the run beginnings in 32 bits (at most (L + 1) / 2); the kept columns (at most L < 2^31) in
// the upper and the target elements (noise columns plus runs plus eos: at most L + (L + 1) / 2 + 1 < 2^32) in the lower
// half of one 64-bit word, so the lower half never carries into the upper one, for every L the call admits.
template <int W, bool VEC>
__global__ __launch_bounds__(TB) void k_rows_span_corrupt(const SpanArgs a) {
    using T = elem_t<W>;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;  // (a whole wavefront)
    const uint32_t L = (uint32_t)a.L, LT = (uint32_t)a.L_tgt;
    const int64_t* p = a.plan + 8 * row;
    int32_t* e0 = lane == 0 ? a.err : nullptr;  // (one lane reports what is wrong with the row's plan)
    int32_t lo_a, hi_a, lo_b, hi_b, first;
    clip_side(p[4], p[3], a.L, e0, lo_a, hi_a, first);
    clip_side(p[7], p[6], a.L, e0, lo_b, hi_b, first);
    if (lo_a < hi_a && lo_b < hi_b && lo_b < hi_a && lo_a < hi_b) note_error(e0, HUTK_E_ARG);  // (sides that overlap: A wins)
    const bool side_a = (a.sides & HUTK_MLM_SIDE_A) != 0, side_b = (a.sides & HUTK_MLM_SIDE_B) != 0;
    const int64_t in0 = row * (int64_t)L, tg0 = row * (int64_t)LT;  // the row's first element in the rectangles
    const uint32_t n_sent = (uint32_t)a.n_sent;

    const auto label = [&](uint32_t at, T v) {  // target element `at` and what the decoder reads behind it
        if (at >= LT) return;
        put1<W>(a.labels, tg0 + at, v);
        if (a.dec && at + 1 < LT) put1<W>(a.dec, tg0 + at + 1, v);
    };

    uint32_t c_max = 0, c_runs = 0;  // carried: the prefix maximum of reach, the run beginnings so far
    bool c_noise = false;            // carried: noise0 of the column in front of the chunk
    uint64_t c_kt = 0;               // carried: kept columns << 32 | target elements
    for (uint32_t base = 0; base < L; base += SPAN_CHUNK) {
        const uint32_t c0 = base + (uint32_t)lane * 4;  // (below 2^32: base < L < 2^31)
        T v[4] = {0, 0, 0, 0};
        uint8_t m[4] = {0, 0, 0, 0};
        if constexpr (VEC) {
            if (c0 < L) {  // (L % 4 == 0: all four or none)
                load4<W>(a.ids, in0 + c0, v);
                const uchar4 x = *reinterpret_cast<const uchar4*>(a.mask + in0 + c0);
                m[0] = x.x, m[1] = x.y, m[2] = x.z, m[3] = x.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (c0 + e < L) v[e] = static_cast<const T*>(a.ids)[in0 + c0 + e], m[e] = a.mask[in0 + c0 + e];
        }
        // reach, and its inclusive maximum: in the lane, across the lanes, with the chunks before
        uint32_t pm[4], lane_max = 0, end[4], len[4], u1[4];
        bool elig[4], starts[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t c = c0 + e;
            const bool in_a = (int64_t)c >= lo_a && (int64_t)c < hi_a;
            const bool in_b = !in_a && (int64_t)c >= lo_b && (int64_t)c < hi_b;
            elig[e] = m[e] != 0 && ((in_a && side_a) || (in_b && side_b));  // (m is 0 behind the row)
            end[e] = (uint32_t)(in_a ? hi_a : hi_b);
            starts[e] = false, len[e] = 1, u1[e] = 0;
            if (elig[e]) {  // only an eligible column draws
                const hutk::Philox4 d = hutk::draw(a.seed, row, c, hutk::DRAW_SPAN);
                starts[e] = d.x < a.start_below;
                u1[e] = d.y;
            }
        }
        // The lengths: one walk through the table for the four columns, the same in every lane (j < n_cmp is uniform, and
        // so is the question whether any lane starts a span at all).
        if (__ballot(starts[0] || starts[1] || starts[2] || starts[3])) {
#pragma unroll
            for (int j = 0; j < SPAN_LEN_MAX - 1; j++) {
                if (j < a.n_cmp) {
#pragma unroll
                    for (int e = 0; e < 4; e++) len[e] += u1[e] >= a.len_below[j];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t c = c0 + e;
            const uint32_t reach = !starts[e] ? 0 : c + len[e] < end[e] ? c + len[e] : end[e];
            lane_max = lane_max > reach ? lane_max : reach;
            pm[e] = lane_max;
        }
        const uint32_t upto = hutk::wave_incl_max(lane_max, lane);
        uint32_t before = __shfl_up(upto, 1);
        if (lane == 0 || before < c_max) before = c_max;
        c_max = __shfl(upto, 63) > c_max ? __shfl(upto, 63) : c_max;
        bool noise[4];
#pragma unroll
        for (int e = 0; e < 4; e++) noise[e] = elig[e] && (pm[e] > before ? pm[e] : before) > c0 + e;
        // run beginnings and their numbers
        const int left = __shfl_up((int)noise[3], 1);
        const int last = __shfl((int)noise[3], 63);
        bool prev = lane == 0 ? c_noise : left != 0;
        c_noise = last != 0;
        bool begin[4];
        uint32_t runs[4], lane_runs = 0;  // inclusive, in the lane
#pragma unroll
        for (int e = 0; e < 4; e++) {
            begin[e] = noise[e] && !prev;
            prev = noise[e];
            lane_runs += begin[e];
            runs[e] = lane_runs;
        }
        const uint32_t runs_upto = hutk::wave_incl(lane_runs, lane);
        const uint32_t runs_before = runs_upto - lane_runs + c_runs;
        c_runs += __shfl(runs_upto, 63);
        // runs past the last sentinel stay text; kept columns and target elements
        uint64_t kt[4], lane_kt = 0;  // exclusive, in the lane
        uint32_t k[4];
        bool keep[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            k[e] = runs_before + runs[e] - 1;  // the number of the run a noise column lies in
            noise[e] = noise[e] && k[e] < n_sent;
            begin[e] = begin[e] && noise[e];
            keep[e] = m[e] != 0 && (!noise[e] || begin[e]);
            kt[e] = lane_kt;
            lane_kt += ((uint64_t)keep[e] << 32) + (noise[e] ? 1u + begin[e] : 0u);
        }
        const uint64_t kt_upto = hutk::wave_incl(lane_kt, lane);
        const uint64_t kt_before = kt_upto - lane_kt + c_kt;
        c_kt += __shfl(kt_upto, 63);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint64_t at = kt_before + kt[e];
            const T sentinel = (T)(a.sentinel_first + (int64_t)k[e] * a.step);
            if (keep[e]) {  // (fewer columns are kept in front of c than there are: inside the row)
                put1<W>(a.out, in0 + (int64_t)(at >> 32), begin[e] ? sentinel : v[e]);
                a.out_mask[in0 + (int64_t)(at >> 32)] = 1;
            }
            if (noise[e]) {
                uint32_t t = (uint32_t)at;
                if (begin[e]) label(t++, sentinel);
                label(t, v[e]);
            }
        }
    }
    const uint32_t kept = (uint32_t)(c_kt >> 32);
    uint32_t targets = (uint32_t)c_kt;
    if (a.eos != HUTK_NO_TOKEN) {
        if (lane == 0) label(targets, (T)a.eos);
        targets++;
    }
    const uint32_t written = targets < LT ? targets : LT;
    wave_fill(static_cast<T*>(a.out) + in0, kept, L, (T)a.pad, lane);
    wave_fill(a.out_mask + in0, kept, L, (uint8_t)0, lane);
    wave_fill(static_cast<T*>(a.labels) + tg0, written, LT, (T)a.ignore, lane);
    if (a.dec) {
        wave_fill(static_cast<T*>(a.dec) + tg0, (int64_t)written + 1, LT, (T)a.pad, lane);
        if (lane == 0) put1<W>(a.dec, tg0, (T)a.dec_start);
    }
    if (lane == 0) {
        a.in_len[row] = (int32_t)kept;
        a.tgt_len[row] = targets > (uint32_t)INT32_MAX ? INT32_MAX : (int32_t)targets;
    }
}

// ---- answer positions -------------------------------------------------------------------------------------------------
// The tokens of the named side of row r are j in [src, src + k) with non-decreasing spans (a_j, b_j); the answer (s, e)
// of the row's item lies in the row iff k > 0, a_src <= s and b_{src + k - 1} >= e, and then starts at the column of
// max j: a_j <= s and ends at that of min j: b_j >= e.  One wavefront per row, two searches.
struct AnsArgs {
    const int64_t* plan;
    int64_t n_rows;
    const void* spans;
    int64_t n_spans;
    const void* answers;
    int64_t n_items;
    int32_t* out;
    int32_t* err;
    int32_t side_b;
};

template <class T>
__global__ __launch_bounds__(TB) void k_rows_answers(const AnsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;  // (a whole wavefront)
    const int64_t* p = a.plan + 8 * row;
    const int64_t item = p[0], src = p[a.side_b ? 5 : 2], k = p[a.side_b ? 6 : 3], col = p[a.side_b ? 7 : 4];
    int32_t c_start = -1, c_end = -1;
    const bool sound = item >= 0 && item < a.n_items && (k <= 0 || (src >= 0 && src < a.n_spans && k <= a.n_spans - src &&
                                                                    col >= 0 && col <= INT32_MAX - k));
    if (!sound) {
        if (lane == 0) note_error(a.err, HUTK_E_ARG);
    } else if (k > 0) {
        const T* ans = static_cast<const T*>(a.answers) + 2 * item;
        const T* sp = static_cast<const T*>(a.spans) + 2 * src;
        const int64_t s = ans[0], e = ans[1];
        if (s < e) {  // ((-1, -1) or s >= e: no answer)
            const int64_t js = hutk::wave_count_leading(k, [&](int64_t j) { return (int64_t)sp[2 * j] <= s; }) - 1;
            const int64_t je = hutk::wave_count_leading(k, [&](int64_t j) { return (int64_t)sp[2 * j + 1] < e; });
            if (js >= 0 && je < k) c_start = (int32_t)(col + js), c_end = (int32_t)(col + je);
        }
    }
    if (lane == 0) a.out[2 * row] = c_start, a.out[2 * row + 1] = c_end;
}

bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

int device_present(const char* who, int* count = nullptr) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return hutk::api_set_error(HUTK_E_DEVICE, std::string(who) + ": no HIP device");
    if (count) *count = n;
    return HUTK_OK;
}

// f(W, VEC) with out_width and vec as compile-time constants: the four instantiations every collation kernel has
template <class F>
void with_width_vec(int out_width, bool vec, F f) {
    using W4 = std::integral_constant<int, 4>;
    using W8 = std::integral_constant<int, 8>;
    if (out_width == 4) {
        if (vec) f(W4{}, std::true_type{});
        else f(W4{}, std::false_type{});
    } else {
        if (vec) f(W8{}, std::true_type{});
        else f(W8{}, std::false_type{});
    }
}

// The host half of the row tile.  What the three row calls fill in of RowArgs alike; the sides' ids and the separators
// are the caller's.
RowArgs row_args(int64_t max_len, int s, int32_t bos_id, int32_t eos_id, int32_t pad_id, int flags, void* d_input_ids,
                 uint8_t* d_mask, uint8_t* d_token_types, int32_t* d_lengths, int64_t* d_row_map, int32_t* d_err) {
    RowArgs r = {};
    r.L = (int32_t)max_len;
    r.s = s;
    r.bos = bos_id;
    r.eos = eos_id;
    r.pad = pad_id;
    r.has_bos = bos_id != HUTK_NO_TOKEN;
    r.pad_left = (flags & HUTK_COLLATE_PAD_LEFT) != 0;
    r.out = d_input_ids;
    r.mask = d_mask;
    r.types = d_token_types;
    r.lengths = d_lengths;
    r.row_map = d_row_map;
    r.err = d_err;
    return r;
}

// The tile of rows of r.L elements, the workgroups that write n_rows of them, and whether they may store 16 bytes at once
int row_grid(const char* who, RowArgs& r, int64_t n_rows, int64_t* blocks, bool* vec) {
    int64_t rpb = PAD_TILE / r.L;
    rpb = rpb < 1 ? 1 : rpb > PAD_ROWS ? PAD_ROWS : rpb;
    r.rows_per_block = (int32_t)rpb;
    r.col_chunks = rpb == 1 ? (int32_t)(((int64_t)r.L + PAD_TILE - 1) / PAD_TILE) : 1;
    *blocks = (n_rows + rpb - 1) / rpb * r.col_chunks;
    if (*blocks < 1) *blocks = 1;  // (n_rows == 0 with items: the kernel reports it)
    if (*blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, std::string(who) + ": the batch is too large for one launch");
    *vec = r.L % 4 == 0 && aligned_to(r.out, 16) && aligned_to(r.mask, 4) && aligned_to(r.types, 4) && aligned_to(r.row_map, 16);
    return HUTK_OK;
}

// What the window calls share: the sizes they refuse before anything else.  C and step come back for the caller.
int window_sizes(const char* who, int64_t max_len, int64_t stride, int s, int64_t* C, int64_t* step) {
    if (max_len < 1 || max_len < s + 1 || max_len > INT32_MAX)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": max_len must be above the number of bos/eos tokens and below 2^31");
    if (stride < 0 || stride >= max_len - s)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": stride must be in 0 .. max_len - s - 1");
    *C = max_len - s;
    *step = *C - stride;
    return HUTK_OK;
}

// The workgroup sums of the rows scan: one small buffer per device, made at the first call there and kept.  Calls that
// share it are serialised like calls on one packer: a mutex on the host, an event on the device.
struct WinScratch {
    int64_t* sums = nullptr;  // [WIN_BLOCKS + 1]
    hipEvent_t ev = nullptr;
    bool ev_recorded = false;
};
std::mutex g_win_mu;
std::map<int, WinScratch> g_win_scratch;

// The current device's scratch, made at its first use there, with `st` waiting for the last call that used it.  The
// caller holds g_win_mu until it has recorded the event behind its own kernels (scratch_used).
int scratch_for(hipStream_t st, WinScratch** out) {
    int device = 0;
    HUTK_HIP_TRY(hipGetDevice(&device));
    WinScratch& w = g_win_scratch[device];
    if (!w.sums) {
        HUTK_HIP_TRY(hipMalloc((void**)&w.sums, (WIN_BLOCKS + 1) * sizeof(int64_t)));
        if (hipError_t e = hipEventCreateWithFlags(&w.ev, hipEventDisableTiming); e != hipSuccess) {
            (void)hipFree(w.sums);
            w.sums = nullptr;
            HUTK_HIP_TRY(e);
        }
    }
    if (w.ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, w.ev, 0));
    *out = &w;
    return HUTK_OK;
}

int scratch_used(WinScratch* w, hipStream_t st) {
    HUTK_HIP_TRY(hipGetLastError());
    HUTK_HIP_TRY(hipEventRecord(w->ev, st));
    w->ev_recorded = true;
    return HUTK_OK;
}

// d_row_offsets[0 .. n] = the exclusive scan of rows(i) over the n items and its sum; d_err is cleared first
template <class Rows>
int rows_scan(const Rows& rows, int64_t n, int64_t* d_row_offsets, int32_t* d_err, hipStream_t st) {
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n == 0) {
        HUTK_HIP_TRY(hipMemsetAsync(d_row_offsets, 0, sizeof(int64_t), st));
        return HUTK_OK;
    }
    ScanArgs a;
    a.n = n;
    // at most WIN_BLOCKS workgroups: beyond WIN_BLOCKS * TB items each takes several chunks of TB
    a.per_block = (n + (int64_t)WIN_BLOCKS * TB - 1) / ((int64_t)WIN_BLOCKS * TB) * TB;
    const int64_t blocks = (n + a.per_block - 1) / a.per_block;
    std::lock_guard<std::mutex> lock(g_win_mu);
    WinScratch* w;
    if (int rc = scratch_for(st, &w)) return rc;
    a.sums = w->sums;
    a.row_offs = d_row_offsets;
    a.err = d_err;
    const dim3 grid((unsigned)blocks), block(TB);
    hipLaunchKernelGGL(k_rows_count<Rows>, grid, block, 0, st, a, rows);
    hutk::launch_scan_i64(w->sums, blocks, st);
    hipLaunchKernelGGL(k_rows_write<Rows>, grid, block, 0, st, a, rows);
    return scratch_used(w, st);
}

// What the pair calls share: the sizes they refuse before anything else.  s (bos, separators, eos) and R = max_len - s
// come back for the caller.
int pair_sizes(const char* who, int64_t max_len, int64_t stride, int strategy, int32_t bos_id, const int32_t* sep_ids,
               int n_sep, int32_t eos_id, int* s, int64_t* R) {
    if (strategy != HUTK_PAIR_LONGEST_FIRST && strategy != HUTK_PAIR_ONLY_FIRST && strategy != HUTK_PAIR_ONLY_SECOND)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": strategy must be one of HUTK_PAIR_*");
    if (n_sep < 0 || n_sep > HUTK_PAIR_MAX_SEP || (n_sep > 0 && !sep_ids))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": sep_ids must hold 0 .. 4 ids");
    for (int i = 0; i < n_sep; i++)
        if (sep_ids[i] == HUTK_NO_TOKEN)
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": sep_ids must not hold HUTK_NO_TOKEN");
    *s = (bos_id != HUTK_NO_TOKEN) + n_sep + (eos_id != HUTK_NO_TOKEN);
    if (max_len < 1 || max_len < *s + 1 || max_len > INT32_MAX)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": max_len must be above the number of bos/sep/eos tokens and below 2^31");
    if (stride < 0 || stride >= max_len - *s)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": stride must be in 0 .. max_len - s - 1");
    *R = max_len - *s;
    return HUTK_OK;
}

// what the three planners launch alike: one thread per row, d_err cleared first
template <class Args, class Kernel>
int launch_plan(const char* who, Kernel k, Args& a, int64_t n_rows, int64_t* d_plan, hipStream_t st) {
    if (!aligned_to(d_plan, 8)) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": d_plan must be 8-byte aligned");
    const int64_t blocks = (n_rows + TB - 1) / TB;
    if (blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, std::string(who) + ": the batch is too large for one launch");
    if (a.r.err) HUTK_HIP_TRY(hipMemsetAsync(a.r.err, 0, sizeof(int32_t), st));
    if (blocks == 0) return HUTK_OK;
    const PlanOut o{d_plan, aligned_to(d_plan, 16)};
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(TB), 0, st, a, o);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

// What the two target calls refuse alike before anything else: the shape of the rows and a fill that does not fit them
int target_sizes(const char* who, int64_t n_rows, int64_t max_len, int width, int64_t ignore_index) {
    if (n_rows < 0 || (width != 4 && width != 8))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": bad arguments (width is 4 or 8)");
    if (max_len < 1 || max_len > INT32_MAX)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": max_len must be in 1 .. 2^31 - 1");
    if (width == 4 && (ignore_index < INT32_MIN || ignore_index > INT32_MAX))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": ignore_index must fit the rows' width");
    return HUTK_OK;
}

// a buffer of np bytes at p and one of nq bytes at q that share a byte
bool overlap(const void* p, int64_t np, const void* q, int64_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

}  // namespace

struct hutk_chat_template {
    int device = 0;
    ChatTable h = {};        // the table on the host, for the sizes
    ChatTable* d = nullptr;  // and on the device: written once, read-only afterwards
};

namespace {

// What the three chat calls refuse alike before anything else.  fixed = [bos] + |tail| and the tail's length come back.
int chat_sizes(const char* who, const hutk_chat_template* t, int64_t n_conv, int64_t n_turns, int64_t n_ids, int gen_role,
               int64_t* fixed, int32_t* tail_len) {
    if (!t) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": the template is NULL");
    if (n_conv < 0 || n_turns < 0 || n_ids < 0 || n_conv > INT32_MAX - 1 || n_turns > INT32_MAX - 1)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": counts must not be negative, n_conv and n_turns below 2^31 - 1");
    if (gen_role < -1 || gen_role >= t->h.n_roles)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": gen_role must be -1 or a role of the template");
    if (gen_role >= 0 && t->h.eos != HUTK_NO_TOKEN)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a generation prompt and an eos exclude each other");
    *tail_len = gen_role >= 0 ? t->h.plen[gen_role] : t->h.eos != HUTK_NO_TOKEN;
    *fixed = (t->h.bos != HUTK_NO_TOKEN) + *tail_len;
    return HUTK_OK;
}

// What the fill-in-the-middle calls refuse alike before anything else (a call without a draw passes 0 for the last three)
int fim_sizes(const char* who, int64_t n_docs, int64_t n_ids, int64_t first_doc, int64_t fim_below, int64_t spm_below) {
    constexpr int64_t ONE = (int64_t)1 << 32;
    if (n_docs < 0 || n_ids < 0 || n_docs > INT32_MAX - 1)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": counts must not be negative, n_docs below 2^31 - 1");
    if (first_doc < 0 || first_doc > INT64_MAX - n_docs)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": first_doc must not be negative, first_doc + n_docs below 2^63");
    if (fim_below < 0 || fim_below > ONE || spm_below < 0 || spm_below > ONE)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": the thresholds must lie in 0 .. 2^32");
    return HUTK_OK;
}

// What the two plan calls do alike: the rows scan over "rendered length of document i", then the plan rows
int fim_plan(const char* who, FimDocs& docs, int64_t n_docs, int64_t n_ids, int has_end, int64_t* d_out_offsets,
             int64_t* d_plan, int32_t* d_kinds_out, int32_t* d_err, hipStream_t st) {
    if (!d_out_offsets || (n_docs > 0 && (!docs.offs || !d_plan || (!docs.kinds_in && !d_kinds_out))))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(docs.offs, 8) || !aligned_to(d_out_offsets, 8) || !aligned_to(d_plan, 8) || !aligned_to(d_kinds_out, 4) ||
        !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its element type");
    if (int rc = device_present(who)) return rc;
    docs.n_docs = n_docs;
    docs.n_ids = n_ids;
    docs.E = has_end ? 1 : 0;
    if (int rc = rows_scan(docs, n_docs, d_out_offsets, d_err, st)) return rc;  // (clears *d_err; n_docs == 0: out_offsets[0] = 0)
    if (n_docs == 0) return HUTK_OK;
    hipLaunchKernelGGL(k_fim_plan, dim3((unsigned)((n_docs + TB - 1) / TB)), dim3(TB), 0, st, docs, d_plan, d_kinds_out);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

}  // namespace

struct hutk_packer {
    int device = 0;
    int64_t L = 0;
    int32_t bos = HUTK_NO_TOKEN, eos = HUTK_NO_TOKEN, pad = 0;
    int width = 4;
    int64_t pending = 0;
    int cur = 0;                 // which half of the carry holds the pending tokens
    int32_t* carry = nullptr;    // [2][3][L]: ids, positions, segments
    hipEvent_t ev = nullptr;     // behind the last kernel of the last call
    bool ev_recorded = false;
    std::mutex mu;
    // channels: the width, the record size and the fill of each, and one carry of [2][L] records for all
    int n_ch = 0;
    int ch_width[HUTK_PACKER_MAX_CHANNELS] = {}, ch_per[HUTK_PACKER_MAX_CHANNELS] = {};
    int64_t ch_fill[HUTK_PACKER_MAX_CHANNELS] = {};
    int64_t ch_at[HUTK_PACKER_MAX_CHANNELS] = {};  // where the channel's two halves begin in ch_carry, a multiple of 16
    char* ch_carry = nullptr;
    int s() const { return (bos != HUTK_NO_TOKEN) + (eos != HUTK_NO_TOKEN); }
    int32_t* half(int h, int which) const { return carry + ((int64_t)h * 3 + which) * L; }
    int64_t ch_rec(int c) const { return (int64_t)ch_width[c] * ch_per[c]; }
    char* ch_half(int h, int c) const { return ch_carry + ch_at[c] + h * L * ch_rec(c); }
};

namespace {

// What the kernels read of the packer's channels: the caller's arrays (NULL where the call has none: flush reads no
// values), the halves of the carry the call consumes and leaves, and the fill as the dwords of a record.
PackChans pack_chans(const hutk_packer* p, const void* const* d_values, void* const* d_rows) {
    PackChans ch = {};
    ch.n = p->n_ch;
    for (int c = 0; c < p->n_ch; c++) {
        PackChan& k = ch.c[c];
        k.values = d_values ? d_values[c] : nullptr;
        k.rows = d_rows ? d_rows[c] : nullptr;
        k.c_car = p->ch_half(p->cur, c);
        k.n_car = p->ch_half(p->cur ^ 1, c);
        k.w8 = p->ch_width[c] == 8;
        k.words = (int32_t)(p->ch_rec(c) / 4);
        const int32_t lo = (int32_t)(uint32_t)(uint64_t)p->ch_fill[c], hi = (int32_t)(uint32_t)((uint64_t)p->ch_fill[c] >> 32);
        if (k.w8) k.f0 = lo, k.f1 = hi, k.f2 = lo, k.f3 = hi;
        else k.f0 = k.f1 = k.f2 = k.f3 = lo;
    }
    return ch;
}

// The pointers of a call with channels: every one given and aligned to its elements.  *wide: all rows 16-byte aligned.
int chan_pointers(const char* who, const hutk_packer* p, const void* const* d_values, bool need_values, void* const* d_rows,
                  bool need_rows, bool* wide) {
    *wide = true;
    if (p->n_ch == 0) return HUTK_OK;
    if ((need_values && !d_values) || (need_rows && !d_rows))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": the packer has channels: d_values and d_channel_rows must be given");
    for (int c = 0; c < p->n_ch; c++) {
        if ((need_values && !d_values[c]) || (need_rows && !d_rows[c]))
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a channel's buffer is NULL");
        if ((need_values && !aligned_to(d_values[c], (uintptr_t)p->ch_width[c])) ||
            (need_rows && !aligned_to(d_rows[c], (uintptr_t)p->ch_width[c])))
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a channel's buffer is not aligned to its elements");
        if (need_rows && !aligned_to(d_rows[c], 16)) *wide = false;
    }
    return HUTK_OK;
}

}  // namespace

extern "C" {

int hutk_collate_padded_device(const int32_t* d_ids, const int64_t* d_offsets, int64_t n_docs, int64_t n_ids,
                               int64_t max_len, int32_t bos_id, int32_t eos_id, int32_t pad_id, int flags,
                               int out_width, void* d_input_ids, uint8_t* d_mask, int32_t* d_lengths, int32_t* d_err,
                               void* hip_stream) {
    const int s = (bos_id != HUTK_NO_TOKEN) + (eos_id != HUTK_NO_TOKEN);
    if (n_docs < 0 || n_ids < 0 || (out_width != 4 && out_width != 8) ||
        (flags & ~(HUTK_COLLATE_TRUNC_LEFT | HUTK_COLLATE_PAD_LEFT)))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_padded_device: bad arguments");
    if (max_len < 1 || max_len < s || max_len > INT32_MAX)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_padded_device: max_len must be at least 1 and the number of "
                                               "bos/eos tokens, and below 2^31");
    if (int rc = device_present("hutk_collate_padded_device")) return rc;
    if (n_docs == 0) return HUTK_OK;
    if (!d_offsets || !d_input_ids || (n_ids > 0 && !d_ids))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_padded_device: a buffer is NULL");
    PadArgs a;
    a.r = row_args(max_len, s, bos_id, eos_id, pad_id, flags, d_input_ids, d_mask, nullptr, d_lengths, nullptr, d_err);
    a.r.ids_a = d_ids;
    a.r.cap_a = n_ids;
    a.offs = d_offsets;
    a.n_docs = n_docs;
    a.trunc_left = (flags & HUTK_COLLATE_TRUNC_LEFT) != 0;
    int64_t blocks;
    bool vec;
    if (int rc = row_grid("hutk_collate_padded_device", a.r, n_docs, &blocks, &vec)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    with_width_vec(out_width, vec, [&](auto w, auto v) {
        hipLaunchKernelGGL((k_collate_padded<decltype(w)::value, decltype(v)::value>), dim3((unsigned)blocks), dim3(TB), 0, st, a);
    });
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int64_t hutk_windows_rows_bound(int64_t n_docs, int64_t n_ids, int64_t max_len, int64_t stride, int s) {
    int64_t C, step;
    if (n_docs < 0 || n_ids < 0 || s < 0 || s > 2) {
        hutk::api_set_error(HUTK_E_ARG, "hutk_windows_rows_bound: bad arguments");
        return -HUTK_E_ARG;
    }
    if (window_sizes("hutk_windows_rows_bound", max_len, stride, s, &C, &step)) return -HUTK_E_ARG;
    return n_docs + n_ids / step;  // ceil((n - C) / step) <= n / step, as step <= C
}

int hutk_windows_rows_device(const int64_t* d_offsets, int64_t n_docs, int64_t n_ids, int64_t max_len, int64_t stride,
                             int32_t bos_id, int32_t eos_id, int64_t* d_row_offsets, int32_t* d_err, void* hip_stream) {
    const int s = (bos_id != HUTK_NO_TOKEN) + (eos_id != HUTK_NO_TOKEN);
    if (n_docs < 0 || n_ids < 0) return hutk::api_set_error(HUTK_E_ARG, "hutk_windows_rows_device: bad arguments");
    DocRows rows;
    if (int rc = window_sizes("hutk_windows_rows_device", max_len, stride, s, &rows.C, &rows.step)) return rc;
    if (int rc = device_present("hutk_windows_rows_device")) return rc;
    if (!d_row_offsets || (n_docs > 0 && !d_offsets))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_windows_rows_device: a buffer is NULL");
    rows.offs = d_offsets;
    rows.n_docs = n_docs;
    rows.n_ids = n_ids;
    return rows_scan(rows, n_docs, d_row_offsets, d_err, (hipStream_t)hip_stream);
}

int hutk_collate_windows_device(const int32_t* d_ids, const int64_t* d_offsets, const int64_t* d_row_offsets,
                                int64_t n_docs, int64_t n_ids, int64_t n_rows, int64_t max_len, int64_t stride,
                                int32_t bos_id, int32_t eos_id, int32_t pad_id, int flags, int out_width,
                                void* d_input_ids, uint8_t* d_mask, int32_t* d_lengths, int64_t* d_row_map,
                                int32_t* d_err, void* hip_stream) {
    const int s = (bos_id != HUTK_NO_TOKEN) + (eos_id != HUTK_NO_TOKEN);
    if (n_docs < 0 || n_ids < 0 || n_rows < 0 || (out_width != 4 && out_width != 8) || (flags & ~HUTK_COLLATE_PAD_LEFT))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_windows_device: bad arguments (of the flags, only "
                                               "HUTK_COLLATE_PAD_LEFT applies)");
    int64_t C, step;
    if (int rc = window_sizes("hutk_collate_windows_device", max_len, stride, s, &C, &step)) return rc;
    if (int rc = device_present("hutk_collate_windows_device")) return rc;
    if (n_docs == 0) return HUTK_OK;
    if (!d_offsets || !d_row_offsets || (n_rows > 0 && !d_input_ids) || (n_ids > 0 && !d_ids))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_windows_device: a buffer is NULL");
    WinArgs a;
    a.r = row_args(max_len, s, bos_id, eos_id, pad_id, flags, d_input_ids, d_mask, nullptr, d_lengths, d_row_map, d_err);
    a.r.ids_a = d_ids;
    a.r.cap_a = n_ids;
    a.offs = d_offsets;
    a.rows = d_row_offsets;
    a.n_docs = n_docs;
    a.n_rows = n_rows;
    a.C = (int32_t)C;
    a.step = (int32_t)step;
    int64_t blocks;
    bool vec;
    if (int rc = row_grid("hutk_collate_windows_device", a.r, n_rows, &blocks, &vec)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    with_width_vec(out_width, vec, [&](auto w, auto v) {
        hipLaunchKernelGGL((k_collate_windows<decltype(w)::value, decltype(v)::value>), dim3((unsigned)blocks), dim3(TB), 0, st, a);
    });
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int64_t hutk_pair_rows_bound(int64_t n_pairs, int64_t n_cut_ids, int64_t max_len, int64_t stride, int s) {
    int64_t C, step;
    if (n_pairs < 0 || n_cut_ids < 0 || s < 0 || s > 2 + HUTK_PAIR_MAX_SEP) {
        hutk::api_set_error(HUTK_E_ARG, "hutk_pair_rows_bound: bad arguments");
        return -HUTK_E_ARG;
    }
    if (window_sizes("hutk_pair_rows_bound", max_len, stride, s, &C, &step)) return -HUTK_E_ARG;
    return n_pairs + n_cut_ids;  // a pair of n > C >= 1 cut ids has 1 + ceil((n - C) / step) <= n rows, as step >= 1
}

int hutk_pair_rows_device(const int64_t* d_offsets_a, const int64_t* d_offsets_b, int64_t n_pairs, int64_t cap_a,
                          int64_t cap_b, int64_t max_len, int64_t stride, int strategy, int32_t bos_id,
                          const int32_t* sep_ids, int n_sep, int32_t eos_id, int64_t* d_row_offsets, int32_t* d_err,
                          void* hip_stream) {
    if (n_pairs < 0 || cap_a < 0 || cap_b < 0) return hutk::api_set_error(HUTK_E_ARG, "hutk_pair_rows_device: bad arguments");
    int s;
    PairRows rows;
    if (int rc = pair_sizes("hutk_pair_rows_device", max_len, stride, strategy, bos_id, sep_ids, n_sep, eos_id, &s, &rows.R))
        return rc;
    if (strategy == HUTK_PAIR_LONGEST_FIRST)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pair_rows_device: strategy must name the side that is cut into windows "
                                               "(HUTK_PAIR_ONLY_FIRST or HUTK_PAIR_ONLY_SECOND)");
    if (int rc = device_present("hutk_pair_rows_device")) return rc;
    if (!d_row_offsets || (n_pairs > 0 && (!d_offsets_a || !d_offsets_b)))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pair_rows_device: a buffer is NULL");
    rows.offs_a = d_offsets_a;
    rows.offs_b = d_offsets_b;
    rows.cap_a = cap_a;
    rows.cap_b = cap_b;
    rows.stride = stride;
    rows.cut_b = strategy == HUTK_PAIR_ONLY_SECOND;
    return rows_scan(rows, n_pairs, d_row_offsets, d_err, (hipStream_t)hip_stream);
}

int hutk_collate_pairs_device(const int32_t* d_ids_a, const int64_t* d_offsets_a, const int32_t* d_ids_b,
                              const int64_t* d_offsets_b, const int64_t* d_row_offsets, int64_t n_pairs, int64_t cap_a,
                              int64_t cap_b, int64_t n_rows, int64_t max_len, int64_t stride, int strategy,
                              int32_t bos_id, const int32_t* sep_ids, int n_sep, int32_t eos_id, int32_t pad_id,
                              int flags, int out_width, void* d_input_ids, uint8_t* d_mask, uint8_t* d_token_types,
                              int32_t* d_lengths, int64_t* d_row_map, int32_t* d_err, void* hip_stream) {
    if (n_pairs < 0 || cap_a < 0 || cap_b < 0 || n_rows < 0 || (out_width != 4 && out_width != 8) ||
        (flags & ~HUTK_COLLATE_PAD_LEFT))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_pairs_device: bad arguments (of the flags, only "
                                               "HUTK_COLLATE_PAD_LEFT applies)");
    int s;
    int64_t R;
    if (int rc = pair_sizes("hutk_collate_pairs_device", max_len, stride, strategy, bos_id, sep_ids, n_sep, eos_id, &s, &R))
        return rc;
    if (d_row_offsets && strategy == HUTK_PAIR_LONGEST_FIRST)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_pairs_device: with d_row_offsets the strategy must name the side "
                                               "that is cut into windows (HUTK_PAIR_ONLY_FIRST or HUTK_PAIR_ONLY_SECOND)");
    if (!d_row_offsets && n_rows != n_pairs)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_pairs_device: without d_row_offsets n_rows must be n_pairs");
    if (int rc = device_present("hutk_collate_pairs_device")) return rc;
    if (n_pairs == 0) return HUTK_OK;
    if (!d_offsets_a || !d_offsets_b || (n_rows > 0 && !d_input_ids) || (cap_a > 0 && !d_ids_a) || (cap_b > 0 && !d_ids_b))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_collate_pairs_device: a buffer is NULL");
    PairArgs a;
    a.r = row_args(max_len, s, bos_id, eos_id, pad_id, flags, d_input_ids, d_mask, d_token_types, d_lengths, d_row_map, d_err);
    a.r.ids_a = d_ids_a;
    a.r.ids_b = d_ids_b;
    a.r.cap_a = cap_a;
    a.r.cap_b = cap_b;
    a.r.sep0 = n_sep > 0 ? sep_ids[0] : 0;
    a.r.sep1 = n_sep > 1 ? sep_ids[1] : 0;
    a.r.sep2 = n_sep > 2 ? sep_ids[2] : 0;
    a.r.sep3 = n_sep > 3 ? sep_ids[3] : 0;
    a.r.n_sep = n_sep;
    a.offs_a = d_offsets_a;
    a.offs_b = d_offsets_b;
    a.rows = d_row_offsets;
    a.n_pairs = n_pairs;
    a.n_rows = n_rows;
    a.R = (int32_t)R;
    a.stride = (int32_t)stride;
    a.strategy = strategy;
    int64_t blocks;
    bool vec;
    if (int rc = row_grid("hutk_collate_pairs_device", a.r, n_rows, &blocks, &vec)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    with_width_vec(out_width, vec, [&](auto w, auto v) {
        hipLaunchKernelGGL((k_collate_pairs<decltype(w)::value, decltype(v)::value>), dim3((unsigned)blocks), dim3(TB), 0, st, a);
    });
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

// ---- row plans, the gather and the answer positions ---------------------------------------------------------
int hutk_padded_plan_device(const int64_t* d_offsets, int64_t n_docs, int64_t n_ids, int64_t max_len, int32_t bos_id,
                            int32_t eos_id, int flags, int64_t* d_plan, int32_t* d_err, void* hip_stream) {
    const int s = (bos_id != HUTK_NO_TOKEN) + (eos_id != HUTK_NO_TOKEN);
    if (n_docs < 0 || n_ids < 0 || (flags & ~(HUTK_COLLATE_TRUNC_LEFT | HUTK_COLLATE_PAD_LEFT)))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_padded_plan_device: bad arguments");
    if (max_len < 1 || max_len < s || max_len > INT32_MAX)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_padded_plan_device: max_len must be at least 1 and the number of "
                                               "bos/eos tokens, and below 2^31");
    if (int rc = device_present("hutk_padded_plan_device")) return rc;
    if (n_docs == 0) return HUTK_OK;
    if (!d_offsets || !d_plan) return hutk::api_set_error(HUTK_E_ARG, "hutk_padded_plan_device: a buffer is NULL");
    PadArgs a;
    a.r = row_args(max_len, s, bos_id, eos_id, 0, flags, nullptr, nullptr, nullptr, nullptr, nullptr, d_err);
    a.r.cap_a = n_ids;
    a.offs = d_offsets;
    a.n_docs = n_docs;
    a.trunc_left = (flags & HUTK_COLLATE_TRUNC_LEFT) != 0;
    return launch_plan("hutk_padded_plan_device", k_plan_padded, a, n_docs, d_plan, (hipStream_t)hip_stream);
}

int hutk_windows_plan_device(const int64_t* d_offsets, const int64_t* d_row_offsets, int64_t n_docs, int64_t n_ids,
                             int64_t n_rows, int64_t max_len, int64_t stride, int32_t bos_id, int32_t eos_id, int flags,
                             int64_t* d_plan, int32_t* d_err, void* hip_stream) {
    const int s = (bos_id != HUTK_NO_TOKEN) + (eos_id != HUTK_NO_TOKEN);
    if (n_docs < 0 || n_ids < 0 || n_rows < 0 || (flags & ~HUTK_COLLATE_PAD_LEFT))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_windows_plan_device: bad arguments (of the flags, only "
                                               "HUTK_COLLATE_PAD_LEFT applies)");
    int64_t C, step;
    if (int rc = window_sizes("hutk_windows_plan_device", max_len, stride, s, &C, &step)) return rc;
    if (int rc = device_present("hutk_windows_plan_device")) return rc;
    if (n_docs == 0) return HUTK_OK;
    if (!d_offsets || !d_row_offsets || (n_rows > 0 && !d_plan))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_windows_plan_device: a buffer is NULL");
    WinArgs a;
    a.r = row_args(max_len, s, bos_id, eos_id, 0, flags, nullptr, nullptr, nullptr, nullptr, nullptr, d_err);
    a.r.cap_a = n_ids;
    a.offs = d_offsets;
    a.rows = d_row_offsets;
    a.n_docs = n_docs;
    a.n_rows = n_rows;
    a.C = (int32_t)C;
    a.step = (int32_t)step;
    return launch_plan("hutk_windows_plan_device", k_plan_windows, a, n_rows, d_plan, (hipStream_t)hip_stream);
}

int hutk_pair_plan_device(const int64_t* d_offsets_a, const int64_t* d_offsets_b, const int64_t* d_row_offsets,
                          int64_t n_pairs, int64_t cap_a, int64_t cap_b, int64_t n_rows, int64_t max_len, int64_t stride,
                          int strategy, int32_t bos_id, const int32_t* sep_ids, int n_sep, int32_t eos_id, int flags,
                          int64_t* d_plan, int32_t* d_err, void* hip_stream) {
    if (n_pairs < 0 || cap_a < 0 || cap_b < 0 || n_rows < 0 || (flags & ~HUTK_COLLATE_PAD_LEFT))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pair_plan_device: bad arguments (of the flags, only "
                                               "HUTK_COLLATE_PAD_LEFT applies)");
    int s;
    int64_t R;
    if (int rc = pair_sizes("hutk_pair_plan_device", max_len, stride, strategy, bos_id, sep_ids, n_sep, eos_id, &s, &R))
        return rc;
    if (d_row_offsets && strategy == HUTK_PAIR_LONGEST_FIRST)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pair_plan_device: with d_row_offsets the strategy must name the side "
                                               "that is cut into windows (HUTK_PAIR_ONLY_FIRST or HUTK_PAIR_ONLY_SECOND)");
    if (!d_row_offsets && n_rows != n_pairs)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pair_plan_device: without d_row_offsets n_rows must be n_pairs");
    if (int rc = device_present("hutk_pair_plan_device")) return rc;
    if (n_pairs == 0) return HUTK_OK;
    if (!d_offsets_a || !d_offsets_b || (n_rows > 0 && !d_plan))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pair_plan_device: a buffer is NULL");
    PairArgs a;
    a.r = row_args(max_len, s, bos_id, eos_id, 0, flags, nullptr, nullptr, nullptr, nullptr, nullptr, d_err);
    a.r.cap_a = cap_a;
    a.r.cap_b = cap_b;
    a.r.n_sep = n_sep;
    a.offs_a = d_offsets_a;
    a.offs_b = d_offsets_b;
    a.rows = d_row_offsets;
    a.n_pairs = n_pairs;
    a.n_rows = n_rows;
    a.R = (int32_t)R;
    a.stride = (int32_t)stride;
    a.strategy = strategy;
    return launch_plan("hutk_pair_plan_device", k_plan_pairs, a, n_rows, d_plan, (hipStream_t)hip_stream);
}

int hutk_rows_gather_device(const int64_t* d_plan, int64_t n_rows, int64_t max_len, const void* d_values_a, int64_t n_a,
                            const void* d_values_b, int64_t n_b, int rec_bytes, const void* fill, void* d_out,
                            int32_t* d_err, void* hip_stream) {
    if (n_rows < 0 || n_a < 0 || n_b < 0 || (rec_bytes != 4 && rec_bytes != 8 && rec_bytes != 16) || !fill)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_rows_gather_device: bad arguments (rec_bytes is 4, 8 or 16)");
    if (max_len < 1 || max_len > INT32_MAX)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_rows_gather_device: max_len must be in 1 .. 2^31 - 1");
    if (int rc = device_present("hutk_rows_gather_device")) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_rows == 0) return HUTK_OK;
    if (!d_plan || !d_out || (n_a > 0 && !d_values_a) || (n_b > 0 && !d_values_b))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_rows_gather_device: a buffer is NULL");
    const uintptr_t least = rec_bytes == 16 ? 8 : 4;  // a record is one or two int32 or int64
    if (!aligned_to(d_plan, 8) || !aligned_to(d_out, least) || !aligned_to(d_values_a, least) || !aligned_to(d_values_b, least))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_rows_gather_device: a buffer is not aligned to its elements");
    GatherArgs a = {};
    a.r.L = (int32_t)max_len;
    a.r.err = d_err;
    a.plan = d_plan;
    a.n_rows = n_rows;
    a.va = d_values_a;
    a.vb = d_values_b;
    a.n_a = n_a;
    a.n_b = n_b;
    int32_t f[4] = {0, 0, 0, 0};
    memcpy(f, fill, (size_t)rec_bytes);
    a.f0 = f[0], a.f1 = f[1], a.f2 = f[2], a.f3 = f[3];
    a.out = d_out;
    int64_t blocks;
    bool vec;
    if (int rc = row_grid("hutk_rows_gather_device", a.r, n_rows, &blocks, &vec)) return rc;
    const bool wide = max_len * rec_bytes % 16 == 0 && aligned_to(d_out, 16) && aligned_to(d_values_a, (uintptr_t)rec_bytes) &&
                      aligned_to(d_values_b, (uintptr_t)rec_bytes);
    const dim3 grid((unsigned)blocks), block(TB);
    auto launch = [&](auto rec) {
        constexpr int REC = decltype(rec)::value;
        if (wide) hipLaunchKernelGGL((k_rows_gather<REC, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_rows_gather<REC, false>), grid, block, 0, st, a);
    };
    if (rec_bytes == 4) launch(std::integral_constant<int, 4>{});
    else if (rec_bytes == 8) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 16>{});
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_rows_answers_device(const int64_t* d_plan, int64_t n_rows, int side, const void* d_spans, int span_width,
                             int64_t n_spans, const void* d_answers, int64_t n_items, int32_t* d_out, int32_t* d_err,
                             void* hip_stream) {
    if (n_rows < 0 || n_spans < 0 || n_items < 0 || (side != 0 && side != 1) || (span_width != 4 && span_width != 8))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_rows_answers_device: bad arguments (side is 0 for A or 1 for B, "
                                               "span_width 4 or 8)");
    if (int rc = device_present("hutk_rows_answers_device")) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_rows == 0) return HUTK_OK;
    if (!d_plan || !d_out || (n_spans > 0 && !d_spans) || (n_items > 0 && !d_answers))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_rows_answers_device: a buffer is NULL");
    if (!aligned_to(d_plan, 8) || !aligned_to(d_spans, (uintptr_t)span_width) || !aligned_to(d_answers, (uintptr_t)span_width) ||
        !aligned_to(d_out, 4))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_rows_answers_device: a buffer is not aligned to its elements");
    const int64_t blocks = (n_rows + TB / 64 - 1) / (TB / 64);
    if (blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, "hutk_rows_answers_device: the batch is too large for one launch");
    const AnsArgs a{d_plan, n_rows, d_spans, n_spans, d_answers, n_items, d_out, d_err, side};
    if (span_width == 4) hipLaunchKernelGGL(k_rows_answers<int32_t>, dim3((unsigned)blocks), dim3(TB), 0, st, a);
    else hipLaunchKernelGGL(k_rows_answers<int64_t>, dim3((unsigned)blocks), dim3(TB), 0, st, a);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

// ---- targets: masked-LM corruption and loss labels ----------------------------------------------------------
int hutk_rows_mlm_device(const int64_t* d_plan, int64_t n_rows, int64_t max_len, const void* d_input_ids, int width,
                         const int32_t* d_words_a, int64_t n_a, const int32_t* d_words_b, int64_t n_b, uint64_t seed,
                         int64_t select_below, int64_t mask_below, int64_t random_below, int32_t mask_id,
                         int64_t vocab_size, int64_t ignore_index, int sides, void* d_out_ids, void* d_labels,
                         int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_rows_mlm_device";
    constexpr int64_t ONE = (int64_t)1 << 32;
    if (int rc = target_sizes(who, n_rows, max_len, width, ignore_index)) return rc;
    const bool words = d_words_a != nullptr;
    if (words && (n_a < 0 || n_b < 0)) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": bad arguments (negative counts)");
    if (select_below < 0 || select_below > ONE || mask_below < 0 || mask_below > random_below || random_below > ONE)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": the thresholds must be 0 <= select_below <= 2^32 and "
                                                                  "0 <= mask_below <= random_below <= 2^32");
    if (vocab_size < 1 || vocab_size > ((int64_t)1 << 31))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": vocab_size must be in 1 .. 2^31");
    if ((sides & ~(HUTK_MLM_SIDE_A | HUTK_MLM_SIDE_B)) || !sides)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": sides must be HUTK_MLM_SIDE_A, HUTK_MLM_SIDE_B or both");
    MlmArgs a = {};
    a.r.L = (int32_t)max_len;
    a.r.err = d_err;
    int64_t blocks;
    bool vec;
    if (int rc = row_grid(who, a.r, n_rows, &blocks, &vec)) return rc;
    if (!aligned_to(d_err, 4)) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
    if (n_rows > 0) {
        if (!d_plan || !d_input_ids || !d_out_ids || !d_labels)
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
        if (!aligned_to(d_plan, 8) || !aligned_to(d_input_ids, (uintptr_t)width) || !aligned_to(d_out_ids, (uintptr_t)width) ||
            !aligned_to(d_labels, (uintptr_t)width) || !aligned_to(d_words_a, 4) || !aligned_to(d_words_b, 4))
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
        const int64_t bytes = n_rows * max_len * width;  // (no overflow: row_grid has bounded the rows)
        if (overlap(d_labels, bytes, d_input_ids, bytes) || overlap(d_labels, bytes, d_out_ids, bytes) ||
            (d_out_ids != d_input_ids && overlap(d_out_ids, bytes, d_input_ids, bytes)))
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": d_labels must not overlap d_input_ids or d_out_ids, and "
                                                                      "d_out_ids must be d_input_ids or apart from it");
    }
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_rows == 0) return HUTK_OK;
    a.plan = d_plan;
    a.n_rows = n_rows;
    a.ids = d_input_ids;
    a.out = d_out_ids;
    a.labels = d_labels;
    a.wa = d_words_a;
    a.wb = d_words_b ? d_words_b : d_words_a;
    a.n_a = n_a;
    a.n_b = d_words_b ? n_b : n_a;
    a.seed = seed;
    a.select_below = (uint64_t)select_below;
    a.mask_below = (uint64_t)mask_below;
    a.random_below = (uint64_t)random_below;
    a.vocab = (uint64_t)vocab_size;
    a.ignore = ignore_index;
    a.mask_id = mask_id;
    a.sides = sides;
    vec = max_len % 4 == 0 && aligned_to(d_input_ids, 16) && aligned_to(d_out_ids, 16) && aligned_to(d_labels, 16);
    const dim3 grid((unsigned)blocks), block(TB);
    with_width_vec(width, vec, [&](auto w, auto v) {
        constexpr int W = decltype(w)::value;
        constexpr bool VEC = decltype(v)::value;
        if (words) hipLaunchKernelGGL((k_rows_mlm<W, VEC, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_rows_mlm<W, VEC, false>), grid, block, 0, st, a);
    });
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_rows_labels_device(const int64_t* d_plan, int64_t n_rows, int64_t max_len, const void* d_input_ids, int width,
                            const uint8_t* d_mask, int flags, int64_t ignore_index, void* d_labels, int32_t* d_err,
                            void* hip_stream) {
    const char* who = "hutk_rows_labels_device";
    constexpr int SELECTING = HUTK_LABELS_A | HUTK_LABELS_B | HUTK_LABELS_TEMPLATE | HUTK_LABELS_END;
    if (int rc = target_sizes(who, n_rows, max_len, width, ignore_index)) return rc;
    if ((flags & ~(SELECTING | HUTK_LABELS_SHIFT)) || !(flags & SELECTING))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": flags must hold HUTK_LABELS_* only, and one of A, B, "
                                                                  "TEMPLATE and END at least");
    LabelArgs a = {};
    a.r.L = (int32_t)max_len;
    a.r.err = d_err;
    int64_t blocks;
    bool vec;
    if (int rc = row_grid(who, a.r, n_rows, &blocks, &vec)) return rc;
    if (!aligned_to(d_err, 4)) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
    if (n_rows > 0) {
        if (!d_plan || !d_input_ids || !d_mask || !d_labels)
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
        if (!aligned_to(d_plan, 8) || !aligned_to(d_input_ids, (uintptr_t)width) || !aligned_to(d_labels, (uintptr_t)width))
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
        const int64_t bytes = n_rows * max_len * width;  // (no overflow: row_grid has bounded the rows)
        if (overlap(d_labels, bytes, d_input_ids, bytes) || overlap(d_labels, bytes, d_mask, n_rows * max_len))
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": d_labels must not overlap d_input_ids or d_mask");
    }
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_rows == 0) return HUTK_OK;
    a.plan = d_plan;
    a.n_rows = n_rows;
    a.ids = d_input_ids;
    a.mask = d_mask;
    a.labels = d_labels;
    a.ignore = ignore_index;
    a.flags = flags;
    vec = max_len % 4 == 0 && aligned_to(d_input_ids, 16) && aligned_to(d_labels, 16) && aligned_to(d_mask, 4);
    with_width_vec(width, vec, [&](auto w, auto v) {
        hipLaunchKernelGGL((k_rows_labels<decltype(w)::value, decltype(v)::value>), dim3((unsigned)blocks), dim3(TB), 0, st, a);
    });
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

// ---- targets: span corruption ---------------------------------------------------------------------------------
int hutk_rows_span_corrupt_device(const int64_t* d_plan, int64_t n_rows, int64_t max_len, const void* d_input_ids, int width,
                                  const uint8_t* d_mask, uint64_t seed, int64_t start_below, const int64_t* len_below,
                                  int n_len, int64_t sentinel_first, int sentinel_step, int64_t n_sentinels,
                                  int32_t target_eos_id, int32_t decoder_start_id, int64_t pad_id, int64_t ignore_index,
                                  int sides, int64_t max_target_len, void* d_out_ids, uint8_t* d_out_mask, void* d_labels,
                                  void* d_decoder_ids, int32_t* d_in_lengths, int32_t* d_tgt_lengths, int32_t* d_err,
                                  void* hip_stream) {
    const char* who = "hutk_rows_span_corrupt_device";
    constexpr int64_t ONE = (int64_t)1 << 32;
    const auto refuse = [&](const char* what) { return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": " + what); };
    if (int rc = target_sizes(who, n_rows, max_len, width, ignore_index)) return rc;
    if (max_target_len < 1 || max_target_len > INT32_MAX) return refuse("max_target_len must be in 1 .. 2^31 - 1");
    if (start_below < 0 || start_below > ONE) return refuse("start_below must be in 0 .. 2^32");
    if (!len_below || n_len < 1 || n_len > SPAN_LEN_MAX) return refuse("len_below must hold 1 .. 32 thresholds");
    for (int j = 0; j < n_len; j++)
        if (len_below[j] < (j ? len_below[j - 1] : 0) || len_below[j] > ONE)
            return refuse("len_below must not decrease and must lie in 0 .. 2^32");
    if (len_below[n_len - 1] != ONE) return refuse("the last entry of len_below must be 2^32");
    if (sentinel_step != 1 && sentinel_step != -1) return refuse("sentinel_step must be -1 or +1");
    if (n_sentinels < 0) return refuse("n_sentinels must not be negative");
    const auto fits = [&](__int128 v) { return width == 4 ? v >= INT32_MIN && v <= INT32_MAX : v >= INT64_MIN && v <= INT64_MAX; };
    const __int128 sentinel_last = (__int128)sentinel_first + (__int128)(n_sentinels ? n_sentinels - 1 : 0) * sentinel_step;
    if (!fits(sentinel_first) || !fits(sentinel_last)) return refuse("the first and the last sentinel must fit the rows' width");
    if (!fits(pad_id)) return refuse("pad_id must fit the rows' width");
    if ((sides & ~(HUTK_MLM_SIDE_A | HUTK_MLM_SIDE_B)) || !sides)
        return refuse("sides must be HUTK_MLM_SIDE_A, HUTK_MLM_SIDE_B or both");
    if (!aligned_to(d_err, 4)) return refuse("a buffer is not aligned to its elements");
    const bool dec = decoder_start_id != HUTK_NO_TOKEN;
    if (!dec) d_decoder_ids = nullptr;
    // four rows a workgroup; the row count is bounded first, so that neither the sum below nor a size in bytes overflows
    constexpr int64_t MOST_ROWS = (int64_t)INT32_MAX * (TB / 64);
    int64_t in_bytes = 0, tg_bytes = 0;
    if (n_rows > MOST_ROWS || __builtin_mul_overflow(n_rows, max_len * width, &in_bytes) ||
        __builtin_mul_overflow(n_rows, max_target_len * width, &tg_bytes))
        return hutk::api_set_error(HUTK_E_UNSUPPORTED, std::string(who) + ": the batch is too large for one launch");
    const int64_t blocks = (n_rows + TB / 64 - 1) / (TB / 64);  // <= INT32_MAX
    if (n_rows > 0) {
        if (!d_plan || !d_input_ids || !d_mask || !d_out_ids || !d_out_mask || !d_labels || !d_in_lengths || !d_tgt_lengths ||
            (dec && !d_decoder_ids))
            return refuse("a buffer is NULL");
        const uintptr_t w = (uintptr_t)width;
        if (!aligned_to(d_plan, 8) || !aligned_to(d_input_ids, w) || !aligned_to(d_out_ids, w) || !aligned_to(d_labels, w) ||
            !aligned_to(d_decoder_ids, w) || !aligned_to(d_in_lengths, 4) || !aligned_to(d_tgt_lengths, 4))
            return refuse("a buffer is not aligned to its elements");
        struct Buf {
            const void* p;
            int64_t bytes;
        };
        const Buf in[] = {{d_plan, n_rows * 64}, {d_input_ids, in_bytes}, {d_mask, n_rows * max_len}};
        const Buf out[] = {{d_out_ids, in_bytes},       {d_out_mask, n_rows * max_len}, {d_labels, tg_bytes}, {d_decoder_ids, dec ? tg_bytes : 0},
                           {d_in_lengths, n_rows * 4}, {d_tgt_lengths, n_rows * 4},    {d_err, d_err ? 4 : 0}};
        for (size_t i = 0; i < sizeof(out) / sizeof(out[0]); i++) {
            if (!out[i].bytes) continue;
            for (const Buf& b : in)
                if (overlap(out[i].p, out[i].bytes, b.p, b.bytes)) return refuse("an output must not overlap an input: there is no in-place form");
            for (size_t j = 0; j < i; j++)
                if (out[j].bytes && overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return refuse("the outputs must not overlap each other");
        }
    }
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_rows == 0) return HUTK_OK;
    SpanArgs a = {};
    a.plan = d_plan;
    a.n_rows = n_rows;
    a.ids = d_input_ids;
    a.mask = d_mask;
    a.out = d_out_ids;
    a.labels = d_labels;
    a.dec = d_decoder_ids;
    a.out_mask = d_out_mask;
    a.in_len = d_in_lengths;
    a.tgt_len = d_tgt_lengths;
    a.err = d_err;
    a.seed = seed;
    a.start_below = (uint64_t)start_below;
    a.sentinel_first = sentinel_first;
    a.pad = pad_id;
    a.ignore = ignore_index;
    a.L = (int32_t)max_len;
    a.L_tgt = (int32_t)max_target_len;
    for (int j = 0; j + 1 < n_len && len_below[j] < ONE; j++) a.len_below[a.n_cmp++] = (uint32_t)len_below[j];
    a.step = sentinel_step;
    a.n_sent = n_sentinels > INT32_MAX ? INT32_MAX : (int32_t)n_sentinels;  // (a row has fewer runs than columns)
    a.eos = target_eos_id;
    a.dec_start = decoder_start_id;
    a.sides = sides;
    const bool vec = max_len % 4 == 0 && aligned_to(d_input_ids, 16) && aligned_to(d_mask, 4);
    with_width_vec(width, vec, [&](auto w, auto v) {
        hipLaunchKernelGGL((k_rows_span_corrupt<decltype(w)::value, decltype(v)::value>), dim3((unsigned)blocks), dim3(TB), 0, st, a);
    });
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_packer_create(hutk_packer** out, int64_t seq_len, int32_t bos_id, int32_t eos_id, int32_t pad_id,
                       int out_width, int device) {
    return hutk_packer_create_channels(out, seq_len, bos_id, eos_id, pad_id, out_width, device, 0, nullptr, nullptr, nullptr);
}

int hutk_packer_create_channels(hutk_packer** out, int64_t seq_len, int32_t bos_id, int32_t eos_id, int32_t pad_id,
                                int out_width, int device, int n_channels, const int* widths, const int* per,
                                const int64_t* fills) {
    const std::string who = n_channels ? "hutk_packer_create_channels" : "hutk_packer_create";
    if (!out) return hutk::api_set_error(HUTK_E_ARG, who + ": out is NULL");
    *out = nullptr;
    if (seq_len < 1 || seq_len > INT32_MAX || (out_width != 4 && out_width != 8))
        return hutk::api_set_error(HUTK_E_ARG, who + ": seq_len must be in 1 .. 2^31 - 1 and out_width 4 or 8");
    if (n_channels < 0 || n_channels > HUTK_PACKER_MAX_CHANNELS || (n_channels > 0 && (!widths || !per || !fills)))
        return hutk::api_set_error(HUTK_E_ARG, who + ": n_channels must be in 0 .. HUTK_PACKER_MAX_CHANNELS, with widths, per and fills");
    for (int c = 0; c < n_channels; c++) {
        if ((widths[c] != 4 && widths[c] != 8) || (per[c] != 1 && per[c] != 2))
            return hutk::api_set_error(HUTK_E_ARG, who + ": a channel's width must be 4 or 8 and its per 1 or 2");
        if (widths[c] == 4 && (fills[c] < INT32_MIN || fills[c] > INT32_MAX))
            return hutk::api_set_error(HUTK_E_ARG, who + ": a channel's fill must fit its width");
    }
    int n = 0;
    if (int rc = device_present(who.c_str(), &n)) return rc;
    if (device < 0) HUTK_HIP_TRY(hipGetDevice(&device));
    if (device >= n) return hutk::api_set_error(HUTK_E_DEVICE, who + ": no such device");
    HUTK_HIP_TRY(hipSetDevice(device));
    hutk_packer* p = new hutk_packer();
    p->device = device;
    p->L = seq_len;
    p->bos = bos_id;
    p->eos = eos_id;
    p->pad = pad_id;
    p->width = out_width;
    p->n_ch = n_channels;
    int64_t ch_bytes = 0;
    for (int c = 0; c < n_channels; c++) {
        p->ch_width[c] = widths[c];
        p->ch_per[c] = per[c];
        p->ch_fill[c] = fills[c];
        p->ch_at[c] = ch_bytes;
        ch_bytes += (2 * seq_len * p->ch_rec(c) + 15) / 16 * 16;
    }
    hipError_t e = hipMalloc((void**)&p->carry, (size_t)seq_len * 6 * sizeof(int32_t));
    if (e == hipSuccess && ch_bytes) e = hipMalloc((void**)&p->ch_carry, (size_t)ch_bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        hutk_packer_destroy(p);
        return hutk::api_set_error(e == hipErrorOutOfMemory ? HUTK_E_MEMORY : HUTK_E_DEVICE,
                                   who + ": " + hipGetErrorString(e));
    }
    *out = p;
    return HUTK_OK;
}

int hutk_packer_channel_count(const hutk_packer* p) { return p ? p->n_ch : -1; }

int64_t hutk_packer_rows(const hutk_packer* p, int64_t n_docs, int64_t n_ids) {
    if (!p || n_docs < 0 || n_ids < 0) return -1;
    return (p->pending + n_ids + n_docs * p->s()) / p->L;
}

int64_t hutk_packer_pending(const hutk_packer* p) { return p ? p->pending : -1; }

// the two add calls; `plain`: the one without channels, which a packer that has some refuses
static int packer_add(const std::string& who, bool plain, hutk_packer* p, const int32_t* d_ids, const int64_t* d_offsets,
                      int64_t n_docs, int64_t n_ids, const void* const* d_values, void* d_input_ids, int32_t* d_position_ids,
                      int32_t* d_segment_ids, void* const* d_channel_rows, int64_t rows_cap, int64_t* n_rows, int32_t* d_err,
                      void* hip_stream) {
    if (!p || n_docs < 0 || n_ids < 0 || rows_cap < 0 || n_docs > INT32_MAX - 1)
        return hutk::api_set_error(HUTK_E_ARG, who + ": bad arguments");
    std::lock_guard<std::mutex> lock(p->mu);
    if (plain && p->n_ch)
        return hutk::api_set_error(HUTK_E_ARG, who + ": the packer has channels, whose carry this call would lose: use "
                                                     "hutk_packer_add_channels_device");
    const int s = p->s();
    const int64_t total = p->pending + n_ids + n_docs * s;
    const int64_t rows = total / p->L;
    if (rows > rows_cap)
        return hutk::api_set_error(HUTK_E_CAPACITY, who + ": rows_cap is below hutk_packer_rows()");
    if ((n_docs > 0 && !d_offsets) || (n_ids > 0 && !d_ids) || (rows > 0 && !d_input_ids))
        return hutk::api_set_error(HUTK_E_ARG, who + ": a buffer is NULL");
    bool wide = true;
    if (n_docs > 0)
        if (int rc = chan_pointers(who.c_str(), p, d_values, n_ids > 0, d_channel_rows, rows > 0, &wide)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(p->device));
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_rows) *n_rows = rows;
    if (n_docs == 0) return HUTK_OK;  // nothing joins the stream (n_ids must then be 0)
    const int64_t rows_all = rows + (total > rows * p->L);
    PackArgs a;
    a.ids = d_ids;
    a.offs = d_offsets;
    a.n_docs = n_docs;
    a.n_ids = n_ids;
    a.L = p->L;
    a.P = p->pending;
    a.total = total;
    a.rows = rows;
    a.s = s;
    a.has_bos = p->bos != HUTK_NO_TOKEN;
    a.has_eos = p->eos != HUTK_NO_TOKEN;
    a.bos = p->bos;
    a.eos = p->eos;
    a.c_ids = p->half(p->cur, 0);
    a.c_pos = p->half(p->cur, 1);
    a.c_seg = p->half(p->cur, 2);
    a.n_ids_out = p->half(p->cur ^ 1, 0);
    a.n_pos = p->half(p->cur ^ 1, 1);
    a.n_seg = p->half(p->cur ^ 1, 2);
    a.out = d_input_ids;
    a.pos = d_position_ids;
    a.seg = d_segment_ids;
    a.err = d_err;
    int64_t blocks;
    if (p->L >= SPAN) {
        a.rows_per_block = 1;
        a.spans_per_row = (int32_t)((p->L + SPAN - 1) / SPAN);
        blocks = rows_all * a.spans_per_row;
    } else {
        a.rows_per_block = (int32_t)(SPAN / p->L);
        a.spans_per_row = 1;
        blocks = (rows_all + a.rows_per_block - 1) / a.rows_per_block;
    }
    if (blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, who + ": the batch is too large for one launch");
    if (blocks > 0) {
        if (p->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, p->ev, 0));
        const bool vec = p->L % 4 == 0 && aligned_to(d_input_ids, 16) && aligned_to(d_position_ids, 16) &&
                         aligned_to(d_segment_ids, 16) && wide;
        if (p->n_ch == 0) {
            with_width_vec(p->width, vec, [&](auto w, auto v) {
                hipLaunchKernelGGL((k_collate_packed<decltype(w)::value, decltype(v)::value>), dim3((unsigned)blocks), dim3(TB), 0, st, a);
            });
        } else {
            // (with no complete row the kernel stores to the carry only: the rows' pointers are never used)
            const PackChans ch = pack_chans(p, n_ids > 0 ? d_values : nullptr, rows > 0 ? d_channel_rows : nullptr);
            with_width_vec(p->width, vec, [&](auto w, auto v) {
                hipLaunchKernelGGL((k_collate_packed_ch<decltype(w)::value, decltype(v)::value>), dim3((unsigned)blocks), dim3(TB), 0, st, a, ch);
            });
        }
        HUTK_HIP_TRY(hipGetLastError());
        HUTK_HIP_TRY(hipEventRecord(p->ev, st));
        p->ev_recorded = true;
        p->cur ^= 1;
    }
    p->pending = total - rows * p->L;
    return HUTK_OK;
}

int hutk_packer_add_device(hutk_packer* p, const int32_t* d_ids, const int64_t* d_offsets, int64_t n_docs,
                           int64_t n_ids, void* d_input_ids, int32_t* d_position_ids, int32_t* d_segment_ids,
                           int64_t rows_cap, int64_t* n_rows, int32_t* d_err, void* hip_stream) {
    return packer_add("hutk_packer_add_device", true, p, d_ids, d_offsets, n_docs, n_ids, nullptr, d_input_ids, d_position_ids,
                      d_segment_ids, nullptr, rows_cap, n_rows, d_err, hip_stream);
}

int hutk_packer_add_channels_device(hutk_packer* p, const int32_t* d_ids, const int64_t* d_offsets, int64_t n_docs,
                                    int64_t n_ids, const void* const* d_values, void* d_input_ids,
                                    int32_t* d_position_ids, int32_t* d_segment_ids, void* const* d_channel_rows,
                                    int64_t rows_cap, int64_t* n_rows, int32_t* d_err, void* hip_stream) {
    return packer_add("hutk_packer_add_channels_device", false, p, d_ids, d_offsets, n_docs, n_ids, d_values, d_input_ids,
                      d_position_ids, d_segment_ids, d_channel_rows, rows_cap, n_rows, d_err, hip_stream);
}

static int packer_flush(const std::string& who, bool plain, hutk_packer* p, void* d_input_ids, int32_t* d_position_ids,
                        int32_t* d_segment_ids, void* const* d_channel_rows, int64_t* n_rows, void* hip_stream) {
    if (!p) return hutk::api_set_error(HUTK_E_ARG, who + ": bad arguments");
    std::lock_guard<std::mutex> lock(p->mu);
    if (plain && p->n_ch)
        return hutk::api_set_error(HUTK_E_ARG, who + ": the packer has channels, whose carry this call would lose: use "
                                                     "hutk_packer_flush_channels_device");
    if (p->pending == 0) {
        if (n_rows) *n_rows = 0;
        return HUTK_OK;
    }
    if (!d_input_ids) return hutk::api_set_error(HUTK_E_ARG, who + ": d_input_ids is NULL");
    bool wide;
    if (int rc = chan_pointers(who.c_str(), p, nullptr, false, d_channel_rows, true, &wide)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(p->device));
    if (p->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, p->ev, 0));
    int64_t blocks = (p->L + TB - 1) / TB;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks), block(TB);
    if (p->width == 4)
        hipLaunchKernelGGL((k_collate_flush<4>), grid, block, 0, st, p->half(p->cur, 0), p->half(p->cur, 1),
                           p->half(p->cur, 2), p->pending, p->L, p->pad, d_input_ids, d_position_ids, d_segment_ids);
    else
        hipLaunchKernelGGL((k_collate_flush<8>), grid, block, 0, st, p->half(p->cur, 0), p->half(p->cur, 1),
                           p->half(p->cur, 2), p->pending, p->L, p->pad, d_input_ids, d_position_ids, d_segment_ids);
    if (p->n_ch)
        hipLaunchKernelGGL(k_collate_flush_ch, grid, block, 0, st, pack_chans(p, nullptr, d_channel_rows), p->pending, p->L);
    HUTK_HIP_TRY(hipGetLastError());
    HUTK_HIP_TRY(hipEventRecord(p->ev, st));
    p->ev_recorded = true;
    p->pending = 0;
    if (n_rows) *n_rows = 1;
    return HUTK_OK;
}

int hutk_packer_flush_device(hutk_packer* p, void* d_input_ids, int32_t* d_position_ids, int32_t* d_segment_ids,
                             int64_t* n_rows, void* hip_stream) {
    return packer_flush("hutk_packer_flush_device", true, p, d_input_ids, d_position_ids, d_segment_ids, nullptr, n_rows,
                        hip_stream);
}

int hutk_packer_flush_channels_device(hutk_packer* p, void* d_input_ids, int32_t* d_position_ids,
                                      int32_t* d_segment_ids, void* const* d_channel_rows, int64_t* n_rows,
                                      void* hip_stream) {
    return packer_flush("hutk_packer_flush_channels_device", false, p, d_input_ids, d_position_ids, d_segment_ids,
                        d_channel_rows, n_rows, hip_stream);
}

void hutk_packer_destroy(hutk_packer* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->ev) {
        if (p->ev_recorded) (void)hipEventSynchronize(p->ev);  // nothing is freed under a running kernel
        (void)hipEventDestroy(p->ev);
    }
    if (p->carry) (void)hipFree(p->carry);
    if (p->ch_carry) (void)hipFree(p->ch_carry);
    delete p;
}

// ---- packed rows for training ---------------------------------------------------------------------------
int hutk_packed_cu_seqlens_device(const int32_t* d_segment_ids, int64_t n_rows, int64_t seq_len, int64_t cap,
                                  int32_t* d_cu_seqlens, int32_t* d_info, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_packed_cu_seqlens_device";
    if (n_rows < 0 || seq_len < 1 || seq_len > INT32_MAX || n_rows > INT32_MAX / seq_len)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": n_rows * seq_len must be below 2^31 (the starts are int32), seq_len at least 1");
    if (cap < 0 || cap > INT32_MAX - 1) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": cap must be in 0 .. 2^31 - 2");
    if (!d_info || (n_rows > 0 && !d_segment_ids))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_segment_ids, 4) || !aligned_to(d_cu_seqlens, 4) || !aligned_to(d_info, 4) || !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    const int64_t n = n_rows * seq_len;
    if (n == 0) {
        HUTK_HIP_TRY(hipMemsetAsync(d_info, 0, 2 * sizeof(int32_t), st));
        if (d_cu_seqlens) HUTK_HIP_TRY(hipMemsetAsync(d_cu_seqlens, 0, (size_t)(cap + 1) * sizeof(int32_t), st));
        return HUTK_OK;
    }
    ScanArgs a;
    a.n = n;
    a.per_block = (n + (int64_t)WIN_BLOCKS * CU_TILE - 1) / ((int64_t)WIN_BLOCKS * CU_TILE) * CU_TILE;
    const int64_t blocks = (n + a.per_block - 1) / a.per_block;
    const CuStarts starts{d_segment_ids, seq_len};
    const CuArgs o{d_cu_seqlens, d_info, cap, n};
    std::lock_guard<std::mutex> lock(g_win_mu);
    WinScratch* w;
    if (int rc = scratch_for(st, &w)) return rc;
    a.sums = w->sums;
    a.row_offs = nullptr;
    a.err = d_err;
    const dim3 grid((unsigned)blocks), block(TB);
    hipLaunchKernelGGL(k_rows_count<CuStarts>, grid, block, 0, st, a, starts);
    hutk::launch_scan_i64(w->sums, blocks, st);
    hipLaunchKernelGGL(k_cu_write, grid, block, 0, st, a, starts, o);
    if (d_cu_seqlens && cap > 0) {
        const int64_t most = cap < n ? cap : n;  // sequences that can have been written
        int64_t gb = (most + TB - 1) / TB;
        if (gb > 1024) gb = 1024;
        hipLaunchKernelGGL(k_cu_gaps, dim3((unsigned)gb), block, 0, st, o);
    }
    return scratch_used(w, st);
}

int hutk_packed_labels_device(const void* d_values, int width, const int32_t* d_segment_ids, int64_t n_rows,
                              int64_t seq_len, int shift, int64_t ignore_index, void* d_labels, void* hip_stream) {
    const char* who = "hutk_packed_labels_device";
    if (int rc = target_sizes(who, n_rows, seq_len, width, ignore_index)) return rc;
    if (n_rows > INT64_MAX / 8 / seq_len) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": the rows are too large");
    const int64_t n = n_rows * seq_len;
    if (n > 0) {
        if (!d_values || !d_segment_ids || !d_labels) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
        if (!aligned_to(d_values, (uintptr_t)width) || !aligned_to(d_labels, (uintptr_t)width) || !aligned_to(d_segment_ids, 4))
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
        if (overlap(d_labels, n * width, d_values, n * width) || overlap(d_labels, n * width, d_segment_ids, n * 4))
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": d_labels must not overlap d_values or d_segment_ids");
    }
    if (int rc = device_present(who)) return rc;
    if (n == 0) return HUTK_OK;
    const bool vec = seq_len % 4 == 0 && aligned_to(d_values, 16) && aligned_to(d_labels, 16) && aligned_to(d_segment_ids, 16);
    const int64_t per = TB * (vec ? 4 : 1);
    const int64_t blocks = (n + per - 1) / per;
    if (blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, std::string(who) + ": the batch is too large for one launch");
    PackedLabelArgs a;
    a.values = d_values;
    a.seg = d_segment_ids;
    a.labels = d_labels;
    a.n = n;
    a.L = seq_len;
    a.ignore = ignore_index;
    a.shift = shift != 0;
    with_width_vec(width, vec, [&](auto w, auto v) {
        hipLaunchKernelGGL((k_packed_labels<decltype(w)::value, decltype(v)::value>), dim3((unsigned)blocks), dim3(TB), 0,
                           (hipStream_t)hip_stream, a);
    });
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_debug_cu_tile(void) { return CU_TILE; }

int hutk_chat_template_create(hutk_chat_template** out, int device, int n_roles, const int32_t* prefix_ids,
                              const int32_t* prefix_offsets, const int32_t* suffix_ids, const int32_t* suffix_offsets,
                              const int32_t* suffix_loss, int32_t bos_id, int32_t eos_id) {
    const char* who = "hutk_chat_template_create";
    if (!out) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": out is NULL");
    *out = nullptr;
    if (n_roles < 1 || n_roles > HUTK_CHAT_MAX_ROLES || !prefix_offsets || !suffix_offsets)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": n_roles must be in 1 .. 16 and the offsets given");
    ChatTable h = {};
    h.n_roles = n_roles;
    h.bos = bos_id;
    h.eos = eos_id;
    for (int side = 0; side < 2; side++) {
        const int32_t* offs = side ? suffix_offsets : prefix_offsets;
        const int32_t* ids = side ? suffix_ids : prefix_ids;
        if (offs[0] != 0) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": the parts' offsets must be a scan from 0");
        for (int r = 0; r < n_roles; r++) {
            const int64_t len = (int64_t)offs[r + 1] - offs[r];
            if (len < 0 || len > HUTK_CHAT_MAX_PART)
                return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a part holds 0 .. 32 ids, and the offsets must not decrease");
            if (len > 0 && !ids) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a part's ids are NULL");
            (side ? h.slen : h.plen)[r] = (int32_t)len;
            for (int k = 0; k < len; k++) {
                const int32_t id = ids[offs[r] + k];
                if (id == HUTK_NO_TOKEN) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a part must not hold HUTK_NO_TOKEN");
                (side ? h.suffix : h.prefix)[r][k] = id;
            }
        }
    }
    for (int r = 0; r < n_roles; r++) {
        h.sloss[r] = suffix_loss ? suffix_loss[r] : h.slen[r];
        if (h.sloss[r] < 0 || h.sloss[r] > h.slen[r])
            return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": suffix_loss must be in 0 .. the suffix's length");
        if (h.plen[r] + h.slen[r] > h.max_part) h.max_part = h.plen[r] + h.slen[r];
    }
    if (device == -2) {  // the table on the host only, as a context's: the sizes, and the checks of the two device calls
        hutk_chat_template* t = new hutk_chat_template();
        t->device = -2;
        t->h = h;
        *out = t;
        return HUTK_OK;
    }
    int n = 0;
    if (int rc = device_present(who, &n)) return rc;
    if (device < 0) HUTK_HIP_TRY(hipGetDevice(&device));
    if (device >= n) return hutk::api_set_error(HUTK_E_DEVICE, std::string(who) + ": no such device");
    HUTK_HIP_TRY(hipSetDevice(device));
    hutk_chat_template* t = new hutk_chat_template();
    t->device = device;
    t->h = h;
    hipError_t e = hipMalloc((void**)&t->d, sizeof(ChatTable));
    if (e == hipSuccess) e = hipMemcpy(t->d, &t->h, sizeof(ChatTable), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hutk_chat_template_destroy(t);
        return hutk::api_set_error(e == hipErrorOutOfMemory ? HUTK_E_MEMORY : HUTK_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    *out = t;
    return HUTK_OK;
}

void hutk_chat_template_destroy(hutk_chat_template* t) {
    if (!t) return;
    if (t->d) {
        (void)hipSetDevice(t->device);
        (void)hipDeviceSynchronize();  // nothing is freed under a running kernel
        (void)hipFree(t->d);
    }
    delete t;
}

int64_t hutk_chat_ids_bound(const hutk_chat_template* t, int64_t n_conv, int64_t n_turns, int64_t n_ids, int gen_role) {
    int64_t fixed;
    int32_t tail_len;
    if (chat_sizes("hutk_chat_ids_bound", t, n_conv, n_turns, n_ids, gen_role, &fixed, &tail_len)) return -HUTK_E_ARG;
    return n_ids + n_turns * t->h.max_part + n_conv * fixed;
}

int hutk_chat_offsets_device(const hutk_chat_template* t, const int64_t* d_offsets, const int32_t* d_roles,
                             const int64_t* d_conv_offsets, int64_t n_conv, int64_t n_turns, int64_t n_ids, int gen_role,
                             int64_t* d_turn_offsets, int64_t* d_out_offsets, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_chat_offsets_device";
    int64_t fixed;
    int32_t tail_len;
    if (int rc = chat_sizes(who, t, n_conv, n_turns, n_ids, gen_role, &fixed, &tail_len)) return rc;
    if (!d_out_offsets || (n_conv > 0 && (!d_offsets || !d_conv_offsets || !d_turn_offsets || (n_turns > 0 && !d_roles))))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_out_offsets, 8) || !aligned_to(d_offsets, 8) || !aligned_to(d_conv_offsets, 8) || !aligned_to(d_turn_offsets, 8) ||
        !aligned_to(d_roles, 4) || !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its element type");
    if (int rc = device_present(who)) return rc;
    if (!t->d) return hutk::api_set_error(HUTK_E_DEVICE, std::string(who) + ": host-only template: no device to render on");
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(t->device));
    if (n_conv == 0) {
        if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
        HUTK_HIP_TRY(hipMemsetAsync(d_out_offsets, 0, sizeof(int64_t), st));
        if (d_turn_offsets) HUTK_HIP_TRY(hipMemsetAsync(d_turn_offsets, 0, sizeof(int64_t), st));
        return HUTK_OK;
    }
    const ChatTurns turns{t->d, d_offsets, d_roles, n_turns, n_ids};
    if (int rc = rows_scan(turns, n_turns, d_turn_offsets, d_err, st)) return rc;
    const ChatOffArgs a{d_conv_offsets, d_turn_offsets, n_conv, n_turns, fixed, d_out_offsets, d_err};
    hipLaunchKernelGGL(k_chat_offsets, dim3((unsigned)((n_conv + 1 + TB - 1) / TB)), dim3(TB), 0, st, a);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_chat_render_device(const hutk_chat_template* t, const int32_t* d_ids, const int64_t* d_offsets,
                            const int32_t* d_roles, const int64_t* d_conv_offsets, const int64_t* d_turn_offsets,
                            const int64_t* d_out_offsets, int64_t n_conv, int64_t n_turns, int64_t n_ids, int gen_role,
                            uint32_t loss_roles, int32_t ignore_index, int64_t out_cap, int32_t* d_out_ids,
                            int32_t* d_labels, int32_t* d_turn_ids, int64_t* d_src, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_chat_render_device";
    int64_t fixed;
    int32_t tail_len;
    if (int rc = chat_sizes(who, t, n_conv, n_turns, n_ids, gen_role, &fixed, &tail_len)) return rc;
    if (out_cap < 0 || (t->h.n_roles < 32 && (loss_roles >> t->h.n_roles) != 0))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": out_cap must not be negative and loss_roles name roles of the template");
    if (n_conv > 0 && (!d_offsets || !d_conv_offsets || !d_turn_offsets || !d_out_offsets || (n_turns > 0 && !d_roles) ||
                       (n_ids > 0 && !d_ids) || (out_cap > 0 && (!d_out_ids || !d_labels))))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_offsets, 8) || !aligned_to(d_conv_offsets, 8) || !aligned_to(d_turn_offsets, 8) || !aligned_to(d_out_offsets, 8) ||
        !aligned_to(d_src, 8) || !aligned_to(d_ids, 4) || !aligned_to(d_roles, 4) || !aligned_to(d_out_ids, 4) ||
        !aligned_to(d_labels, 4) || !aligned_to(d_turn_ids, 4) || !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its element type");
    if (int rc = device_present(who)) return rc;
    if (!t->d) return hutk::api_set_error(HUTK_E_DEVICE, std::string(who) + ": host-only template: no device to render on");
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(t->device));
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_conv == 0) return HUTK_OK;
    // n_out is on the device only: as many workgroups as the capacity holds spans (one that finds its span behind n_out
    // returns at once), at least the one that reports a capacity of nothing
    int64_t blocks = (out_cap + CHAT_SPAN - 1) / CHAT_SPAN;
    if (blocks < 1) blocks = 1;
    if (blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, std::string(who) + ": the batch is too large for one launch");
    ChatArgs a = {};
    a.tab = t->d;
    a.ids = d_ids;
    a.offs = d_offsets;
    a.roles = d_roles;
    a.conv = d_conv_offsets;
    a.T = d_turn_offsets;
    a.oo = d_out_offsets;
    a.n_conv = n_conv;
    a.n_turns = n_turns;
    a.n_ids = n_ids;
    a.out_cap = out_cap;
    a.gen_role = gen_role;
    a.has_bos = t->h.bos != HUTK_NO_TOKEN;
    a.tail_len = tail_len;
    a.fixed = (int32_t)fixed;
    a.loss_roles = loss_roles;
    a.ignore = ignore_index;
    a.out_ids = d_out_ids;
    a.labels = d_labels;
    a.turn_ids = d_turn_ids;
    a.src = d_src;
    a.err = d_err;
    a.wide = (aligned_to(d_out_ids, 16) ? 1 : 0) | (aligned_to(d_labels, 16) ? 2 : 0) | (aligned_to(d_turn_ids, 16) ? 4 : 0) |
             (aligned_to(d_src, 16) ? 8 : 0);
    hipLaunchKernelGGL(k_chat_render, dim3((unsigned)blocks), dim3(TB), 0, st, a);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_debug_chat_span(void) { return CHAT_SPAN; }

int64_t hutk_fim_ids_bound(int64_t n_docs, int64_t n_ids, int has_end) {
    if (fim_sizes("hutk_fim_ids_bound", n_docs, n_ids, 0, 0, 0)) return -HUTK_E_ARG;
    return n_ids + (3 + (has_end ? 1 : 0)) * n_docs;
}

int hutk_fim_cut_text_device(const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes, uint64_t seed,
                             int64_t first_doc, int64_t fim_below, int64_t spm_below, int64_t* d_piece_offsets,
                             int32_t* d_kinds, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_fim_cut_text_device";
    if (int rc = fim_sizes(who, n_docs, n_bytes, first_doc, fim_below, spm_below)) return rc;
    if (n_docs == 0 && n_bytes != 0) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": bytes without documents");
    if (!d_piece_offsets || (n_docs > 0 && (!d_offsets || !d_kinds || (n_bytes > 0 && !d_bytes))))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_offsets, 8) || !aligned_to(d_piece_offsets, 8) || !aligned_to(d_kinds, 4) || !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its element type");
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_docs == 0) {
        HUTK_HIP_TRY(hipMemsetAsync(d_piece_offsets, 0, sizeof(int64_t), st));
        return HUTK_OK;
    }
    const FimCutArgs a{d_bytes, d_offsets, n_docs, n_bytes, first_doc, seed, (uint64_t)fim_below, (uint64_t)spm_below,
                       d_piece_offsets, d_kinds, d_err};
    hipLaunchKernelGGL(k_fim_cut, dim3((unsigned)((n_docs + TB - 1) / TB)), dim3(TB), 0, st, a);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_fim_plan_tokens_device(const int64_t* d_offsets, int64_t n_docs, int64_t n_ids, uint64_t seed, int64_t first_doc,
                                int64_t fim_below, int64_t spm_below, int has_end, int64_t* d_out_offsets, int64_t* d_plan,
                                int32_t* d_kinds, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_fim_plan_tokens_device";
    if (int rc = fim_sizes(who, n_docs, n_ids, first_doc, fim_below, spm_below)) return rc;
    FimDocs docs = {};
    docs.offs = d_offsets;
    docs.first_doc = first_doc;
    docs.seed = seed;
    docs.fim_below = (uint64_t)fim_below;
    docs.spm_below = (uint64_t)spm_below;
    return fim_plan(who, docs, n_docs, n_ids, has_end, d_out_offsets, d_plan, d_kinds, d_err, (hipStream_t)hip_stream);
}

int hutk_fim_plan_pieces_device(const int64_t* d_piece_id_offsets, const int32_t* d_kinds, int64_t n_docs, int64_t n_ids,
                                int has_end, int64_t* d_out_offsets, int64_t* d_plan, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_fim_plan_pieces_device";
    if (int rc = fim_sizes(who, n_docs, n_ids, 0, 0, 0)) return rc;
    if (n_docs > 0 && !d_kinds) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_kinds, 4)) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its element type");
    FimDocs docs = {};
    docs.offs = d_piece_id_offsets;
    docs.kinds_in = d_kinds;
    return fim_plan(who, docs, n_docs, n_ids, has_end, d_out_offsets, d_plan, nullptr, d_err, (hipStream_t)hip_stream);
}

int hutk_fim_render_device(const int32_t* d_ids, const int64_t* d_plan, const int32_t* d_kinds, const int64_t* d_out_offsets,
                           int64_t n_docs, int64_t n_ids, int32_t pre_id, int32_t suf_id, int32_t mid_id, int32_t end_id,
                           uint32_t loss_parts, int32_t ignore_index, int64_t out_cap, int32_t* d_out_ids, int32_t* d_labels,
                           int32_t* d_parts, int64_t* d_src, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_fim_render_device";
    if (int rc = fim_sizes(who, n_docs, n_ids, 0, 0, 0)) return rc;
    if (pre_id == HUTK_NO_TOKEN || suf_id == HUTK_NO_TOKEN || mid_id == HUTK_NO_TOKEN)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": pre_id, suf_id and mid_id must not be HUTK_NO_TOKEN");
    if (out_cap < 0 || (loss_parts >> 6) != 0)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": out_cap must not be negative and loss_parts name parts 0 .. 4 and HUTK_FIM_LOSS_END");
    if (n_docs > 0 && (!d_plan || !d_kinds || !d_out_offsets || (n_ids > 0 && !d_ids) || (out_cap > 0 && !d_out_ids)))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_plan, 8) || !aligned_to(d_out_offsets, 8) || !aligned_to(d_src, 8) || !aligned_to(d_ids, 4) ||
        !aligned_to(d_kinds, 4) || !aligned_to(d_out_ids, 4) || !aligned_to(d_labels, 4) || !aligned_to(d_parts, 4) ||
        !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its element type");
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_docs == 0) return HUTK_OK;
    // n_out is on the device only: as many workgroups as the capacity holds spans (one that finds its span behind n_out
    // returns at once), at least the one that reports a capacity of nothing
    int64_t blocks = (out_cap + FIM_SPAN - 1) / FIM_SPAN;
    if (blocks < 1) blocks = 1;
    if (blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, std::string(who) + ": the batch is too large for one launch");
    FimArgs a = {};
    a.ids = d_ids;
    a.plan = d_plan;
    a.kinds = d_kinds;
    a.oo = d_out_offsets;
    a.n_docs = n_docs;
    a.n_ids = n_ids;
    a.out_cap = out_cap;
    a.pre = pre_id;
    a.suf = suf_id;
    a.mid = mid_id;
    a.end = end_id;
    a.E = end_id != HUTK_NO_TOKEN;
    a.loss_parts = loss_parts;
    a.ignore = ignore_index;
    a.out_ids = d_out_ids;
    a.labels = d_labels;
    a.parts = d_parts;
    a.src = d_src;
    a.err = d_err;
    a.wide = (aligned_to(d_out_ids, 16) ? 1 : 0) | (aligned_to(d_labels, 16) ? 2 : 0) | (aligned_to(d_parts, 16) ? 4 : 0) |
             (aligned_to(d_src, 16) ? 8 : 0);
    hipLaunchKernelGGL(k_fim_render, dim3((unsigned)blocks), dim3(TB), 0, st, a);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

int hutk_debug_fim_span(void) { return FIM_SPAN; }

int hutk_debug_fim_decide(uint64_t seed, int64_t doc, int64_t len, int64_t fim_below, int64_t spm_below, int64_t out3[3]) {
    constexpr int64_t ONE = (int64_t)1 << 32;
    if (!out3 || fim_below < 0 || fim_below > ONE || spm_below < 0 || spm_below > ONE)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_debug_fim_decide: out3 is NULL or a threshold lies outside 0 .. 2^32");
    const hutk::FimCut c = hutk::fim_decide(seed, doc, len, (uint64_t)fim_below, (uint64_t)spm_below);
    out3[0] = c.kind, out3[1] = c.lo, out3[2] = c.hi;
    return HUTK_OK;
}

int hutk_debug_fim_locate(int64_t n, int64_t lo, int64_t hi, int kind, int has_end, int64_t p, int64_t out2[2]) {
    if (!out2 || kind < hutk::FIM_PLAIN || kind > hutk::FIM_SPM || lo < 0 || lo > hi || hi > n)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_debug_fim_locate: out2 is NULL, a kind outside 0 .. 2 or cuts that are not 0 <= lo <= hi <= n");
    const hutk::FimPlace at = hutk::fim_locate(n, lo, hi, kind, has_end ? 1 : 0, p);
    out2[0] = at.part, out2[1] = at.v;
    return HUTK_OK;
}

}  // extern "C"
