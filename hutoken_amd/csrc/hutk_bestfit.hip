// hutk_bestfit.hip -- best-fit packing: rows of whole documents (the rule: include/hutoken_amd.h,
// "BEST FIT").  Ding et al. 2024, "Fewer Truncations Improve Language Modeling": cut only what is longer than a row, pack
// the tails best-fit-decreasing.  Three entry points that enqueue and return; the one wait there can be is for the device
// when the shared scratch buffer has to grow (scratch_for), which the plan call takes on for the rows call behind it:
//
// The PLAN (hutk_bestfit_plan_device), documents -> doc_map and info:
//   k_bf_count   a wavefront owns a contiguous run of documents and counts its items per length class, counts[wave][l],
//                and sums its whole rows
//   k_bf_cols    per class the exclusive scan of the counts over the wavefronts, and the class totals (the histogram);
//                launch_scan_i64 over the whole-row sums
//   k_bf_walk    ONE wavefront walks the classes from the longest down.  Best fit is not sequential in the items: bins that
//                opened together and absorbed the same items stay identical, so the state is a list of GROUPS (first bin,
//                bins, room, items so far) over contiguous bin numbers, kept in one list per room value, each sorted by
//                first bin, under a three-level bitmap of the rooms in use.  A class visits the groups of room >= l in the
//                order (room, first bin); every bin of a visited group takes room / l items in a row; the class's items
//                fill the bins from the lowest number up in document order.  Every visit is recorded:
//                (first rank, first bin, items per bin, room, items so far).  The classes above L / 2 open a bin per item
//                and are done 64 at a time; the others are serial, on lane 0.
//   k_bf_place   the wavefronts of k_bf_count again: the rank of every item inside its class in document order -- the
//                counts of the wavefronts in front (k_bf_cols), plus the equal lengths in front of it inside the wavefront's
//                run -- then a search among the class's visits gives bin, column and with them the doc_map row.
// The ranks are a stable counting rank.  The one atomic whose return is used (the cursor of a class inside a wavefront's
// own row of counts) is only ever issued by that wavefront, in program order, so its returns are an order of the
// program and not of the hardware.
//
// The ROWS (hutk_bestfit_rows_device), doc_map + ids -> the five row arrays.  The writer is driven by the OUTPUT element:
// a thread owns four consecutive columns (one on the element path) and writes them once, so nothing in a hostile doc_map
// can move a write.  What it needs is the inverse of doc_map, which the call builds itself:
//   k_br_wsum / launch_scan_i64 / k_br_docs   the whole rows in front of every document, from the offsets alone (a
//                whole row finds its document by a search in that scan, never through doc_map); every doc_map row is checked
//                against the offsets and the row count, and a good item sets the bit (row, col) of a start bitmap
//   k_br_rowscan / launch_scan_i64            per bin row the set bits in front of every 32-bit word, and the items in
//                front of every row
//   k_br_items   item j of row r -> its document, at item_doc[items before r + j] (j from the bitmap: no atomics)
//   k_br_write   segment = the start bits at or in front of the column, document = item_doc[..], the rest from the
//                document's doc_map row and offsets, all range-checked again.
//
// The GATHER (hutk_rows_gather_source_device): out[e] = source[e] >= 0 ? values[source[e]] : fill, one elementwise pass.
#include <map>
#include <mutex>
#include <string>
#include <type_traits>

#include "hutk_host.h"
#include "hutk_wave.h"

namespace {

constexpr int TB = 256;
constexpr int BF_TILE = TB;                   // documents a workgroup of the document passes owns at least: 4 wavefronts x 64
constexpr int64_t BF_MAX_L = 65536;           // the classes are ranked by 16 ballots and their rooms sit in a 3-level bitmap
constexpr int64_t BF_COUNT_CELLS = 1 << 21;   // counts[wavefronts][L]: at most this many cells (8 MiB)
constexpr int BF_LDS_HEADS = 8192;            // up to this L the list heads of k_bf_walk are in LDS
constexpr int64_t BR_MAX_WAVES = 4096;        // wavefronts of the rows call's document passes (k_br_wsum, k_br_docs) ...
constexpr int64_t BR_MIN_PER_WAVE = 128;      // ... and the documents each owns at least: two chunks, so that every batch of more than 64 documents carries from chunk to chunk
constexpr int VISIT_WORDS = 6;                // first rank, first bin, items per bin, room, items so far, (unused)

__device__ __forceinline__ void note_error(int32_t* err, int code) {
    if (err) atomicCAS(err, 0, code);
}

// What the document passes read of document i: whole rows w and item length l of its sequence.  Offsets that do not
// describe the ids give an empty document and ok = false; nothing is derived from them.
struct DocLens {
    int64_t off, n, w;
    int32_t l;
    bool ok;
};
__device__ __forceinline__ DocLens doc_lens(const int64_t* offs, int64_t i, int64_t n_ids, int32_t L, int32_t s) {
    DocLens d;
    const int64_t a = offs[i], b = offs[i + 1];
    d.ok = a >= 0 && a <= b && b <= n_ids;
    d.off = d.ok ? a : 0;
    d.n = d.ok ? b - a : 0;
    const int64_t m = d.ok ? d.n + s : 0;
    d.w = m / L;
    d.l = (int32_t)(m % L);
    return d;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------
struct PlanArgs {
    const int64_t* offs;
    int64_t n_docs, n_ids;
    int32_t L, s;
    int64_t per_wave;     // documents a wavefront owns: a multiple of 64
    int32_t n_waves;
    uint32_t* counts;     // [n_waves][L]: items of class l in the wavefront's run; after k_bf_cols those of the runs in front
    int64_t* wsum;        // [n_waves + 1]: whole rows of the run; after the scan those in front, and W
    uint32_t* hist;       // [L]
    int32_t* cls_vfirst;  // [L] the class's visits are visits[cls_vfirst[l] .. + cls_vcount[l])
    int32_t* cls_vcount;  // [L]
    int32_t* visits;      // [v_cap][VISIT_WORDS]
    int64_t v_cap;
    int4* nodes;          // [ng_cap] a group: first bin, bins, room, items so far
    int32_t* next;        // [ng_cap] the next group of the same room, by first bin; -1: none
    int32_t* heads;       // [L] the first group of every room (L > BF_LDS_HEADS; smaller ones: LDS)
    int64_t ng_cap;
    int64_t* doc_map;     // [n_docs][4]
    int64_t* info;        // [2]
    int64_t rows_cap;
    int32_t* err;
};

__global__ __launch_bounds__(TB) void k_bf_count(const PlanArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (g >= a.n_waves) return;
    if (g == 0 && lane == 0 && (a.offs[0] != 0 || a.offs[a.n_docs] != a.n_ids)) note_error(a.err, HUTK_E_ARG);
    const int64_t d0 = g * a.per_wave, d1 = d0 + a.per_wave < a.n_docs ? d0 + a.per_wave : a.n_docs;
    uint32_t* mine = a.counts + g * a.L;
    int64_t rows = 0;
    for (int64_t i = d0 + lane; i < d1; i += 64) {
        const DocLens d = doc_lens(a.offs, i, a.n_ids, a.L, a.s);
        if (!d.ok) note_error(a.err, HUTK_E_ARG);
        if (d.l > 0) atomicAdd(&mine[d.l], 1u);
        rows += d.w;
    }
    rows = hutk::wave_incl(rows, lane);
    if (lane == 63) a.wsum[g] = rows;
}

__global__ __launch_bounds__(TB) void k_bf_cols(const PlanArgs a) {
    const int64_t l = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (l >= a.L) return;
    uint32_t run = 0;
#pragma unroll 8
    for (int64_t g = 0; g < a.n_waves; g++) {
        const uint32_t c = a.counts[g * a.L + l];
        a.counts[g * a.L + l] = run;
        run += c;
    }
    a.hist[l] = run;
}

// The rooms in use: bit r of b0, a bit per word of b0 in b1, a bit per word of b1 in b2.
struct RoomBits {
    uint64_t* b0;  // [1024]
    uint64_t* b1;  // [16]
    uint64_t* b2;  // [1]
    __device__ __forceinline__ void set(int32_t r) {
        const int w = r >> 6;
        b0[w] |= 1ull << (r & 63);
        b1[w >> 6] |= 1ull << (w & 63);
        b2[0] |= 1ull << (w >> 6);
    }
    __device__ __forceinline__ void clear(int32_t r) {
        const int w = r >> 6;
        if ((b0[w] &= ~(1ull << (r & 63))) != 0) return;
        if ((b1[w >> 6] &= ~(1ull << (w & 63))) != 0) return;
        b2[0] &= ~(1ull << (w >> 6));
    }
    // the smallest room in use that is at least r, -1: none
    __device__ __forceinline__ int32_t next_from(int32_t r) const {
        int w = r >> 6;
        uint64_t m = b0[w] & (~0ull << (r & 63));
        if (m) return w * 64 + __builtin_ctzll(m);
        int w1 = w >> 6;
        m = (w & 63) == 63 ? 0 : b1[w1] & (~0ull << ((w & 63) + 1));
        if (!m) {
            m = b2[0] & (~0ull << (w1 + 1));  // (w1 <= 15)
            if (!m) return -1;
            w1 = __builtin_ctzll(m);
            m = b1[w1];
        }
        w = w1 * 64 + __builtin_ctzll(m);
        return w * 64 + __builtin_ctzll(b0[w]);
    }
};

struct Walk {
    const PlanArgs& a;
    int32_t* head;
    RoomBits bits;
    int64_t bins = 0, v = 0, ng = 0;
    bool full = false;  // a bound of the scratch was reached: cannot happen (hutk_bestfit_plan_device derives them), checked all the same

    __device__ __forceinline__ void visit(int64_t rank, int64_t bin, int32_t per_bin, int32_t room, int32_t items) {
        if (v >= a.v_cap) {
            full = true;
            return;
        }
        int32_t* p = a.visits + v * VISIT_WORDS;
        p[0] = (int32_t)rank, p[1] = (int32_t)bin, p[2] = per_bin, p[3] = room, p[4] = items;
        v++;
    }
    // group idx, already written to nodes, into the list of its room: behind the groups of lower first bin
    __device__ __forceinline__ void insert(int32_t idx, int32_t room, int32_t first) {
        int32_t p = head[room];
        if (p < 0 || a.nodes[p].x > first) {
            a.next[idx] = p;
            head[room] = idx;
            if (p < 0) bits.set(room);
            return;
        }
        int32_t q;
        while ((q = a.next[p]) >= 0 && a.nodes[q].x < first) p = q;
        a.next[idx] = q;
        a.next[p] = idx;
    }
    __device__ __forceinline__ void add(int64_t first, int64_t n, int32_t room, int32_t items) {
        if (n <= 0 || room <= 0) return;  // (a full bin takes nothing more)
        if (ng >= a.ng_cap) {
            full = true;
            return;
        }
        const int32_t idx = (int32_t)ng++;
        a.nodes[idx] = make_int4((int32_t)first, (int32_t)n, room, items);
        insert(idx, room, (int32_t)first);
    }
    __device__ __forceinline__ void unlink_head(int32_t room, int32_t idx) {
        const int32_t nx = a.next[idx];
        head[room] = nx;
        if (nx < 0) bits.clear(room);
    }
    // the c items of class l (l <= L / 2), ranks 0 .. c - 1
    __device__ void take(int32_t l, int64_t c) {
        const int64_t v0 = v;
        int64_t rem = c, rank = 0;
        while (rem > 0 && !full) {
            const int32_t room = bits.next_from(l);
            if (room < 0) break;
            const int32_t idx = head[room];
            const int4 gq = a.nodes[idx];  // first bin, bins, room, items so far
            const int32_t k = room / l;
            const int64_t cap = (int64_t)gq.y * k;
            visit(rank, gq.x, k, room, gq.w);
            if (cap <= rem) {  // every bin of the group takes k
                unlink_head(room, idx);
                rem -= cap, rank += cap;
                const int32_t left = room - k * l;
                if (left > 0) {
                    a.nodes[idx] = make_int4(gq.x, gq.y, left, gq.w + k);
                    insert(idx, left, gq.x);
                }
            } else {  // the items run out here: full bins, one partly filled bin, untouched bins
                const int32_t n_full = (int32_t)(rem / k), t = (int32_t)(rem % k), part = t > 0;
                const int32_t n_un = gq.y - n_full - part;
                if (n_un > 0) a.nodes[idx] = make_int4(gq.x + n_full + part, n_un, room, gq.w);  // (still the first of its list)
                else unlink_head(room, idx);
                add(gq.x, n_full, room - k * l, gq.w + k);
                add(gq.x + n_full, part, room - t * l, gq.w + t);
                rank += rem, rem = 0;
            }
        }
        if (rem > 0 && !full) {  // new bins
            const int32_t k = a.L / l;
            visit(rank, bins, k, a.L, 0);
            const int64_t n_full = rem / k;
            const int32_t t = (int32_t)(rem % k), part = t > 0;
            add(bins, n_full, a.L - k * l, k);
            add(bins + n_full, part, a.L - t * l, t);
            bins += n_full + part;
        }
        a.cls_vfirst[l] = (int32_t)v0;
        a.cls_vcount[l] = (int32_t)(v - v0);
    }
};

__global__ __launch_bounds__(64) void k_bf_walk(const PlanArgs a) {
    __shared__ uint64_t s_b0[1024], s_b1[16], s_b2[1];
    __shared__ int32_t s_head[BF_LDS_HEADS];
    const int lane = threadIdx.x;
    const int32_t L = a.L;
    int32_t* head = L <= BF_LDS_HEADS ? s_head : a.heads;
    for (int i = lane; i < 1024; i += 64) s_b0[i] = 0;
    if (lane < 16) s_b1[lane] = 0;
    if (lane == 0) s_b2[0] = 0;
    for (int i = lane; i < L; i += 64) head[i] = -1;
    __threadfence();
    __syncthreads();
    Walk w{a, head, RoomBits{s_b0, s_b1, s_b2}};
    // classes above L / 2: every item opens a bin, nothing open can take one (the open rooms are below L / 2)
    for (int32_t top = L - 1; 2 * top > L; top -= 64) {
        const int32_t l = top - lane;
        const bool in = 2 * l > L;
        const int64_t c = in ? a.hist[l] : 0;
        const int64_t incl = hutk::wave_incl(c, lane);
        const uint64_t some = __ballot(c > 0);
        const int64_t slot = __popcll(some & ((1ull << lane) - 1));
        if (in && c == 0) a.cls_vcount[l] = 0;
        if (c > 0) {
            const int64_t v = w.v + slot, idx = w.ng + slot, first = w.bins + incl - c;
            if (v < a.v_cap && idx < a.ng_cap) {
                int32_t* p = a.visits + v * VISIT_WORDS;
                p[0] = 0, p[1] = (int32_t)first, p[2] = 1, p[3] = L, p[4] = 0;
                a.cls_vfirst[l] = (int32_t)v;
                a.cls_vcount[l] = 1;
                a.nodes[idx] = make_int4((int32_t)first, (int32_t)c, L - l, 1);  // (one group per room here)
                a.next[idx] = -1;
                head[L - l] = (int32_t)idx;
                const int r = L - l, wd = r >> 6;
                atomicOr((unsigned long long*)&s_b0[wd], 1ull << (r & 63));
                atomicOr((unsigned long long*)&s_b1[wd >> 6], 1ull << (wd & 63));
                atomicOr((unsigned long long*)&s_b2[0], 1ull << (wd >> 6));
            } else {
                a.cls_vcount[l] = 0;
                w.full = true;
            }
        }
        w.full = __any(w.full);
        w.bins += __shfl(incl, 63);
        w.v += __popcll(some);
        w.ng += __popcll(some);
    }
    __threadfence();
    __syncthreads();
    // the others, from the longest down: lane 0 walks, the wavefront reads the histogram 64 classes at a time
    for (int32_t top = L / 2; top >= 1; top -= 64) {
        const int32_t l_mine = top - lane;
        const int64_t c_mine = l_mine >= 1 ? a.hist[l_mine] : 0;
        if (l_mine >= 1 && c_mine == 0) a.cls_vcount[l_mine] = 0;
        uint64_t some = __ballot(c_mine > 0);
        while (some) {
            const int j = __builtin_ctzll(some);
            some &= some - 1;
            const int64_t c = __shfl(c_mine, j);
            if (lane == 0) w.take(top - j, c);
        }
    }
    if (lane == 0) {
        const int64_t W = a.wsum[a.n_waves];
        a.info[0] = W + w.bins;
        a.info[1] = W;
        if (w.full) note_error(a.err, HUTK_E_UNSUPPORTED);
        else if (W + w.bins > a.rows_cap) note_error(a.err, HUTK_E_CAPACITY);
    }
}

__global__ __launch_bounds__(TB) void k_bf_place(const PlanArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (g >= a.n_waves) return;
    const int64_t d0 = g * a.per_wave, d1 = d0 + a.per_wave < a.n_docs ? d0 + a.per_wave : a.n_docs;
    uint32_t* cursor = a.counts + g * a.L;  // per class: the items in front of this wavefront's next one
    const int64_t W = a.wsum[a.n_waves];
    int64_t rows_before = a.wsum[g];
    const uint64_t below = (1ull << lane) - 1;
    for (int64_t at = d0; at < d1; at += 64) {  // (every lane takes every trip: the ballots are the wavefront's)
        const int64_t i = at + lane;
        DocLens d{0, 0, 0, 0, true};
        if (i < d1) d = doc_lens(a.offs, i, a.n_ids, a.L, a.s);
        const int64_t incl = hutk::wave_incl(d.w, lane);
        // the lanes that hold an item of this lane's length
        uint64_t same = __ballot(d.l > 0);
        for (int32_t bit = 1; bit < a.L; bit <<= 1) {
            const uint64_t b = __ballot((d.l & bit) != 0);
            same &= (d.l & bit) ? b : ~b;
        }
        const int leader = d.l > 0 ? __builtin_ctzll(same) : lane;
        uint32_t base = 0;
        if (d.l > 0 && lane == leader) base = atomicAdd(&cursor[d.l], (uint32_t)__popcll(same));
        base = __shfl(base, leader);
        if (i < d1) {
            int64_t row = -1, col = -1;
            if (d.l > 0) {
                const int64_t rank = (int64_t)base + __popcll(same & below);
                const int32_t* vs = a.visits + (int64_t)a.cls_vfirst[d.l] * VISIT_WORDS;
                int32_t lo = 0, hi = a.cls_vcount[d.l];  // the last visit whose first rank is at or below rank
                while (hi - lo > 1) {
                    const int32_t mid = (lo + hi) >> 1;
                    if (vs[(int64_t)mid * VISIT_WORDS] <= rank) lo = mid;
                    else hi = mid;
                }
                if (hi > 0) {  // (hi == 0: the walk gave up, its error word is set)
                    const int32_t* p = vs + (int64_t)lo * VISIT_WORDS;
                    const int64_t j = rank - p[0];
                    row = W + p[1] + j / p[2];
                    col = a.L - p[3] + (j % p[2]) * d.l;
                }
            }
            int64_t* m = a.doc_map + i * 4;
            m[0] = d.w > 0 ? rows_before + incl - d.w : -1;
            m[1] = d.w;
            m[2] = row;
            m[3] = col;
        }
        rows_before += __shfl(incl, 63);
    }
}

// ---- the rows -----------------------------------------------------------------------------------------------------------
struct RowsArgs {
    const int32_t* ids;
    const int64_t* offs;
    const int64_t* doc_map;
    int64_t n_docs, n_ids, R, n;  // n = R * L elements
    int32_t L, s, words;          // words: 32-bit words of the start bitmap per row
    int32_t bos, eos, pad;
    int64_t per_wave;
    int32_t n_waves;
    int64_t* wsum;      // [n_waves + 1]
    int64_t* ws;        // [n_docs + 1] whole rows in front of every document; ws[n_docs] = W
    uint32_t* bits;     // [R][words] bit c of row r - W: an item starts at column c
    uint32_t* before;   // [R][words] set bits of the row in front of the word
    int64_t* row_base;  // [R + 1] items in the rows in front
    int32_t* item_doc;  // [n_docs]
    void* out;
    int32_t *pos, *seg, *lengths;
    int64_t* source;
    int32_t* err;
};

__global__ __launch_bounds__(TB) void k_br_wsum(const RowsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (g >= a.n_waves) return;
    if (g == 0 && lane == 0 && (a.offs[0] != 0 || a.offs[a.n_docs] != a.n_ids)) note_error(a.err, HUTK_E_ARG);
    const int64_t d0 = g * a.per_wave, d1 = d0 + a.per_wave < a.n_docs ? d0 + a.per_wave : a.n_docs;
    int64_t rows = 0;
    for (int64_t i = d0 + lane; i < d1; i += 64) rows += doc_lens(a.offs, i, a.n_ids, a.L, a.s).w;
    rows = hutk::wave_incl(rows, lane);
    if (lane == 63) a.wsum[g] = rows;
}

// Is the item of document i where its doc_map row says a row of these outputs?  W: the whole rows of the batch.
__device__ __forceinline__ bool item_ok(const RowsArgs& a, const DocLens& d, int64_t row, int64_t col, int64_t W) {
    return d.ok && d.l > 0 && row >= W && row < a.R && col >= 0 && col <= a.L - d.l;
}

__global__ __launch_bounds__(TB) void k_br_docs(const RowsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (g >= a.n_waves) return;
    const int64_t d0 = g * a.per_wave, d1 = d0 + a.per_wave < a.n_docs ? d0 + a.per_wave : a.n_docs;
    const int64_t W = a.wsum[a.n_waves];
    int64_t rows_before = a.wsum[g];
    if (g == 0 && lane == 0) a.ws[a.n_docs] = W;
    for (int64_t at = d0; at < d1; at += 64) {
        const int64_t i = at + lane;
        DocLens d{0, 0, 0, 0, true};
        if (i < d1) d = doc_lens(a.offs, i, a.n_ids, a.L, a.s);
        const int64_t incl = hutk::wave_incl(d.w, lane);
        if (i < d1) {
            const int64_t first = rows_before + incl - d.w;
            a.ws[i] = first;
            const int64_t* m = a.doc_map + i * 4;
            const int64_t row = m[2], col = m[3];
            bool good = d.ok && m[1] == d.w && m[0] == (d.w > 0 ? first : -1) && first + d.w <= a.R;
            if (d.l == 0) good = good && row == -1 && col == -1;
            else if (item_ok(a, d, row, col, W)) {
                const uint32_t bit = 1u << (col & 31);
                const uint32_t old = atomicOr(&a.bits[(row - W) * a.words + (col >> 5)], bit);
                good = good && !(old & bit);  // (two items at one place)
            } else good = false;
            if (!good) note_error(a.err, HUTK_E_ARG);
        }
        rows_before += __shfl(incl, 63);
    }
}

// one wavefront per row
__global__ __launch_bounds__(TB) void k_br_rowscan(const RowsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (r >= a.R) return;
    uint32_t run = 0;
    for (int32_t w0 = 0; w0 < a.words; w0 += 64) {
        const int32_t w = w0 + lane;
        const uint32_t c = w < a.words ? __popc(a.bits[r * a.words + w]) : 0;
        const uint32_t incl = hutk::wave_incl(c, lane);
        if (w < a.words) a.before[r * a.words + w] = run + incl - c;
        run += __shfl(incl, 63);
    }
    if (lane == 0) a.row_base[r] = run;
}

__global__ __launch_bounds__(TB) void k_br_items(const RowsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= a.n_docs) return;
    const DocLens d = doc_lens(a.offs, i, a.n_ids, a.L, a.s);
    const int64_t row = a.doc_map[i * 4 + 2], col = a.doc_map[i * 4 + 3], W = a.ws[a.n_docs];
    if (!item_ok(a, d, row, col, W)) return;
    const int64_t at = (row - W) * a.words + (col >> 5);
    const int64_t j = a.before[at] + __popc(a.bits[at] & ((1u << (col & 31)) - 1u));
    const int64_t slot = a.row_base[row - W] + j;
    if (slot < a.n_docs) a.item_doc[slot] = (int32_t)i;  // (as many slots as good items: always)
}

template <int W>
using elem_t = std::conditional_t<W == 4, int32_t, int64_t>;

template <int W, bool VEC>
__device__ __forceinline__ void put(void* base, int64_t i, const elem_t<W>* v) {
    elem_t<W>* p = static_cast<elem_t<W>*>(base) + i;
    if constexpr (!VEC) p[0] = v[0];
    else if constexpr (W == 4) *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
    else {
        reinterpret_cast<longlong2*>(p)[0] = make_longlong2(v[0], v[1]);
        reinterpret_cast<longlong2*>(p)[1] = make_longlong2(v[2], v[3]);
    }
}

// Token t of the sequence of a document: its id and its index into the ids (-1: bos, eos).
__device__ __forceinline__ int32_t seq_token(const RowsArgs& a, const DocLens& d, int64_t t, int64_t& src) {
    const int has_bos = a.bos != HUTK_NO_TOKEN;
    src = -1;
    if (has_bos && t == 0) return a.bos;
    const int64_t k = t - has_bos;
    if (k >= d.n) return a.eos;  // (t < n + s: the caller's check)
    src = d.off + k;
    return a.ids[src];
}

template <int W, bool VEC, bool SRC>
__global__ __launch_bounds__(TB) void k_br_write(const RowsArgs a) {
    constexpr int V = VEC ? 4 : 1;
    using T = elem_t<W>;
    const int64_t at = ((int64_t)blockIdx.x * TB + threadIdx.x) * V;
    const bool live = at < a.n;
    if (!__any(live)) return;
    const int64_t r = live ? at / a.L : -1;
    const int32_t c0 = live ? (int32_t)(at % a.L) : 0;  // (VEC: L % 4 == 0, the V elements share a row)
    const int64_t Wr = a.ws[a.n_docs];
    T id[V];
    int32_t pos[V], seg[V];
    int64_t src[V];
#pragma unroll
    for (int e = 0; e < V; e++) id[e] = a.pad, pos[e] = 0, seg[e] = 0, src[e] = -1;
    int32_t len = 0;
    // a whole row finds its document in the scan of whole rows: the last document whose rows begin at or before r.  A
    // wavefront inside one row searches once, together.
    const int64_t r0 = __shfl(r, 0);
    int64_t doc = -1;
    if (__all(!live || r == r0) && r0 >= 0 && r0 < Wr) {
        doc = hutk::wave_count_leading(a.n_docs, [&](int64_t j) { return a.ws[j] <= r0; }) - 1;
    } else if (live && r < Wr) {
        int64_t lo = 0, hi = a.n_docs;  // ws[lo] <= r (ws[0] = 0), ws[hi] > r
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.ws[mid] <= r) lo = mid;
            else hi = mid;
        }
        doc = lo;
    }
    if (!live) return;
    if (r < Wr) {
        const DocLens d = doc_lens(a.offs, doc, a.n_ids, a.L, a.s);
        const int64_t t0 = (r - a.ws[doc]) * a.L + c0;
        len = a.L;
#pragma unroll
        for (int e = 0; e < V; e++) {
            if (t0 + e < d.n + a.s) id[e] = seq_token(a, d, t0 + e, src[e]);  // (always: the row is one of the document's)
            pos[e] = c0 + e, seg[e] = 1;
        }
    } else {
        const int64_t rb = r - Wr, wi = rb * a.words + (c0 >> 5);
        const uint32_t bits = a.bits[wi], bef = a.before[wi];
        int32_t j_at = -1, col = 0;
        DocLens d{0, 0, 0, 0, false};
#pragma unroll
        for (int e = 0; e < V; e++) {
            const int32_t c = c0 + e;
            const int32_t cnt = (int32_t)(bef + __popc(bits & ((2u << (c & 31)) - 1u)));  // starts at or in front of c
            if (cnt == 0) continue;
            if (cnt - 1 != j_at) {
                j_at = cnt - 1;
                d.ok = false;
                const int64_t slot = a.row_base[rb] + j_at;
                const int64_t i = slot < a.n_docs ? a.item_doc[slot] : -1;
                if (i >= 0 && i < a.n_docs) {
                    d = doc_lens(a.offs, i, a.n_ids, a.L, a.s);
                    const int64_t mr = a.doc_map[i * 4 + 2], mc = a.doc_map[i * 4 + 3];
                    d.ok = item_ok(a, d, mr, mc, Wr) && mr == r && mc <= c;
                    col = (int32_t)mc;
                }
            }
            if (!d.ok) continue;
            const int32_t q = c - col;
            len = col + d.l;
            if (q >= d.l) continue;  // behind the row's last item
            id[e] = seq_token(a, d, d.w * a.L + q, src[e]);
            pos[e] = q, seg[e] = cnt;
        }
    }
    put<W, VEC>(a.out, at, id);
    put<4, VEC>(a.pos, at, pos);
    put<4, VEC>(a.seg, at, seg);
    if constexpr (SRC) put<8, VEC>(a.source, at, src);
    if (c0 + V == a.L) a.lengths[r] = len;
}

// ---- the gather by source --------------------------------------------------------------------------------------------
struct GatherArgs {
    const int64_t* source;
    int64_t n, n_values;
    const void* values;
    void* out;
    int64_t fill;
    int32_t* err;
};

template <int RB>
struct rec_of;
template <>
struct rec_of<4> { using type = uint32_t; };
template <>
struct rec_of<8> { using type = uint2; };
template <>
struct rec_of<16> { using type = uint4; };

// the fill as a record: `width` bytes of it, `per` times
template <int RB>
__device__ __forceinline__ typename rec_of<RB>::type fill_record(int64_t fill, int width) {
    const uint32_t lo = (uint32_t)(uint64_t)fill, hi = (uint32_t)((uint64_t)fill >> 32);
    if constexpr (RB == 4) return lo;
    else if constexpr (RB == 8) return width == 4 ? make_uint2(lo, lo) : make_uint2(lo, hi);
    else return make_uint4(lo, hi, lo, hi);
}

template <int RB, bool VEC>
__global__ __launch_bounds__(TB) void k_gather_source(const GatherArgs a, int width) {
    constexpr int V = VEC ? 4 : 1;
    using R = typename rec_of<RB>::type;
    const int64_t at = ((int64_t)blockIdx.x * TB + threadIdx.x) * V;
    if (at >= a.n) return;
    const R fill = fill_record<RB>(a.fill, width);
    const R* values = static_cast<const R*>(a.values);
    R* out = static_cast<R*>(a.out);
    if (VEC && at + V <= a.n) {
        const longlong2 x = *reinterpret_cast<const longlong2*>(a.source + at), y = *reinterpret_cast<const longlong2*>(a.source + at + 2);
        // (no arrays of records: four named values stay in registers)
        const int64_t n_values = a.n_values;
        int32_t* const err = a.err;
        const auto get = [=](int64_t s) -> R {
            if (s >= n_values) note_error(err, HUTK_E_ARG);
            const bool in = s >= 0 && s < n_values;
            if constexpr (RB == 4) {
                uint32_t x = fill;
                if (in) x = values[s];
                return x;
            } else if constexpr (RB == 8) {
                uint32_t x = fill.x, y = fill.y;
                if (in) {
                    const uint2 t = values[s];
                    x = t.x, y = t.y;
                }
                return make_uint2(x, y);
            } else {
                uint32_t x = fill.x, y = fill.y, z = fill.z, w = fill.w;
                if (in) {
                    const uint4 t = values[s];
                    x = t.x, y = t.y, z = t.z, w = t.w;
                }
                return make_uint4(x, y, z, w);
            }
        };
        const R v0 = get(x.x), v1 = get(x.y), v2 = get(y.x), v3 = get(y.y);
        if constexpr (RB == 4) *reinterpret_cast<uint4*>(out + at) = make_uint4(v0, v1, v2, v3);
        else if constexpr (RB == 8) {
            reinterpret_cast<uint4*>(out + at)[0] = make_uint4(v0.x, v0.y, v1.x, v1.y);
            reinterpret_cast<uint4*>(out + at)[1] = make_uint4(v2.x, v2.y, v3.x, v3.y);
        } else {
            out[at] = v0, out[at + 1] = v1, out[at + 2] = v2, out[at + 3] = v3;
        }
        return;
    }
    for (int64_t k = at; k < at + V && k < a.n; k++) {
        const int64_t s = a.source[k];
        if (s >= a.n_values) note_error(a.err, HUTK_E_ARG);
        if constexpr (RB == 16) {  // (records of two 8-byte elements are 8-byte aligned on this path)
            const uint2* v2 = static_cast<const uint2*>(a.values);
            uint2* o2 = static_cast<uint2*>(a.out);
            const bool in = s >= 0 && s < a.n_values;
            o2[2 * k] = in ? v2[2 * s] : make_uint2(fill.x, fill.y);
            o2[2 * k + 1] = in ? v2[2 * s + 1] : make_uint2(fill.z, fill.w);
        } else if constexpr (RB == 8) {  // (two 4-byte elements are 4-byte aligned)
            const uint32_t* v1 = static_cast<const uint32_t*>(a.values);
            uint32_t* o1 = static_cast<uint32_t*>(a.out);
            const bool in = s >= 0 && s < a.n_values;
            o1[2 * k] = in ? v1[2 * s] : fill.x;
            o1[2 * k + 1] = in ? v1[2 * s + 1] : fill.y;
        } else {
            out[k] = s >= 0 && s < a.n_values ? values[s] : fill;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

int device_present(const char* who) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return hutk::api_set_error(HUTK_E_DEVICE, std::string(who) + ": no HIP device");
    return HUTK_OK;
}

// The scratch of the plan and of the rows: one buffer per device that grows to the largest call so far, carved up by the
// call.  Calls that share it are serialised like calls on one packer: a mutex on the host, an event on the device.
struct BfScratch {
    DevBuf<uint8_t> buf;
    hipEvent_t ev = nullptr;
    bool ev_recorded = false;
};
std::mutex g_bf_mu;
std::map<int, BfScratch> g_bf_scratch;

// the caller holds g_bf_mu until scratch_used
int scratch_for(hipStream_t st, size_t bytes, BfScratch** out) {
    int device = 0;
    HUTK_HIP_TRY(hipGetDevice(&device));
    BfScratch& w = g_bf_scratch[device];
    if (!w.ev) HUTK_HIP_TRY(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
    HUTK_HIP_TRY(w.buf.reserve(bytes));  // (growing waits for the device: an earlier call may still use the old one)
    if (w.ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, w.ev, 0));
    *out = &w;
    return HUTK_OK;
}

int scratch_used(BfScratch* w, hipStream_t st) {
    HUTK_HIP_TRY(hipGetLastError());
    HUTK_HIP_TRY(hipEventRecord(w->ev, st));
    w->ev_recorded = true;
    return HUTK_OK;
}

// carves arrays of 16-byte aligned starts out of one buffer; with base == nullptr it only adds up
struct Carver {
    uint8_t* base;
    size_t at = 0;
    template <class T>
    T* take(size_t n) {
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += (n * sizeof(T) + 15) & ~(size_t)15;
        return p;
    }
};

// what the best-fit calls refuse before anything else; s comes back
int bestfit_sizes(const char* who, int64_t n_docs, int64_t n_ids, int64_t seq_len, int32_t bos_id, int32_t eos_id, int64_t rows_cap,
                  int* s) {
    *s = (bos_id != HUTK_NO_TOKEN) + (eos_id != HUTK_NO_TOKEN);
    if (seq_len < 1 || seq_len < *s || seq_len > INT32_MAX)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": seq_len must be at least 1, hold the bos/eos tokens and be below 2^31");
    if (seq_len > BF_MAX_L) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": seq_len above 65536 is not supported (the length classes are ranked by 16 bits)");
    if (n_docs < 0 || n_ids < 0 || n_docs >= INT32_MAX || rows_cap < 0)
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": n_docs, n_ids and rows_cap must not be negative, n_docs below 2^31 - 1");
    return HUTK_OK;
}

// the documents of a wavefront: at most max_waves wavefronts, whole chunks of 64, min_per at least
void doc_waves(int64_t n_docs, int64_t max_waves, int64_t* per_wave, int32_t* n_waves, int64_t min_per = 64) {
    int64_t per = (n_docs + max_waves - 1) / max_waves;
    per = (per + 63) / 64 * 64;
    if (per < min_per) per = min_per;
    *per_wave = per;
    *n_waves = (int32_t)((n_docs + per - 1) / per);
}

int floor_log2(int64_t v) {
    int b = 0;
    while ((v >> (b + 1)) > 0) b++;
    return b;
}

// the rows call's scratch, carved (base != nullptr) or only added up
size_t rows_carve(RowsArgs& a, uint8_t* base, int64_t n_docs, int64_t rows_cap) {
    const size_t cells = (size_t)rows_cap * (size_t)a.words;
    Carver c{base};
    a.bits = c.take<uint32_t>(cells);
    a.before = c.take<uint32_t>(cells);
    a.wsum = c.take<int64_t>((size_t)a.n_waves + 1);
    a.ws = c.take<int64_t>((size_t)n_docs + 1);
    a.row_base = c.take<int64_t>((size_t)rows_cap + 1);
    a.item_doc = c.take<int32_t>((size_t)n_docs + 1);
    return c.at;
}

template <class F>
void with_width_vec_src(int width, bool vec, bool src, F f) {
    auto pick = [&](auto w, auto v) {
        if (src) f(w, v, std::true_type{});
        else f(w, v, std::false_type{});
    };
    auto pick_v = [&](auto w) {
        if (vec) pick(w, std::true_type{});
        else pick(w, std::false_type{});
    };
    if (width == 4) pick_v(std::integral_constant<int, 4>{});
    else pick_v(std::integral_constant<int, 8>{});
}

}  // namespace

extern "C" {

int hutk_debug_bestfit_tile(void) { return BF_TILE; }

int64_t hutk_bestfit_rows_bound(int64_t n_docs, int64_t n_ids, int64_t seq_len, int s) {
    if (n_docs < 0 || n_ids < 0 || seq_len < 1 || s < 0 || s > 2 || seq_len < s || seq_len > INT32_MAX || n_docs >= INT32_MAX ||
        n_ids > INT64_MAX / 4)
        return -(int64_t)HUTK_E_ARG;
    if (n_docs == 0) return 0;
    const int64_t T = n_ids + (int64_t)s * n_docs;
    const int64_t by_fill = 2 * T / seq_len + 1, by_docs = T / seq_len + n_docs;
    return by_fill < by_docs ? by_fill : by_docs;
}

int hutk_bestfit_plan_device(const int64_t* d_offsets, int64_t n_docs, int64_t n_ids, int64_t seq_len, int32_t bos_id,
                             int32_t eos_id, int64_t rows_cap, int64_t* d_doc_map, int64_t* d_info, int32_t* d_err,
                             void* hip_stream) {
    const char* who = "hutk_bestfit_plan_device";
    int s;
    if (int rc = bestfit_sizes(who, n_docs, n_ids, seq_len, bos_id, eos_id, rows_cap, &s)) return rc;
    if (!d_offsets || !d_info || (n_docs > 0 && !d_doc_map)) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_offsets, 8) || !aligned_to(d_doc_map, 8) || !aligned_to(d_info, 8) || !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n_docs == 0) {
        HUTK_HIP_TRY(hipMemsetAsync(d_info, 0, 2 * sizeof(int64_t), st));
        return HUTK_OK;
    }
    PlanArgs a{};
    a.offs = d_offsets, a.n_docs = n_docs, a.n_ids = n_ids, a.L = (int32_t)seq_len, a.s = s;
    const int64_t max_waves = BF_COUNT_CELLS / seq_len > 1 ? BF_COUNT_CELLS / seq_len : 1;
    doc_waves(n_docs, max_waves, &a.per_wave, &a.n_waves);
    // The bounds of the walk's scratch.  A class adds at most four groups: the group its items run out in becomes three,
    // its new bins are full ones and one partly filled one.  There are at most min(L - 1, n_docs) classes with items.
    // A visit that takes a whole group leaves it with room mod l, less than half its room: at most floor(log2 L) + 1
    // of those per group; besides them a class has one visit where its items run out and one for its new bins.  And
    // every visit places an item, so there are never more visits than documents.
    const int64_t classes = seq_len - 1 < n_docs ? seq_len - 1 : n_docs;
    a.ng_cap = 4 * classes + 1;
    const int64_t by_groups = a.ng_cap * (floor_log2(seq_len) + 1) + 2 * classes;
    a.v_cap = (by_groups < n_docs ? by_groups : n_docs) + 1;
    a.doc_map = d_doc_map, a.info = d_info, a.rows_cap = rows_cap, a.err = d_err;
    const size_t cells = (size_t)a.n_waves * (size_t)seq_len;
    auto carve = [&](uint8_t* base) {
        Carver c{base};
        a.counts = c.take<uint32_t>(cells);
        a.wsum = c.take<int64_t>((size_t)a.n_waves + 1);
        a.hist = c.take<uint32_t>((size_t)seq_len);
        a.cls_vfirst = c.take<int32_t>((size_t)seq_len);
        a.cls_vcount = c.take<int32_t>((size_t)seq_len);
        a.visits = c.take<int32_t>((size_t)a.v_cap * VISIT_WORDS);
        a.nodes = c.take<int4>((size_t)a.ng_cap);
        a.next = c.take<int32_t>((size_t)a.ng_cap);
        a.heads = c.take<int32_t>((size_t)seq_len);
        return c.at;
    };
    size_t bytes = carve(nullptr);
    // The rows call that follows a plan takes rows_cap rows of these documents.  The buffer is shared, so it is made large
    // enough for that call here: growing it waits for the device, and it must not do so between the two calls.
    if (rows_cap <= INT64_MAX / 16 / seq_len) {
        RowsArgs r{};
        r.words = (int32_t)((seq_len + 31) / 32);
        int64_t per_wave;
        doc_waves(n_docs, BR_MAX_WAVES, &per_wave, &r.n_waves, BR_MIN_PER_WAVE);
        const size_t for_rows = rows_carve(r, nullptr, n_docs, rows_cap);
        if (for_rows > bytes) bytes = for_rows;
    }
    std::lock_guard<std::mutex> lock(g_bf_mu);
    BfScratch* w;
    if (int rc = scratch_for(st, bytes, &w)) return rc;
    carve(w->buf.p);
    HUTK_HIP_TRY(hipMemsetAsync(a.counts, 0, cells * sizeof(uint32_t), st));
    const dim3 grid((unsigned)((a.n_waves + TB / 64 - 1) / (TB / 64))), block(TB);
    hipLaunchKernelGGL(k_bf_count, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_bf_cols, dim3((unsigned)((seq_len + TB - 1) / TB)), block, 0, st, a);
    hutk::launch_scan_i64(a.wsum, a.n_waves, st);
    hipLaunchKernelGGL(k_bf_walk, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_bf_place, grid, block, 0, st, a);
    return scratch_used(w, st);
}

int hutk_bestfit_rows_device(const int32_t* d_ids, const int64_t* d_offsets, const int64_t* d_doc_map, int64_t n_docs,
                             int64_t n_ids, int64_t seq_len, int32_t bos_id, int32_t eos_id, int32_t pad_id, int out_width,
                             int64_t rows_cap, void* d_input_ids, int32_t* d_position_ids, int32_t* d_segment_ids,
                             int32_t* d_lengths, int64_t* d_source, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_bestfit_rows_device";
    int s;
    if (int rc = bestfit_sizes(who, n_docs, n_ids, seq_len, bos_id, eos_id, rows_cap, &s)) return rc;
    if (out_width != 4 && out_width != 8) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": out_width must be 4 or 8");
    if (rows_cap > INT64_MAX / 16 / seq_len) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": the rows are too large");
    if (!d_offsets || (n_ids > 0 && !d_ids) || (n_docs > 0 && !d_doc_map) ||
        (rows_cap > 0 && (!d_input_ids || !d_position_ids || !d_segment_ids || !d_lengths)))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_ids, 4) || !aligned_to(d_offsets, 8) || !aligned_to(d_doc_map, 8) || !aligned_to(d_input_ids, (uintptr_t)out_width) ||
        !aligned_to(d_position_ids, 4) || !aligned_to(d_segment_ids, 4) || !aligned_to(d_lengths, 4) || !aligned_to(d_source, 8) ||
        !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (rows_cap == 0) return HUTK_OK;  // (nothing to write: a plan with rows_cap 0 has said whether that is enough)
    RowsArgs a{};
    a.ids = d_ids, a.offs = d_offsets, a.doc_map = d_doc_map, a.n_docs = n_docs, a.n_ids = n_ids, a.R = rows_cap;
    a.n = rows_cap * seq_len, a.L = (int32_t)seq_len, a.s = s, a.words = (int32_t)((seq_len + 31) / 32);
    a.bos = bos_id, a.eos = eos_id, a.pad = pad_id;
    doc_waves(n_docs, BR_MAX_WAVES, &a.per_wave, &a.n_waves, BR_MIN_PER_WAVE);
    a.out = d_input_ids, a.pos = d_position_ids, a.seg = d_segment_ids, a.lengths = d_lengths, a.source = d_source, a.err = d_err;
    const bool vec = seq_len % 4 == 0 && aligned_to(d_input_ids, 16) && aligned_to(d_position_ids, 16) && aligned_to(d_segment_ids, 16) &&
                     aligned_to(d_source, 16);
    const int64_t per = TB * (vec ? 4 : 1);
    const int64_t blocks = (a.n + per - 1) / per;
    const int64_t scan_blocks = (rows_cap + TB / 64 - 1) / (TB / 64);
    if (blocks > INT32_MAX || scan_blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, std::string(who) + ": the batch is too large for one launch");
    const size_t cells = (size_t)rows_cap * (size_t)a.words;
    const size_t bytes = rows_carve(a, nullptr, n_docs, rows_cap);
    std::lock_guard<std::mutex> lock(g_bf_mu);
    BfScratch* w;
    if (int rc = scratch_for(st, bytes, &w)) return rc;
    rows_carve(a, w->buf.p, n_docs, rows_cap);
    HUTK_HIP_TRY(hipMemsetAsync(a.bits, 0, cells * sizeof(uint32_t), st));
    const dim3 block(TB);
    if (n_docs > 0) {
        const dim3 grid((unsigned)((a.n_waves + TB / 64 - 1) / (TB / 64)));
        hipLaunchKernelGGL(k_br_wsum, grid, block, 0, st, a);
        hutk::launch_scan_i64(a.wsum, a.n_waves, st);
        hipLaunchKernelGGL(k_br_docs, grid, block, 0, st, a);
    } else {
        HUTK_HIP_TRY(hipMemsetAsync(a.ws, 0, sizeof(int64_t), st));
    }
    hipLaunchKernelGGL(k_br_rowscan, dim3((unsigned)scan_blocks), block, 0, st, a);
    hutk::launch_scan_i64(a.row_base, rows_cap, st);
    if (n_docs > 0) hipLaunchKernelGGL(k_br_items, dim3((unsigned)((n_docs + TB - 1) / TB)), block, 0, st, a);
    with_width_vec_src(out_width, vec, d_source != nullptr, [&](auto wd, auto v, auto sr) {
        hipLaunchKernelGGL((k_br_write<decltype(wd)::value, decltype(v)::value, decltype(sr)::value>), dim3((unsigned)blocks), block, 0, st, a);
    });
    return scratch_used(w, st);
}

int hutk_rows_gather_source_device(const int64_t* d_source, int64_t n, const void* d_values, int64_t n_values, int width, int per,
                                   int64_t fill, void* d_out, int32_t* d_err, void* hip_stream) {
    const char* who = "hutk_rows_gather_source_device";
    if (n < 0 || n_values < 0 || (width != 4 && width != 8) || (per != 1 && per != 2))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": counts must not be negative, width is 4 or 8, per is 1 or 2");
    if (width == 4 && (fill < INT32_MIN || fill > INT32_MAX)) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": fill does not fit the width");
    if (n > 0 && (!d_source || !d_out || (n_values > 0 && !d_values))) return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is NULL");
    if (!aligned_to(d_source, 8) || !aligned_to(d_values, (uintptr_t)width) || !aligned_to(d_out, (uintptr_t)width) || !aligned_to(d_err, 4))
        return hutk::api_set_error(HUTK_E_ARG, std::string(who) + ": a buffer is not aligned to its elements");
    if (int rc = device_present(who)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (n == 0) return HUTK_OK;
    const int rb = width * per;
    // the wide path: 16-byte loads of the sources, 16-byte stores, and records read whole (16-byte ones from 16-byte places)
    const bool vec = aligned_to(d_source, 16) && aligned_to(d_out, 16) && aligned_to(d_values, (uintptr_t)rb);
    const int64_t each = TB * (vec ? 4 : 1);
    const int64_t blocks = (n + each - 1) / each;
    if (blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, std::string(who) + ": the batch is too large for one launch");
    const GatherArgs a{d_source, n, n_values, d_values, d_out, fill, d_err};
    const dim3 grid((unsigned)blocks), block(TB);
    if (rb == 4) {
        if (vec) hipLaunchKernelGGL((k_gather_source<4, true>), grid, block, 0, st, a, width);
        else hipLaunchKernelGGL((k_gather_source<4, false>), grid, block, 0, st, a, width);
    } else if (rb == 8) {
        if (vec) hipLaunchKernelGGL((k_gather_source<8, true>), grid, block, 0, st, a, width);
        else hipLaunchKernelGGL((k_gather_source<8, false>), grid, block, 0, st, a, width);
    } else {
        if (vec) hipLaunchKernelGGL((k_gather_source<16, true>), grid, block, 0, st, a, width);
        else hipLaunchKernelGGL((k_gather_source<16, false>), grid, block, 0, st, a, width);
    }
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

}  // extern "C"
