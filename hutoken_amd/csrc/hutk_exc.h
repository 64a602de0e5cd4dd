// hutk_exc.h -- the exception path of the encode pipeline: the words k_tiles / k_ptiles hand over as exception records
// (more than 32 units or 63 bytes, an end outside the tile's window, beyond the tile's prefix budget, items of several
// units).  Part of hutk_kernels.hip's translation unit, included there behind k_tiles: k_tail_small calls every routine
// in here, and they use the helpers of hutk_kdev.h.
//
//   bpe_wave, bpe_wave_big, bpe_wave_fast   the merge rule for one word by one wavefront (shifting / dead-unit marks and
//                                           per-chunk minima / links and 32-bit keys)
//   d_exc_lane, d_exc_medium                words of up to 63 bytes, one LANE per word (k_exc_a)
//   d_exc_ends                              the ends of the words whose end no tile saw; the five lists by length
//   d_exc_group_fast<2 .. 16>, d_exc_quad   words of up to 1024 / 256 units, two .. sixteen lanes per word (k_exc_b)
//   d_exc                                   the rest, one wavefront per word
//   k_exc_a, k_exc_b                        the two launches
#pragma once

// ------------------------------------------------------------------------
// The merge rule for one exception word by one wavefront: bpe_wave, bpe_wave_big, bpe_wave_fast
// ------------------------------------------------------------------------
struct LdsArr {
    uint32_t* p;
    __device__ __forceinline__ uint32_t get(int64_t i) const { return p[i]; }
    __device__ __forceinline__ void set(int64_t i, uint32_t v) const { p[i] = v; }
};
struct HbmArr {  // L1-bypassing accesses: lanes of the wave exchange data through it
    uint32_t* p;
    __device__ __forceinline__ uint32_t get(int64_t i) const {
        return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void set(int64_t i, uint32_t v) const {
        __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// minimum over the wavefront, in every lane: DPP row shifts and broadcasts (the scan's pattern; a lane without a source
// reads all ones), then lane 63's value.  (Twelve ds_bpermute round trips through the LDS pipe before: a merge of a long
// exception word does four of these reductions.)
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
    auto step = [&](auto ctrl, auto rows) {
        const uint32_t oh = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)(v >> 32), decltype(ctrl)::value, decltype(rows)::value, 0xf, false);
        const uint32_t ol = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)v, decltype(ctrl)::value, decltype(rows)::value, 0xf, false);
        const uint64_t o = ((uint64_t)oh << 32) | ol;
        v = o < v ? o : v;
    };
    step(std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
    step(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
    const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
    return ((uint64_t)h << 32) | l;
}

// Cooperative merge of n symbols held in Sa (pairs in Ma) by one wavefront.
// Dense arrays: a merge removes element p+1 by shifting the tail left.
template <class Arr>
__device__ __forceinline__ int64_t bpe_wave(const DevTables& T, Arr Sa, Arr Ma, int64_t n, int lane) {
    for (int64_t i = lane; i < n; i += 64)
        Ma.set(i, (i + 1 < n) ? pair_lookup(T, Sa.get(i), Sa.get(i + 1)) : SYM_NONE);
    wave_wg_sync();
    while (n > 1) {
        uint64_t best = ~0ull;
        for (int64_t i = lane; i + 1 < n; i += 64) {
            const uint32_t m = Ma.get(i);
            if (m != SYM_NONE) {
                const uint64_t k = ((uint64_t)rank_of(T, m) << 32) | (uint64_t)i;
                best = k < best ? k : best;
            }
        }
        best = wave_min_u64(best);
        if (best == ~0ull) break;
        const int64_t p = (int64_t)(best & 0xFFFFFFFFull);
        const uint32_t merged = Ma.get(p);
        const bool has_left = p > 0, has_right = p + 2 < n;
        const uint32_t sl = has_left ? Sa.get(p - 1) : 0u;
        const uint32_t sr = has_right ? Sa.get(p + 2) : 0u;
        wave_wg_sync();
        for (int64_t base = p + 1; base + 1 < n; base += 64) {
            const int64_t i = base + lane;
            uint32_t s = 0, m = 0;
            const bool on = i + 1 < n;
            if (on) {
                s = Sa.get(i + 1);
                m = Ma.get(i + 1);
            }
            wave_wg_sync();
            if (on) {
                Sa.set(i, s);
                Ma.set(i, m);
            }
            wave_wg_sync();
        }
        n -= 1;
        if (lane == 0) {
            Sa.set(p, merged);
            Ma.set(p, has_right ? pair_lookup(T, merged, sr) : SYM_NONE);
        }
        if (lane == 1 && has_left) Ma.set(p - 1, pair_lookup(T, sl, merged));
        wave_wg_sync();
    }
    return n;
}

constexpr int EXC_CHUNK = 256;                    // positions examined per step when a word end is unknown
constexpr int EXC_WIN = 16 + EXC_CHUNK + 16;      // staged bytes per step

// The same merge rule for words too long for the LDS arrays (up to MAX_WORD_BYTES units), in time
// O(merges x chunk) instead of O(merges x n): units stay where they are (a consumed unit is marked
// dead), and the minimum over all pairs comes from a two-level structure -- per chunk of CH units the
// best (rank, position) key in LDS (L1r/L1p, at most 1024 chunks), the global best by a wave reduction
// over those.  A merge touches three pair results, so three chunks are rescanned.  The survivors are
// compacted to the front at the end.  Sg/Mg are this word's regions of the exception arrays in HBM.
constexpr uint32_t UNIT_DEAD = 0xFFFFFFFEu;
constexpr int64_t EXC_SHIFT_MAX = 128;  // longest word in LDS that d_exc merges by shifting (bpe_wave)
template <class Arr>
__device__ __forceinline__ int64_t bpe_wave_big(const DevTables& T, Arr Sg, Arr Mg, uint32_t* L1r, uint32_t* L1p, int64_t n,
                                int lane) {
    const int64_t CH = (((n + EXC_LDS_UNITS - 1) / EXC_LDS_UNITS) + 63) & ~(int64_t)63;  // units per chunk
    const int NC = (int)((n + CH - 1) / CH);                                               // <= 1024
    for (int64_t i = lane; i < n; i += 64)
        Mg.set(i, (i + 1 < n) ? pair_lookup(T, Sg.get(i), Sg.get(i + 1)) : SYM_NONE);
    wave_wg_sync();
    auto rescan = [&](int64_t c) {  // whole wavefront: best key of chunk c -> L1
        const int64_t lo = c * CH, hi = (lo + CH < n) ? lo + CH : n;
        uint64_t best = ~0ull;
        for (int64_t i = lo + lane; i < hi; i += 64) {
            const uint32_t m = Mg.get(i);
            if (m != SYM_NONE) {
                const uint64_t k = ((uint64_t)rank_of(T, m) << 32) | (uint64_t)i;
                best = k < best ? k : best;
            }
        }
        best = wave_min_u64(best);
        if (lane == 0) {
            L1r[c] = (uint32_t)(best >> 32);
            L1p[c] = (uint32_t)best;
        }
    };
    for (int c = 0; c < NC; c++) rescan(c);
    wave_wg_sync();
    // first live unit at or after `from` (-1: none); last live unit at or before `from` (-1: none)
    auto next_live = [&](int64_t from) -> int64_t {
        for (int64_t base = from; base < n; base += 64) {
            const int64_t i = base + lane;
            const unsigned long long bal = __ballot(i < n && Sg.get(i) != UNIT_DEAD);
            if (bal) return base + __builtin_ctzll(bal);
        }
        return -1;
    };
    auto prev_live = [&](int64_t from) -> int64_t {
        for (int64_t base = from; base >= 0; base -= 64) {
            const int64_t i = base - lane;
            const unsigned long long bal = __ballot(i >= 0 && Sg.get(i) != UNIT_DEAD);
            if (bal) return base - __builtin_ctzll(bal);
        }
        return -1;
    };
    for (;;) {
        uint64_t best = ~0ull;
        for (int c = lane; c < NC; c += 64) {
            const uint64_t k = ((uint64_t)L1r[c] << 32) | (uint64_t)L1p[c];
            best = k < best ? k : best;
        }
        best = wave_min_u64(best);
        if (best == ~0ull) break;
        const int64_t p = (int64_t)(best & 0xFFFFFFFFull);
        const uint32_t merged = Mg.get(p);
        const int64_t q = next_live(p + 1);  // the unit the merge consumes (exists: the pair was a candidate)
        const int64_t q2 = next_live(q + 1), p0 = prev_live(p - 1);
        const uint32_t sr = q2 >= 0 ? Sg.get(q2) : 0u, sl = p0 >= 0 ? Sg.get(p0) : 0u;
        wave_wg_sync();
        if (lane == 0) {
            Sg.set(p, merged);
            Sg.set(q, UNIT_DEAD);
            Mg.set(q, SYM_NONE);
            Mg.set(p, q2 >= 0 ? pair_lookup(T, merged, sr) : SYM_NONE);
        }
        if (lane == 1 && p0 >= 0) Mg.set(p0, pair_lookup(T, sl, merged));
        wave_wg_sync();
        const int64_t cp = p / CH, cq = q / CH, c0 = p0 >= 0 ? p0 / CH : cp;
        rescan(cp);
        if (cq != cp) rescan(cq);
        if (c0 != cp) rescan(c0);
        wave_wg_sync();
    }
    // compaction of the survivors to the front, 64 units at a time (writes never pass the reads)
    int64_t out = 0;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t i = base + lane;
        const uint32_t sym = i < n ? Sg.get(i) : UNIT_DEAD;
        const bool live = sym != UNIT_DEAD;
        const unsigned long long bal = __ballot(live);
        wave_wg_sync();
        if (live) Sg.set(out + __popcll(bal & ((1ull << lane) - 1ull)), sym);
        out += __popcll(bal);
        wave_wg_sync();
    }
    return out;
}


// minimum over the wavefront of a 32-bit key, in every lane (the scan's DPP pattern; lane 63's value read back)
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x111, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x112, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x114, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x118, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x142, 0xa, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x143, 0xc, 0xf, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The merge rule for ONE word of 2..EXC_LDS_UNITS units held in LDS, by one wavefront -- the form for vocabularies whose
// rank is the symbol order (T.rank_is_sym); round 4: about half the time per merge of bpe_wave_big, which it replaces there.
//   Sl[i] = symbol (20 bits) | index of the NEXT live unit << 20 (11 bits, FL_NONE: none) | dead << 31
//   Ml[i] = merged symbol of (unit i, next live unit) (20 bits, PAIR_ABSENT: no rank) | index of the PREVIOUS live unit << 20
//   l1[c] = smallest key  merged symbol << 10 | index  among the 64 units of chunk c (all ones: none)
// A merge: the smallest key over the chunks (one read, one DPP reduction); its neighbours by following the links -- three
// dependent LDS reads that every lane makes at the same address, where bpe_wave_big scanned for live units with ballots;
// lanes 0 and 1 ask the pair table for the two new pairs; while those loads fly the (at most three) chunks the merge touched
// are searched again without the entries that are about to change, which are folded in when the loads are back.  No workgroup
// barrier: one wavefront, LDS in program order.
constexpr uint32_t FL_NONE = 0x7FFu, FL_SYM = 0xFFFFFu, FL_DEAD = 0x80000000u;
constexpr int FAST_LDS_UNITS = 2046;  // eleven bits of position in the key and in the links, 0x7FF means "none" (d_exc<2048>)
__device__ __forceinline__ int64_t bpe_wave_fast(const DevTables& T, uint32_t* Sl, uint32_t* Ml, uint32_t* l1, int n, int lane) {
    constexpr uint32_t NOKEY = 0xFFFFFFFFu;
    const int NC = (n + 63) >> 6;
    // links and the pair results of neighbours, every unit at once
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        uint32_t s0 = 0, s1 = 0;
        if (i < n) s0 = Sl[i] & FL_SYM;
        if (i + 1 < n) s1 = Sl[i + 1] & FL_SYM;
        wave_sync();  // (every lane has read its neighbour's plain symbol before anybody adds the link bits)
        if (i < n) {
            const uint32_t m = (i + 1 < n) ? pair_lookup(T, s0, s1) : SYM_NONE;
            Sl[i] = s0 | ((i + 1 < n ? (uint32_t)(i + 1) : FL_NONE) << 20);
            Ml[i] = (m == SYM_NONE ? PAIR_ABSENT : m) | ((i > 0 ? (uint32_t)(i - 1) : FL_NONE) << 20);
        }
    }
    wave_sync();
    auto chunk_key = [&](int c, uint32_t skip_a, uint32_t skip_b) -> uint32_t {  // smallest key of chunk c, two positions left out
        const uint32_t i = (uint32_t)(64 * c + lane);
        uint32_t k = NOKEY;
        if ((int)i < n && i != skip_a && i != skip_b) {
            const uint32_t m = Ml[i] & FL_SYM;
            if (m != PAIR_ABSENT) k = (m << 11) | i;
        }
        return wave_min_u32(k);
    };
    for (int c = 0; c < NC; c++) {
        const uint32_t k = chunk_key(c, NOKEY, NOKEY);
        if (lane == 0) l1[c] = k;
    }
    wave_sync();
    int left = n;
    for (;;) {
        const uint32_t best = wave_min_u32(lane < NC ? l1[lane] : NOKEY);
        if (best == NOKEY) break;
        const uint32_t p = best & 2047u, merged = best >> 11;
        const uint32_t sp = Sl[p], mp = Ml[p];
        const uint32_t q = (sp >> 20) & FL_NONE, p0 = (mp >> 20) & FL_NONE;  // the unit the merge consumes (there is one), the unit in front (or none)
        const uint32_t sq = Sl[q];
        const uint32_t sl0 = p0 != FL_NONE ? Sl[p0] : 0u;
        const uint32_t q2 = (sq >> 20) & FL_NONE;  // the unit behind the consumed one (or none)
        const uint32_t sr0 = q2 != FL_NONE ? Sl[q2] : 0u;
        const uint32_t mp0 = p0 != FL_NONE ? Ml[p0] : 0u, mq2 = q2 != FL_NONE ? Ml[q2] : 0u;
        // the two new pairs: lane 0 asks for (merged, right neighbour), lane 1 for (left neighbour, merged)
        uint32_t lk = SYM_NONE;
        const bool ask = (lane == 0 && q2 != FL_NONE) || (lane == 1 && p0 != FL_NONE);
        PairProbe pr{};
        const uint32_t pl = lane == 0 ? merged : (sl0 & FL_SYM), prr = lane == 0 ? (sr0 & FL_SYM) : merged;
        if (ask) pr = pair_issue(T, pl, prr);
        // the merge itself
        wave_sync();
        if (lane == 0) {
            Sl[p] = merged | (q2 << 20);
            Sl[q] = FL_DEAD;
            Ml[q] = PAIR_ABSENT | (FL_NONE << 20);
            if (q2 != FL_NONE) Ml[q2] = (mq2 & FL_SYM) | (p << 20);
        }
        left--;
        wave_sync();
        // the chunks the merge touched, without p and p0 (their pairs are being looked up) -- q is dead: its entry reads "no rank"
        const int cp = (int)(p >> 6), cq = (int)(q >> 6), c0 = p0 != FL_NONE ? (int)(p0 >> 6) : cp;
        uint32_t kp = chunk_key(cp, p, p0);
        uint32_t kq = cq != cp ? chunk_key(cq, p, p0) : NOKEY;
        uint32_t k0 = (c0 != cp && c0 != cq) ? chunk_key(c0, p, p0) : NOKEY;
        if (ask) lk = pair_resolve(T, pr, pl, prr);
        const uint32_t mr = (uint32_t)__builtin_amdgcn_readlane((int)lk, 0), ml = (uint32_t)__builtin_amdgcn_readlane((int)lk, 1);
        const uint32_t mrf = (q2 != FL_NONE && mr != SYM_NONE) ? mr : PAIR_ABSENT;
        const uint32_t mlf = (p0 != FL_NONE && ml != SYM_NONE) ? ml : PAIR_ABSENT;
        const uint32_t key_r = mrf != PAIR_ABSENT ? ((mrf << 11) | p) : NOKEY;
        const uint32_t key_l = mlf != PAIR_ABSENT ? ((mlf << 11) | p0) : NOKEY;
        kp = min(kp, key_r);
        if (c0 == cp) kp = min(kp, key_l);
        else if (c0 == cq) kq = min(kq, key_l);
        else k0 = min(k0, key_l);
        if (lane == 0) {
            Ml[p] = mrf | (p0 << 20);
            if (p0 != FL_NONE) Ml[p0] = mlf | (mp0 & ~FL_SYM);
            l1[cp] = kp;
            if (cq != cp) l1[cq] = kq;
            if (c0 != cp && c0 != cq) l1[c0] = k0;
        }
        wave_sync();
    }
    // the survivors to the front as plain symbols, 64 units at a time (writes never pass the reads)
    int out = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const uint32_t e = i < n ? Sl[i] : FL_DEAD;
        const bool live = !(e & FL_DEAD);
        const unsigned long long bal = __ballot(live);
        wave_sync();
        if (live) Sl[out + __popcll(bal & ((1ull << lane) - 1ull))] = e & FL_SYM;
        out += __popcll(bal);
        wave_sync();
    }
    (void)left;
    return out;
}

// document holding byte ws of tile `tile`: last d with offsets[d] <= ws.  The tile metadata brackets it
// (tile_first_doc = first document at or after the tile start - LOOKBACK), so the search is two or three
// probes instead of log2(n_docs).
__device__ __forceinline__ int64_t doc_of(const BatchArgs& A, const Workspace& W, int64_t ws, uint32_t tile) {
    const int64_t f = W.tile_first_doc[tile];
    int64_t lo = f > 0 ? f - 1 : 0;                                                     // offsets[lo] <= ws
    int64_t hi = ((int64_t)tile + 2 < A.n_tiles) ? W.tile_first_doc[tile + 2] : A.n_docs;  // offsets[hi] > ws
    if (hi > A.n_docs) hi = A.n_docs;
    if (hi <= lo) hi = lo + 1;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.offsets[mid] <= ws) lo = mid; else hi = mid;
    }
    return lo;
}

// One unit of a word outside byte-encoder mode, for a lane that walks its word: the character that begins at p[0], `room`
// bytes of the word left -> its symbol, *len = its bytes.  A continuation byte or F8..FF in a lead byte's place and a
// character that runs over the word's end raise HUTK_E_INVALID_UTF8 and are one byte of SYM_UNK.  d_exc_lane and d_exc_medium
// (k_exc_a) call it.  d_exc_group_fast has the same lines written out: with k_exc_b's routines rewritten, k_exc_b<true> measured
// 0.9 % slower on CJK paragraphs without seams (profiles/refactor_exc_ab.txt), so that kernel stays as it compiled before.
// d_exc, sixty-four lanes on sixty-four bytes, and k_tiles, tables in LDS, have tests of their own.
__device__ __forceinline__ uint32_t char_unit(const DevTables& T, const BatchArgs& A, const uint8_t* p, int room, int* len) {
    const uint32_t b = p[0];
    int L = (b < 0x80u) ? 1 : (b >= 0xF0u) ? 4 : (b >= 0xE0u) ? 3 : (b >= 0xC0u) ? 2 : 1;
    uint32_t sym;
    if ((b >= 0x80u && (L == 1 || b >= 0xF8u)) || L > room) {
        raise(A.err, HUTK_E_INVALID_UTF8);
        sym = SYM_UNK;
        L = 1;
    } else if (T.item_direct[b]) {
        sym = T.item_sym[b];
    } else if (L == 1) {
        sym = SYM_UNK;
    } else {
        uint32_t packed = b | ((uint32_t)p[1] << 8);
        if (L > 2) packed |= (uint32_t)p[2] << 16;
        if (L > 3) packed |= (uint32_t)p[3] << 24;
        sym = char_lookup(T, packed);
    }
    *len = L;
    return sym;
}

// ------------------------------------------------------------------------
// d_exc_medium: exception words whose end the tile could see (at most 63 bytes, so at most 63 units) and
// that were refused only for having more than 32 units (or, non-byte mode, for the prefix budget): ONE LANE
// PER WORD, 64 words per wavefront, the merge loop of k_tiles with 64-bit unit masks.  Whatever it does not
// take (unknown end, more than 64 units with a prefix) is left for k_exc_b: medium_leave puts it on its list.
// ------------------------------------------------------------------------
constexpr int MEDIUM_UNITS = 64;
constexpr int QUAD_UNITS = 256;  // longest word of exc_quad's two lists (d_exc_quad, d_exc_group_fast<4>)
// A word of known length that d_exc_medium does not take (prefix units make it longer than MEDIUM_UNITS) goes straight on
// the list of its length (exc_list_of), one atomic per wavefront and list; words of unknown length are d_exc_ends' business.
// (exc_quad is TWO lists in one array: words of up to 128 units -- prefix included, whether or not the word gets it --
// from the front, counters[CTR_G2_COUNT] of them, the longer ones from the back, counters[CTR_G4_COUNT]: d_exc_group_fast<2> and <4> each walk
// their own.  As one list, 800 k words of 70-120 letters were walked a second time, 50 k lots of a cursor atomic and
// two dependent loads each, to find nothing.)
__device__ __forceinline__ uint32_t quad_list_len(const Workspace& W) { return W.counters[CTR_G2_COUNT] + W.counters[CTR_G4_COUNT]; }
__device__ __forceinline__ uint32_t quad_list_at(const Workspace& W, uint64_t li) {
    const uint32_t ns = W.counters[CTR_G2_COUNT];
    return li < ns ? W.exc_quad[li] : W.exc_quad[W.cap_exc - 1 - (int64_t)(li - ns)];
}
constexpr int QUAD_SHORT_UNITS = 128;
constexpr int GROUP_UNITS = 1024;  // longest word of d_exc_group_fast (16 lanes per word)
// the list of a word of `units` units (the prefix counted in, whether or not the word gets it): 0 / 1 exc_quad's two lists,
// 2 / 3 exc_mid's (d_exc_group_fast<8>, <16>: 16-bit symbols with rank == symbol order only), 4 d_exc's
__device__ __forceinline__ int exc_list_of(const DevTables& T, int64_t units) {
    const bool quad_ok = (T.is_byte_encoder || T.sym16) && T.rank_is_sym && !T.has_multi;
    const bool group_ok = T.sym16 && T.rank_is_sym && !T.has_multi;
    return quad_ok && units <= QUAD_SHORT_UNITS ? 0 : quad_ok && units <= QUAD_UNITS ? 1
         : group_ok && units <= GROUP_UNITS / 2 ? 2 : group_ok && units <= GROUP_UNITS ? 3 : 4;
}
__device__ __forceinline__ uint32_t* exc_list_slot(const Workspace& W, int list, uint32_t k) {  // entry k of list 0 .. 4
    return list == 0 ? W.exc_quad + k : list == 1 ? W.exc_quad + (W.cap_exc - 1 - (int64_t)k)
         : list == 2 ? W.exc_mid + k : list == 3 ? W.exc_mid + (W.cap_exc - 1 - (int64_t)k) : W.exc_wave + k;
}
__device__ __forceinline__ uint32_t* exc_list_count(const Workspace& W, int list) {
    return W.counters + (list == 0 ? CTR_G2_COUNT : list == 1 ? CTR_G4_COUNT : list == 2 ? CTR_G8_COUNT : list == 3 ? CTR_G16_COUNT : CTR_WAVE_COUNT);
}
__device__ __forceinline__ void medium_leave(const DevTables& T, const Workspace& W, bool leave, uint64_t idx, int lane, int32_t len) {
    // (a length from k_tiles can be anything up to a tile's window; outside byte-encoder mode exc_quad's lists are d_exc_group_fast's only)
    const int list = leave ? exc_list_of(T, (int64_t)len + T.n_prefix) : -1;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int l = 0; l < 5; l++) {  // one atomic per wavefront and list
        const unsigned long long b = __ballot(list == l);
        if (b) {
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(exc_list_count(W, l), (uint32_t)__popcll(b));
            at = __shfl(at, 0, 64);
            if (list == l) *exc_list_slot(W, l, at + __popcll(b & below)) = (uint32_t)idx;
        }
    }
}

// The same for 16-bit symbols with rank == symbol order (GPT-2-shaped files, the id-keyed path): ONE DWORD PER UNIT,
// merged symbol of (unit, next live unit) << 16 | symbol of the unit, in a row of the lane's own (MEDIUM_ROW dwords), so
// that the search for the best pair reads FOUR units per LDS instruction and prices each with one v_and_or:
// key = merged << 16 | position, smallest key = minimal rank, leftmost on ties (queue.c:162-164); a dead unit and a pair
// without a rank read 0xFFFF in the upper half.  (The general form below looks its candidates up one by one through
// 64-bit masks: ~10 instructions per candidate and trip, which on words of 33..62 letters was 4/5 of the kernel's time.)
//
// d_exc_lane takes the words d_exc_medium would: up to 64 units, straight from the exception records, 64 words per wavefront,
// liveness in one 64-bit word.
constexpr int MEDIUM_ROW = MEDIUM_UNITS + 4;  // dwords per lane: 16-byte aligned rows, lanes spread over the banks
__device__ __forceinline__ void d_exc_lane(const DevTables& T, const BatchArgs& A, const Workspace& W, uint32_t vblock,
                                           uint32_t vgrid, uint8_t* lds) {
    const int lane = threadIdx.x & 63;
    uint32_t* const U = reinterpret_cast<uint32_t*>(lds) + lane * MEDIUM_ROW;
    constexpr uint32_t HI = 0xFFFF0000u;
    const uint32_t n_exc = W.counters[CTR_EXC];
    // 64 words at a time: the first lot by block index, further ones from a device cursor: words differ in
    // their number of merges, and a fixed share per wavefront left the last ones running alone
    for (uint32_t round = 0;; round++) {
        uint32_t lot = vblock;
        if (round) {
            if (lane == 0) lot = vgrid + atomicAdd(&W.counters[CTR_LANE_CURSOR], 1u);
            lot = (uint32_t)__shfl((int)lot, 0, 64);
        }
        const uint64_t base = (uint64_t)lot * 64;
        if (base >= n_exc || (int64_t)base >= W.cap_exc) break;
        const uint64_t idx = base + lane;  // the word's exception record
        bool have = idx < n_exc && (int64_t)idx < W.cap_exc;
        ExcRec rec{};
        if (have) rec = W.exc[idx];
        have = have && rec.len >= 1 && rec.len <= LANE_MAX_BYTES && rec.cnt == 0;
        have = have && !T.has_multi;  // (items of several units: every exception word goes to d_exc, which expands them)
        int64_t gbase = 0;
        int n = 0, na = 0;
        uint64_t live = 0;  // units still alive
        uint32_t best = 0xFFFFFFFFu;
        // best key of the lane's row: 16 bytes = four units per read, four reads in flight (the row reads "no rank" from
        // the word's last unit to the next multiple of 16)
        auto scan_row = [&](int nn) -> uint32_t {
            uint32_t b0 = 0xFFFFFFFFu, b1 = 0xFFFFFFFFu;
            for (int i = 0; i < nn; i += 16) {
                uint4 v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = *reinterpret_cast<const uint4*>(U + i + 4 * j);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t at = (uint32_t)(i + 4 * j);
                    b0 = min(b0, min((v[j].x & HI) | at, (v[j].y & HI) | (at + 1u)));
                    b1 = min(b1, min((v[j].z & HI) | (at + 2u), (v[j].w & HI) | (at + 3u)));
                }
            }
            return min(b0, b1);
        };
        if (have) {
            const int64_t ws = rec.ws;
            const int nb = rec.len;
            const int64_t d = T.has_prefix ? doc_of(A, W, ws, rec.tile) : 0;  // (needed for the prefix and its room in exc_tok only)
            const bool docfirst = T.has_prefix && word_is_first(A, ws, A.offsets[d]);
            const bool with_prefix = T.has_prefix && docfirst;
            const bool alone = with_prefix && doc_begins_with_space(A, ws);  // core.c:365-366, 421-446
            const int kp = (with_prefix && !alone) ? T.n_prefix : 0;
            na = alone ? T.n_prefix_alone : 0;
            gbase = ws * T.unit_scale + (int64_t)W.pad_per_doc * (docfirst ? d : d + 1);
            if (kp + nb > MEDIUM_UNITS) {
                have = false;  // k_exc_b's (medium_leave, below)
            } else {
                for (int i = 0; i < kp; i++) U[i] = HI | (T.prefix_syms[i] & 0xFFFFu);
                n = kp;
                int looked_up = 0;  // units [0, looked_up) still need their pair result from the pair table
                if (T.is_byte_encoder) {
                    // sixteen units per step: their bytes in flight together, then their (byte, next byte) table entries --
                    // merged symbol of the pair << 16 | symbol of the byte: the row's dword as it is
                    const uint8_t* wb = A.bytes + ws;
                    const uint32_t* bp = reinterpret_cast<const uint32_t*>(T.bytepair);
                    for (int i0 = 0; i0 < nb; i0 += 16) {
                        uint32_t b[17];
#pragma unroll
                        for (int j = 0; j < 17; j++) b[j] = wb[min(i0 + j, nb - 1)];  // (clamped: in bounds, no branch)
                        uint32_t e[16];
#pragma unroll
                        for (int j = 0; j < 16; j++) e[j] = bp[b[j] | (b[j + 1] << 8)];
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            if (i0 + j < nb) U[n + i0 + j] = (i0 + j + 1 < nb) ? e[j] : (e[j] | HI);
                    }
                    looked_up = n;  // (prefix units in front: their pairs, and the one into the word)
                    n += nb;
                } else {
                    for (int i = 0; i < nb;) {
                        int L;
                        const uint32_t sym = char_unit(T, A, A.bytes + ws + i, nb - i, &L);
                        U[n] = HI | (sym & 0xFFFFu);
                        n++;
                        i += L;
                    }
                    looked_up = n - 1;
                }
                for (int i0 = 0; i0 < looked_up; i0 += 4) {  // four lookups (eight loads) in flight
                    PairProbe pr[4];
                    uint32_t sy[5];
#pragma unroll
                    for (int j = 0; j < 5; j++) sy[j] = (i0 + j < n) ? (U[i0 + j] & 0xFFFFu) : 0u;
#pragma unroll
                    for (int j = 0; j < 5; j++) sy[j] = sy[j] == 0xFFFFu ? SYM_UNK : sy[j];
#pragma unroll
                    for (int j = 0; j < 4; j++) pr[j] = pair_issue(T, sy[j], sy[j + 1]);
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (i0 + j < looked_up && i0 + j + 1 < n) {
                            const uint32_t m = pair_resolve(T, pr[j], sy[j], sy[j + 1]);
                            U[i0 + j] = (m << 16) | (sy[j] & 0xFFFFu);  // (SYM_NONE: 0xFFFF in the upper half)
                        }
                }
                for (int i = n; i < ((n + 15) & ~15); i++) U[i] = 0xFFFFFFFFu;  // the row's last reads cover them
                live = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
                best = scan_row(n);
            }
        }
        // One merge per trip and lane: apply the best pair, issue the lookups of the two new neighbour pairs, search the
        // row again while those loads fly (the pairs that change read "no rank" meanwhile), fold the two new keys in.
        for (;;) {
            const bool act = have && best < HI;
            if (!__any(act)) break;
            if (act) {
                const int p = (int)(best & 0xFFFFu);
                const uint32_t merged = best >> 16;
                const uint64_t behind = ~((2ull << p) - 1ull);  // (p <= 62: a candidate pair has a unit behind it)
                const int q = __builtin_ctzll(live & behind);  // the unit the merge consumes (there is one: the pair was a candidate)
                live &= ~(1ull << q);
                const uint64_t lr = live & behind, ll = live & ((1ull << p) - 1ull);
                const bool right = lr != 0, left = ll != 0;
                const int q2 = right ? __builtin_ctzll(lr) : p;
                const int p0 = left ? 63 - __builtin_clzll(ll) : p;
                const uint32_t ur = U[q2], ul = U[p0];
                uint32_t sr = ur & 0xFFFFu, sl = ul & 0xFFFFu;
                sr = sr == 0xFFFFu ? SYM_UNK : sr;  // (a unit that is no symbol: never a member of a pair)
                sl = sl == 0xFFFFu ? SYM_UNK : sl;
                const PairProbe pr = pair_issue(T, merged, sr), pl = pair_issue(T, sl, merged);  // both in flight
                U[q] = 0xFFFFFFFFu;
                U[p0] = ul | HI;      // (first: without a left neighbour p0 == p)
                U[p] = HI | merged;
                best = scan_row(n);
                if (right) {
                    const uint32_t m = pair_resolve(T, pr, merged, sr);
                    U[p] = (m << 16) | merged;
                    best = min(best, (m << 16) | (uint32_t)p);
                }
                if (left) {
                    const uint32_t m = pair_resolve(T, pl, sl, merged);
                    U[p0] = (m << 16) | (ul & 0xFFFFu);
                    best = min(best, (m << 16) | (uint32_t)p0);
                }
            }
        }
        if (have) {
            int32_t* out = W.exc_tok + gbase;
            for (int i = 0; i < na; i++) out[i] = T.prefix_alone_ids[i];
            int k = na;
            for (uint64_t c = live; c;) {  // eight ids per step, as in d_exc_group_fast
                int pos[8];
                bool ok[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    ok[i] = c != 0;
                    pos[i] = ok[i] ? __builtin_ctzll(c) : 0;
                    c &= c - 1;
                }
                uint32_t sy[8];
#pragma unroll
                for (int i = 0; i < 8; i++) sy[i] = U[pos[i]] & 0xFFFFu;
                int32_t id[8];
#pragma unroll
                for (int i = 0; i < 8; i++) id[i] = sym_to_id(T, sy[i] == 0xFFFFu ? SYM_UNK : sy[i]);
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if (ok[i]) { out[k] = id[i]; k++; }
            }
            rec.cnt = (uint32_t)k;
            rec.tok_base = gbase;
            W.exc[idx] = rec;
            atomicAdd(&W.tile_count[rec.tile], rec.cnt);
        }
        medium_leave(T, W, !have && idx < n_exc && (int64_t)idx < W.cap_exc && rec.len >= 1 && rec.cnt == 0, idx, lane, rec.len);
    }
}

// Words of 65..1024 units with NW LANES PER WORD: d_exc_lane's rows, 32 (NW = 2: up to 128 units)
// or 16 (NW = 4) words per wavefront -- every lane at work, where the one-lane form kept 16 / 8 of 64 busy to stay within
// 8.4 KB.  What a lane did alone is shared out:
//   * the row's search, 3/4 of a trip's instructions: the row is 16-unit blocks dealt round the group (lane s: blocks s,
//     s + NW, ...: four per lane), a lane keeps the best key of each of its blocks in a register, and a trip searches again
//     only the blocks whose dwords it changed -- at most one per lane, read at a lane-dependent address, so the wavefront
//     runs the 16-unit search ONCE per trip whatever the words' lengths (a word whose live units lie so far apart that
//     a lane owns two changed blocks searches all its blocks: seldom); a DPP minimum over the group ends the trip;
//   * the liveness bits: lane s holds units 64 s .. 64 s + 63, a neighbour is a DPP minimum / maximum of the lanes' answers;
//   * the two pair lookups of a merge: lane 0 the new right pair, lane 1 the new left one.
// The search now follows the lookups (it reads their results) instead of running under them: with two or more
// wavefronts per SIMD the kernel is bound by the instructions it issues, not by a trip's latency (k_exc_b with half its
// wavefronts took the same time, profiles/r04_exc_group_ab.txt).
template <int LPW>
__device__ __forceinline__ uint32_t group_min_u32(uint32_t v) {  // minimum over each group of LPW (2 .. 16) lanes, in every lane
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    if (LPW >= 4) v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    if (LPW >= 8) v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x141, 0xf, 0xf, false));  // row_half_mirror
    if (LPW >= 16) v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x140, 0xf, 0xf, false)); // row_mirror
    return v;
}
template <int LPW>
__device__ __forceinline__ uint32_t group_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false));
    if (LPW >= 4) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false));
    if (LPW >= 8) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false));
    if (LPW >= 16) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false));
    return v;
}
template <int NW>
__device__ __forceinline__ void d_exc_group_fast(const DevTables& T, const BatchArgs& A, const Workspace& W, uint32_t vblock,
                                                 uint32_t vgrid, uint8_t* lds) {
    constexpr int LPW = NW, UNITS = 64 * NW, ROW = UNITS + 4, WPW = 64 / LPW;
    static_assert(NW == 2 || NW == 4 || NW == 8 || NW == 16, "groups within a DPP row");
    static_assert(UNITS <= GROUP_UNITS, "the lists hold words of up to GROUP_UNITS units");
    const int lane = threadIdx.x & 63, sub = lane % LPW, w = lane / LPW;
    uint32_t* const U = reinterpret_cast<uint32_t*>(lds) + w * ROW;
    constexpr uint32_t HI = 0xFFFF0000u;
    const uint32_t n_exc = W.counters[NW == 2 ? CTR_G2_COUNT : NW == 4 ? CTR_G4_COUNT : NW == 8 ? CTR_G8_COUNT : CTR_G16_COUNT];  // entries of my list (medium_leave)
    for (uint32_t round = 0;; round++) {
        uint32_t lot = vblock;
        if (round) {
            if (lane == 0) lot = vgrid + atomicAdd(&W.counters[NW == 2 ? CTR_G2_CURSOR : NW == 4 ? CTR_G4_CURSOR : NW == 8 ? CTR_G8_CURSOR : CTR_G16_CURSOR], 1u);
            lot = (uint32_t)__shfl((int)lot, 0, 64);
        }
        const uint64_t base = (uint64_t)lot * WPW;
        if (base >= n_exc) break;
        const uint64_t at = base + w;
        bool have = at < n_exc;  // (the same for a group's lanes, as everything below that does not mention sub)
        uint64_t idx = 0;
        if (have) idx = NW == 2 ? W.exc_quad[at] : NW == 4 ? W.exc_quad[W.cap_exc - 1 - (int64_t)at] : NW == 8 ? W.exc_mid[at] : W.exc_mid[W.cap_exc - 1 - (int64_t)at];
        ExcRec rec{};
        if (have) rec = W.exc[idx];
        const uint32_t rec_tile = rec.tile;  // (the record itself does not stay in registers over the trips)
        int64_t gbase = 0;
        int n = 0, na = 0;
        uint64_t lv = 0;       // the lane's share of the liveness bits: units 64 sub .. 64 sub + 63
        uint32_t bm[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // best keys of blocks sub, sub + LPW, ...
        uint32_t best = 0xFFFFFFFFu;
        // best key of the 16 units of block blk: four 16-byte reads in flight (the row reads "no rank" from the word's last
        // unit to the next multiple of 16; a block behind that is not the word's: no key)
        auto scan_block = [&](int blk) -> uint32_t {
            uint4 v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = *reinterpret_cast<const uint4*>(U + 16 * blk + 4 * j);
            uint32_t b0 = 0xFFFFFFFFu, b1 = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t at = (uint32_t)(16 * blk + 4 * j);
                b0 = min(b0, min((v[j].x & HI) | at, (v[j].y & HI) | (at + 1u)));
                b1 = min(b1, min((v[j].z & HI) | (at + 2u), (v[j].w & HI) | (at + 3u)));
            }
            return 16 * blk < n ? min(b0, b1) : 0xFFFFFFFFu;
        };
        if (have) {
            const int64_t ws = rec.ws;
            const int nb = rec.len;
            // (the word's document matters for the prefix and its room in exc_tok only: without a prefix, five dependent loads less)
            const int64_t d = T.has_prefix ? doc_of(A, W, ws, rec.tile) : 0;
            const bool docfirst = T.has_prefix && word_is_first(A, ws, A.offsets[d]);
            const bool with_prefix = T.has_prefix && docfirst;
            const bool alone = with_prefix && doc_begins_with_space(A, ws);  // core.c:365-366, 421-446
            const int kp = (with_prefix && !alone) ? T.n_prefix : 0;
            na = alone ? T.n_prefix_alone : 0;
            gbase = ws * T.unit_scale + (int64_t)W.pad_per_doc * (docfirst ? d : d + 1);
            if (kp + nb > UNITS) {
                have = false;  // (cannot be: the lists were made with the prefix counted in)
            } else {
                if (sub == 0)
                    for (int i = 0; i < kp; i++) U[i] = HI | (T.prefix_syms[i] & 0xFFFFu);
                n = kp;
                int looked_up = 0;  // units [0, looked_up) still need their pair result from the pair table
                if (T.is_byte_encoder) {
                    // eight units per step and lane, the steps dealt round the group, two steps at a time: their bytes as three
                    // unaligned dwords each (the ninth byte is the next unit's: its pair), then their sixteen byte-pair entries
                    // in flight together -- two round trips per sixteen of the lane's units
                    const uint8_t* wb = A.bytes + ws;
                    const uint32_t* bp = reinterpret_cast<const uint32_t*>(T.bytepair);
                    const bool wide_ok = ws + ((nb + 7) & ~7) + 4 <= A.n_bytes;  // (a dword may reach 11 bytes past a step's first)
                    for (int i00 = 8 * sub; i00 < nb; i00 += 16 * LPW) {
                        uint32_t wd[2][3];
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const int i0 = i00 + 8 * LPW * h;
                            if (wide_ok) {
#pragma unroll
                                for (int j = 0; j < 3; j++) {
                                    uint32_t x;
                                    __builtin_memcpy(&x, wb + min(i0, (nb - 1) & ~7) + 4 * j, 4);
                                    wd[h][j] = x;
                                }
                            } else {
#pragma unroll
                                for (int j = 0; j < 3; j++) {
                                    uint32_t x = 0;
                                    for (int q = 0; q < 4; q++) x |= (uint32_t)wb[min(i0 + 4 * j + q, nb - 1)] << (8 * q);
                                    wd[h][j] = x;
                                }
                            }
                        }
                        uint32_t e[2][8];
#pragma unroll
                        for (int h = 0; h < 2; h++)
#pragma unroll
                            for (int j = 0; j < 8; j++) {
                                const uint32_t b0 = (wd[h][j >> 2] >> (8 * (j & 3))) & 0xFFu;
                                const uint32_t b1 = (wd[h][(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu;
                                e[h][j] = bp[b0 | (b1 << 8)];
                            }
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const int i0 = i00 + 8 * LPW * h;
#pragma unroll
                            for (int j = 0; j < 8; j++)
                                if (i0 + j < nb) U[n + i0 + j] = (i0 + j + 1 < nb) ? e[h][j] : (e[h][j] | HI);
                        }
                    }
                    looked_up = n;  // (prefix units in front: their pairs, and the one into the word)
                    n += nb;
                } else {
                    if (sub == 0) {  // (characters of one to four bytes: one lane walks them)
                        for (int i = 0; i < nb;) {
                            const uint32_t b = A.bytes[ws + i];
                            int L = (b < 0x80u) ? 1 : (b >= 0xF0u) ? 4 : (b >= 0xE0u) ? 3 : (b >= 0xC0u) ? 2 : 1;
                            uint32_t sym;
                            if ((b >= 0x80u && (L == 1 || b >= 0xF8u)) || i + L > nb) {
                                raise(A.err, HUTK_E_INVALID_UTF8);
                                sym = SYM_UNK;
                                L = 1;
                            } else if (T.item_direct[b]) {
                                sym = T.item_sym[b];
                            } else if (L == 1) {
                                sym = SYM_UNK;
                            } else {
                                uint32_t packed = b | ((uint32_t)A.bytes[ws + i + 1] << 8);
                                if (L > 2) packed |= (uint32_t)A.bytes[ws + i + 2] << 16;
                                if (L > 3) packed |= (uint32_t)A.bytes[ws + i + 3] << 24;
                                sym = char_lookup(T, packed);
                            }
                            U[n] = HI | (sym & 0xFFFFu);
                            n++;
                            i += L;
                        }
                    }
                    n = __shfl(n, lane - sub, 64);
                    looked_up = n - 1;
                }
                for (int i0 = 4 * sub; i0 < looked_up; i0 += 4 * LPW) {  // four lookups (eight loads) in flight per lane
                    PairProbe pr[4];
                    uint32_t sy[5];
#pragma unroll
                    for (int j = 0; j < 5; j++) sy[j] = (i0 + j < n) ? (U[i0 + j] & 0xFFFFu) : 0u;
#pragma unroll
                    for (int j = 0; j < 5; j++) sy[j] = sy[j] == 0xFFFFu ? SYM_UNK : sy[j];
#pragma unroll
                    for (int j = 0; j < 4; j++) pr[j] = pair_issue(T, sy[j], sy[j + 1]);
                    // (a unit's dword is written by the lane that holds its step only: the next step's lane has read the
                    // symbol it needs -- the low half, which stays -- whenever it comes by)
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (i0 + j < looked_up && i0 + j + 1 < n) {
                            const uint32_t m = pair_resolve(T, pr[j], sy[j], sy[j + 1]);
                            U[i0 + j] = (m << 16) | (sy[j] & 0xFFFFu);  // (SYM_NONE: 0xFFFF in the upper half)
                        }
                }
                if (sub == 0)
                    for (int i = n; i < ((n + 15) & ~15); i++) U[i] = 0xFFFFFFFFu;  // the row's last reads cover them
                const int mine_n = n - 64 * sub;
                lv = mine_n >= 64 ? ~0ull : mine_n > 0 ? ((1ull << mine_n) - 1ull) : 0ull;
            }
        }
        // (one block at a time: unrolled, the compiler keeps all sixteen reads' registers at once)
        auto scan_all = [&]() {
#pragma unroll 1
            for (int k = 0; k < 4; k++) {
                const uint32_t r = scan_block(sub + LPW * k);
#pragma unroll
                for (int j = 0; j < 4; j++) bm[j] = k == j ? r : bm[j];
            }
        };
        if (have) {
            scan_all();
            best = group_min_u32<LPW>(min(min(bm[0], bm[1]), min(bm[2], bm[3])));
        }
        // One merge per trip and word
        for (;;) {
            const bool act = have && best < HI;
            if (!__any(act)) break;
            if (act) {
                const int p = (int)(best & 0xFFFFu);
                const uint32_t merged = best >> 16;
                auto first_after = [&](int x) -> int {  // first live unit behind x, or 0xFFFF
                    const int sx = x >> 6;
                    const uint64_t m = sub == sx ? (lv & ~((2ull << (x & 63)) - 1ull)) : sub > sx ? lv : 0ull;
                    return (int)group_min_u32<LPW>(m ? (uint32_t)(64 * sub + __builtin_ctzll(m)) : 0xFFFFu);
                };
                const int q = first_after(p);  // the unit the merge consumes (there is one: the pair was a candidate)
                if (sub == (q >> 6)) lv &= ~(1ull << (q & 63));
                const int qn = first_after(q);
                const int sp = p >> 6;
                const uint64_t mb = sub == sp ? (lv & ((1ull << (p & 63)) - 1ull)) : sub < sp ? lv : 0ull;
                const int pn = (int)group_max_u32<LPW>(mb ? (uint32_t)(64 * sub + 64 - __builtin_clzll(mb)) : 0u) - 1;  // last live unit in front of p, or -1
                const bool right = qn != 0xFFFF, left = pn >= 0;
                const bool mine = sub == 0 ? right : sub == 1 ? left : false;  // lane 0: the pair (p, qn), lane 1: (pn, p)
                uint32_t a = 0, b = 0, low = 0;
                PairProbe pr{};
                if (mine) {
                    const uint32_t un = U[sub == 0 ? qn : pn];
                    uint32_t sn = un & 0xFFFFu;
                    sn = sn == 0xFFFFu ? SYM_UNK : sn;  // (a unit that is no symbol: never a member of a pair)
                    a = sub == 0 ? merged : sn;
                    b = sub == 0 ? sn : merged;
                    low = un & 0xFFFFu;
                    pr = pair_issue(T, a, b);
                }
                if (sub == 0) U[q] = 0xFFFFFFFFu;
                // which of its blocks has the lane to search again?  The changed dwords are pn's, p's and q's: blocks bl <= bp <= bq
                const int bq = q >> 4, bl = (left ? pn : p) >> 4, bpp = p >> 4;
                const bool wide = bq - bl >= LPW;  // (a lane may own two of them)
                const int tb = (bq % LPW) == sub ? bq : (bpp % LPW) == sub ? bpp : (bl % LPW) == sub ? bl : sub;
                if (sub == 0 || mine) {  // (lane 0 stores the merged symbol whether or not it has a right neighbour)
                    const uint32_t r = pair_resolve(T, pr, a, b);
                    const uint32_t m = mine ? r : SYM_NONE;
                    U[sub == 0 ? p : pn] = (m << 16) | (sub == 0 ? merged : low);
                }
                if (wide) {
                    scan_all();
                } else {
                    const uint32_t r = scan_block(tb);
                    const int k = tb / LPW;
#pragma unroll
                    for (int j = 0; j < 4; j++) bm[j] = k == j ? r : bm[j];
                }
                best = group_min_u32<LPW>(min(min(bm[0], bm[1]), min(bm[2], bm[3])));
            }
        }
        if (have) {
            int32_t* out = W.exc_tok + gbase;
            if (sub == 0)
                for (int i = 0; i < na; i++) out[i] = T.prefix_alone_ids[i];
            // lane s: the units of its 64 liveness bits, behind those of the lanes before it
            const int cnt = __popcll(lv);
            int incl = cnt;  // inclusive scan over the group's lanes
#pragma unroll
            for (int dlt = 1; dlt < LPW; dlt *= 2) {
                const int o = __shfl_up(incl, dlt, LPW);
                if (sub >= dlt) incl += o;
            }
            const int total = na + __shfl(incl, LPW - 1, LPW);
            int k = na + incl - cnt;
            // eight ids per step: their symbols' LDS reads together, their sym_id loads together (one by one, each id was a
            // dependent LDS read and global load: 46 k of a lot's 85 k cycles outside its trips, profiles/r04_exc_group_ab.txt)
            for (uint64_t c = lv; c;) {
                int pos[8];
                bool ok[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    ok[j] = c != 0;
                    pos[j] = ok[j] ? __builtin_ctzll(c) : 0;
                    c &= c - 1;  // (0 stays 0)
                }
                uint32_t sy[8];
#pragma unroll
                for (int j = 0; j < 8; j++) sy[j] = U[64 * sub + pos[j]] & 0xFFFFu;
                int32_t id[8];
#pragma unroll
                for (int j = 0; j < 8; j++) id[j] = sym_to_id(T, sy[j] == 0xFFFFu ? SYM_UNK : sy[j]);
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (ok[j]) out[k + j] = id[j];
                k += 8;  // (the last step's surplus is not stored)
            }
            if (sub == 0) {
                W.exc[idx].cnt = (uint32_t)total;
                W.exc[idx].tok_base = gbase;
                atomicAdd(&W.tile_count[rec_tile], (uint32_t)total);
            }
        }
    }
}

template <typename SymT>
__device__ __forceinline__ void d_exc_medium(const DevTables& T, const BatchArgs& A, const Workspace& W, uint32_t vblock,
                                             uint32_t vgrid, uint8_t* lds) {
    // 16-bit symbols when the vocabulary allows: half the LDS, twice the resident wavefronts (the loop is
    // bound by the latency of its pair lookups)
    // unit i of the lane's word at Sm[i * 64 + lane]; Mm: merged symbol of (unit i, next live unit) or NONE
    SymT* const Sm = reinterpret_cast<SymT*>(lds);
    SymT* const Mm = Sm + MEDIUM_UNITS * 64;
    const int lane = threadIdx.x;
    const uint32_t n_exc = W.counters[CTR_EXC];
    for (uint64_t base = (uint64_t)vblock * 64; base < n_exc && (int64_t)base < W.cap_exc;
         base += (uint64_t)vgrid * 64) {
        const uint64_t idx = base + lane;
        bool have = idx < n_exc && (int64_t)idx < W.cap_exc;
        ExcRec rec{};
        if (have) rec = W.exc[idx];
        have = have && rec.len >= 1 && rec.len <= LANE_MAX_BYTES && rec.cnt == 0;
        have = have && !T.has_multi;  // (items of several units: every exception word goes to d_exc, which expands them)
        int64_t d = 0, gbase = 0;
        int n = 0, na = 0, pairs_to = 0;
        uint64_t live = 0, cand = 0;
        if (have) {
            const int64_t ws = rec.ws;
            const int nb = rec.len;
            d = doc_of(A, W, ws, rec.tile);
            const bool docfirst = word_is_first(A, ws, A.offsets[d]);
            const bool with_prefix = T.has_prefix && docfirst;
            const bool alone = with_prefix && doc_begins_with_space(A, ws);  // core.c:365-366, 421-446
            const int kp = (with_prefix && !alone) ? T.n_prefix : 0;
            na = alone ? T.n_prefix_alone : 0;
            gbase = ws * T.unit_scale + (int64_t)W.pad_per_doc * (docfirst ? d : d + 1);
            if (kp + nb > MEDIUM_UNITS) {
                have = false;  // k_exc_b's (medium_leave, below)
            } else {
                for (int i = 0; i < kp; i++) Sm[i * 64 + lane] = Sym<SymT>::narrow(T.prefix_syms[i]);
                n = kp;
                if (T.is_byte_encoder) {
                    // sixteen units per step: their bytes in flight together, then their (byte, next byte) table entries --
                    // {symbol of the byte, merged symbol of the pair}, as in k_tiles -- together: two round trips per step
                    // instead of two per unit (a word of 47 letters: 6 instead of ~100)
                    const uint8_t* wb = A.bytes + ws;
                    const typename Sym<SymT>::Pair* bp = reinterpret_cast<const typename Sym<SymT>::Pair*>(T.bytepair);
                    for (int i0 = 0; i0 < nb; i0 += 16) {
                        uint32_t b[17];
#pragma unroll
                        for (int j = 0; j < 17; j++) b[j] = wb[min(i0 + j, nb - 1)];  // (clamped: in bounds, no branch)
                        typename Sym<SymT>::Pair e[16];
#pragma unroll
                        for (int j = 0; j < 16; j++) e[j] = bp[b[j] | (b[j + 1] << 8)];
#pragma unroll
                        for (int j = 0; j < 16; j++) {
                            const int i = i0 + j;
                            if (i < nb) {
                                Sm[(n + i) * 64 + lane] = Sym<SymT>::pair_sym(e[j]);
                                if (i + 1 < nb) {
                                    const SymT mv = Sym<SymT>::pair_merged(e[j]);
                                    Mm[(n + i) * 64 + lane] = mv;
                                    if (mv != Sym<SymT>::NONE) cand |= 1ull << (n + i);
                                }
                            }
                        }
                    }
                    pairs_to = n;  // (prefix units in front: their pairs, and the one into the word, are looked up below)
                    n += nb;
                } else {
                    for (int i = 0; i < nb;) {
                        int L;
                        const uint32_t sym = char_unit(T, A, A.bytes + ws + i, nb - i, &L);
                        Sm[n * 64 + lane] = Sym<SymT>::narrow(sym);
                        n++;
                        i += L;
                    }
                }
                live = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
                // pair results by table lookup: all of them outside byte-encoder mode; in it only those with a prefix unit
                // (units [0, pairs_to] as left members), the rest came with the (byte, next byte) entries
                for (int i0 = 0; i0 + 1 < (T.is_byte_encoder ? pairs_to + 1 : n); i0 += 4) {  // four lookups (eight loads) in flight
                    PairProbe pr[4];
                    uint32_t sy[5];
#pragma unroll
                    for (int j = 0; j < 5; j++) sy[j] = (i0 + j < n) ? Sym<SymT>::widen(Sm[(i0 + j) * 64 + lane]) : 0u;
#pragma unroll
                    for (int j = 0; j < 4; j++) pr[j] = pair_issue(T, sy[j], sy[j + 1]);
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (i0 + j + 1 < n && (!T.is_byte_encoder || i0 + j < pairs_to)) {
                            const uint32_t m = pair_resolve(T, pr[j], sy[j], sy[j + 1]);
                            Mm[(i0 + j) * 64 + lane] = Sym<SymT>::narrow(m);
                            if (m != SYM_NONE) cand |= 1ull << (i0 + j);
                        }
                }
            }
        }
        // One merge per trip and lane: the candidate of minimal rank, leftmost on ties (queue.c:162-164).  As in
        // k_tiles the lane keeps its best pair (br, bp, bm) across trips: a trip applies it, issues the lookups of
        // the two new neighbour pairs, rescans the untouched candidates while those loads fly (four LDS reads per
        // step), and picks the next best among {rescan, new right pair, new left pair}.
        const bool ris = T.rank_is_sym != 0;
        auto RKm = [&](uint32_t m) -> uint32_t { return ris ? m : ((uint32_t)T.sym_id[m] ^ 0x80000000u); };
        auto scan4 = [&](uint64_t c, uint32_t& br, int& bp, uint32_t& bm) {
            while (c) {
                const uint64_t c1 = c & (c - 1), c2 = c1 & (c1 - 1), c3 = c2 & (c2 - 1);
                const int i0 = __builtin_ctzll(c);
                const int i1 = c1 ? __builtin_ctzll(c1) : i0, i2 = c2 ? __builtin_ctzll(c2) : i0,
                          i3 = c3 ? __builtin_ctzll(c3) : i0;
                const uint32_t m0 = Sym<SymT>::widen(Mm[i0 * 64 + lane]), m1 = Sym<SymT>::widen(Mm[i1 * 64 + lane]),
                               m2 = Sym<SymT>::widen(Mm[i2 * 64 + lane]), m3 = Sym<SymT>::widen(Mm[i3 * 64 + lane]);
                const uint32_t r0 = RKm(m0), r1 = RKm(m1), r2 = RKm(m2), r3 = RKm(m3);
                if (r0 < br) { br = r0; bp = i0; bm = m0; }
                if (r1 < br) { br = r1; bp = i1; bm = m1; }
                if (r2 < br) { br = r2; bp = i2; bm = m2; }
                if (r3 < br) { br = r3; bp = i3; bm = m3; }
                c = c3 & (c3 - 1);
            }
        };
        uint32_t br = 0xFFFFFFFFu, bm = 0;
        int bp = 0;
        if (have) scan4(cand, br, bp, bm);
        for (;;) {
            const bool act = have && cand != 0;
            if (!__any(act)) break;
            if (act) {
                const int p = bp;
                const uint32_t merged = bm;
                const uint64_t above = live & ~((2ull << p) - 1ull);
                const int q = __builtin_ctzll(above);  // the unit the merge consumes
                Sm[p * 64 + lane] = Sym<SymT>::narrow(merged);
                live &= ~(1ull << q);
                cand &= ~((1ull << q) | (1ull << p));
                const uint64_t right = above & (above - 1ull);
                const uint64_t left = live & ((1ull << p) - 1ull);
                const int p0 = left ? 63 - __builtin_clzll(left) : 0;
                const uint32_t sr = right ? Sym<SymT>::widen(Sm[__builtin_ctzll(right) * 64 + lane]) : 0u;
                const uint32_t sl = left ? Sym<SymT>::widen(Sm[p0 * 64 + lane]) : 0u;
                const PairProbe pr = pair_issue(T, merged, sr), pl = pair_issue(T, sl, merged);  // both in flight
                if (left) cand &= ~(1ull << p0);
                br = 0xFFFFFFFFu;
                scan4(cand, br, bp, bm);
                if (right) {
                    const uint32_t m = pair_resolve(T, pr, merged, sr);
                    Mm[p * 64 + lane] = Sym<SymT>::narrow(m);
                    if (m != SYM_NONE) {
                        cand |= 1ull << p;
                        const uint32_t r = RKm(m);
                        if (r < br || (r == br && p < bp)) { br = r; bp = p; bm = m; }
                    }
                }
                if (left) {
                    const uint32_t m = pair_resolve(T, pl, sl, merged);
                    Mm[p0 * 64 + lane] = Sym<SymT>::narrow(m);
                    if (m != SYM_NONE) {
                        cand |= 1ull << p0;
                        const uint32_t r = RKm(m);
                        if (r < br || (r == br && p0 < bp)) { br = r; bp = p0; bm = m; }
                    }
                }
            }
        }
        if (have) {
            int32_t* out = W.exc_tok + gbase;
            for (int i = 0; i < na; i++) out[i] = T.prefix_alone_ids[i];
            int k = na;
            for (uint64_t c = live; c; c &= c - 1) out[k++] = sym_to_id(T, Sym<SymT>::widen(Sm[__builtin_ctzll(c) * 64 + lane]));
            rec.cnt = (uint32_t)k;
            rec.tok_base = gbase;
            W.exc[idx] = rec;
            atomicAdd(&W.tile_count[rec.tile], rec.cnt);
        }
        medium_leave(T, W, !have && idx < n_exc && (int64_t)idx < W.cap_exc && rec.len >= 1 && rec.cnt == 0, idx, lane, rec.len);
    }
}

// ------------------------------------------------------------------------
// d_exc_quad: words of 64..256 units (byte-encoder mode, rank == symbol order): SIXTEEN LANES PER WORD, four
// words per wavefront.  Lane l of a group owns units 16l..16l+15: it keeps the best (rank, position) key of
// its own pairs in a register, the group minimum is a DPP row reduction, a consumed unit is marked dead
// (no compaction), and only the lanes whose pairs changed rescan.  A merge costs one round trip of pair
// lookups for four words at once instead of ~2 us for one word in d_exc.
// ------------------------------------------------------------------------
__device__ __forceinline__ uint32_t row_min_u32(uint32_t v) {  // minimum over each row of 16 lanes, in every lane
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x111, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x112, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x114, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x118, 0xf, 0xf, false));
    return (uint32_t)__shfl((int)v, (int)((threadIdx.x & 63) | 15), 64);  // lane 15 of the row holds it
}
__device__ __forceinline__ uint32_t row_excl_sum(uint32_t v) {  // exclusive prefix sum inside each row of 16 lanes
    uint32_t inc = v;
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x111, 0xf, 0xf, false);
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x112, 0xf, 0xf, false);
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x114, 0xf, 0xf, false);
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x118, 0xf, 0xf, false);
    return inc - v;
}

__device__ __forceinline__ void d_exc_quad(const DevTables& T, const BatchArgs& A, const Workspace& W, uint32_t vblock,
                                           uint32_t vgrid, uint8_t* lds) {
    uint32_t* const Sq = reinterpret_cast<uint32_t*>(lds);
    uint32_t* const Mq = Sq + 4 * QUAD_UNITS;
    const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15, gl0 = lane & 48;  // group, lane in group, its lane 0
    uint32_t* Sg = Sq + g * QUAD_UNITS;
    uint32_t* Mg = Mq + g * QUAD_UNITS;
    const uint32_t n_list = quad_list_len(W);
    for (uint32_t base = vblock * 4; base < n_list; base += vgrid * 4) {
        const uint32_t li = base + g;
        bool have = li < n_list;
        uint32_t idx = 0;
        ExcRec rec{};
        if (have) {
            idx = quad_list_at(W, li);
            rec = W.exc[idx];
        }
        int n = 0, na = 0;
        int64_t gbase = 0;
        if (have) {
            const int64_t ws = rec.ws;
            const int64_t d = T.has_prefix ? doc_of(A, W, ws, rec.tile) : 0;  // (needed for the prefix and its room in exc_tok only)
            const bool docfirst = T.has_prefix && word_is_first(A, ws, A.offsets[d]);
            const bool with_prefix = T.has_prefix && docfirst;
            const bool alone = with_prefix && doc_begins_with_space(A, ws);
            const int kp = (with_prefix && !alone) ? T.n_prefix : 0;
            na = alone ? T.n_prefix_alone : 0;
            gbase = ws * T.unit_scale + (int64_t)W.pad_per_doc * (docfirst ? d : d + 1);
            {
                n = kp + rec.len;  // <= QUAD_UNITS: the ends pass checked
                for (int i = l; i < kp; i += 16) Sg[i] = T.prefix_syms[i];
                for (int i = l; i < rec.len; i += 16) Sg[kp + i] = T.item_sym[A.bytes[ws + i]];
            }
        }
        wave_sync();
        // my 16 units: pair results and liveness
        const int lo = 16 * l;
        uint32_t live16 = 0;
        if (have) {
            const int cnt = n - lo;
            live16 = cnt >= 16 ? 0xFFFFu : cnt > 0 ? ((1u << cnt) - 1u) : 0u;
        }
        for (int k0 = 0; k0 < 16; k0 += 4) {  // four lookups in flight
            PairProbe pr[4];
            uint32_t sy[5];
#pragma unroll
            for (int j = 0; j < 5; j++) sy[j] = (have && lo + k0 + j < n) ? Sg[lo + k0 + j] : 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) pr[j] = pair_issue(T, sy[j], sy[j + 1]);
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (have && lo + k0 + j < n)
                    Mg[lo + k0 + j] = (lo + k0 + j + 1 < n) ? pair_resolve(T, pr[j], sy[j], sy[j + 1]) : SYM_NONE;
        }
        wave_sync();
        bool dirty = true;
        uint32_t mybest = 0xFFFFFFFFu;  // (merged symbol = rank) << 8 | unit index, over my live units
        for (;;) {
            if (dirty) {
                mybest = 0xFFFFFFFFu;
                for (uint32_t c = live16; c; c &= c - 1) {
                    const int i = lo + __builtin_ctz(c);
                    const uint32_t m = Mg[i];
                    if (m != SYM_NONE) mybest = min(mybest, (m << 8) | (uint32_t)i);
                }
                dirty = false;
            }
            const uint32_t gbest = row_min_u32(have ? mybest : 0xFFFFFFFFu);
            const bool act = gbest != 0xFFFFFFFFu;
            if (!__any(act)) break;
            // neighbours of the pair, from the per-lane liveness masks of the group (all shuffles unconditional)
            const int p = (int)(gbest & 0xFFu);
            const uint32_t ne = (uint32_t)(__ballot(live16 != 0) >> gl0) & 0xFFFFu;  // lanes of my group with live units
            auto live_of = [&](int x) -> uint32_t { return (uint32_t)__shfl((int)live16, gl0 | (x & 15), 64); };
            auto next_after = [&](int pos) -> int {
                const int lx = pos >> 4;
                const uint32_t a = live_of(lx) & ~((2u << (pos & 15)) - 1u) & 0xFFFFu;
                const uint32_t m = ne & ~((2u << lx) - 1u) & 0xFFFFu;
                const int ly = m ? __builtin_ctz(m) : 0;
                const uint32_t lv = live_of(ly);
                return a ? (pos & ~15) + __builtin_ctz(a) : (m && lv) ? 16 * ly + __builtin_ctz(lv) : -1;
            };
            auto prev_before = [&](int pos) -> int {
                const int lx = pos >> 4;
                const uint32_t a = live_of(lx) & ((1u << (pos & 15)) - 1u);
                const uint32_t m = ne & ((1u << lx) - 1u);
                const int ly = m ? 31 - __builtin_clz(m) : 0;
                const uint32_t lv = live_of(ly);
                return a ? (pos & ~15) + (31 - __builtin_clz(a)) : (m && lv) ? 16 * ly + (31 - __builtin_clz(lv)) : -1;
            };
            const int q = next_after(act ? p : 0);           // the unit the merge consumes
            const int q2 = next_after(q >= 0 ? q : 0);
            const int p0 = prev_before(act ? p : 0);
            const uint32_t merged = gbest >> 8;
            const uint32_t sr = (act && q >= 0 && q2 >= 0) ? Sg[q2] : 0u;
            const uint32_t sl = (act && p0 >= 0) ? Sg[p0] : 0u;
            const PairProbe prr = pair_issue(T, merged, sr), prl = pair_issue(T, sl, merged);
            const uint32_t mr = (act && q >= 0 && q2 >= 0) ? pair_resolve(T, prr, merged, sr) : SYM_NONE;
            const uint32_t ml = (act && p0 >= 0) ? pair_resolve(T, prl, sl, merged) : SYM_NONE;
            wave_sync();  // everybody has read S before the owners write
            if (act && q >= 0) {
                if (l == (p >> 4)) {
                    Sg[p] = merged;
                    Mg[p] = mr;
                    dirty = true;
                }
                if (l == (q >> 4)) {
                    live16 &= ~(1u << (q & 15));
                    Mg[q] = SYM_NONE;
                    dirty = true;
                }
                if (p0 >= 0 && l == (p0 >> 4)) {
                    Mg[p0] = ml;
                    dirty = true;
                }
            }
            wave_sync();
        }
        // survivors in order: alone ids, then each lane's live units at its row prefix
        const uint32_t mine = (uint32_t)__popc(live16);
        const uint32_t before = row_excl_sum(have ? mine : 0u);
        const uint32_t total = (uint32_t)__shfl((int)(before + (have ? mine : 0u)), lane | 15, 64);
        if (have) {
            int32_t* out = W.exc_tok + gbase;
            for (int i = l; i < na; i += 16) out[i] = T.prefix_alone_ids[i];
            uint32_t k = (uint32_t)na + before;
            for (uint32_t c = live16; c; c &= c - 1) out[k++] = sym_to_id(T, Sg[lo + __builtin_ctz(c)]);
            if (l == 0) {
                rec.cnt = (uint32_t)na + total;
                rec.tok_base = gbase;
                W.exc[idx] = rec;
                atomicAdd(&W.tile_count[rec.tile], rec.cnt);
            }
        }
        wave_sync();
    }
}

// The splitter's window of a wavefront: word starts of EXC_CHUNK positions from `base`, computed with the bytes of document
// `doc` (the others read as zero), one bit per position.  Exception words of one tile follow each other closely, so the
// window that held one word's end usually holds the next one's as well and is not staged again.
struct EndsWin {
    int64_t base = -1, doc = -1;
    unsigned long long bits[EXC_CHUNK / 64];
};
// End of a word whose end its tile could not see (more than 63 bytes, or beyond the tile's window): the splitter's rule
// applied 256 positions at a time (src/parser.c:24-183 as in k_tiles' exact form), or -- regex pre-token path -- the next
// start bit of the host's bitmap.  One wavefront; sb / scode / docm are its LDS scratch, cw its window (above).
// -> end offset; *too_large when the word passes the reference's limit (core.c:402-407).
__device__ int64_t exc_word_end(const DevTables& T, const BatchArgs& A, int64_t ws, int64_t d, int64_t ds, int64_t de, uint8_t* sb,
                                uint8_t* scode, uint32_t* docm, int lane, bool* too_large, EndsWin& cw, bool seams = true) {
    int64_t we = -1;
    *too_large = false;
    if (A.word_bits) {
        for (int64_t wi = (ws + 1) >> 5; we < 0; wi += 64) {
            const int64_t w = wi + lane;
            uint32_t bits = (w << 5) <= A.n_bytes ? A.word_bits[w] : 0u;
            if (w == ((ws + 1) >> 5)) bits &= ~0u << ((ws + 1) & 31);
            const unsigned long long bal = __ballot(bits != 0);
            if (bal) {
                const int l0 = __builtin_ctzll(bal);
                const uint32_t b0 = (uint32_t)__shfl((int)bits, l0, 64);
                we = ((wi + l0) << 5) + __builtin_ctz(b0);
            } else if ((wi << 5) > A.n_bytes) {
                we = A.n_bytes;  // (cannot happen: the host sets the bit at n_bytes)
            }
        }
        if (we - ws > MAX_WORD_BYTES) *too_large = true;
        return we;
    }
    for (int64_t pos = ws + 1; we < 0;) {  // (every value here is the same in all lanes)
        if (pos - ws > MAX_WORD_BYTES + 1) { *too_large = true; break; }
        if (!(cw.doc == d && pos >= cw.base && pos < cw.base + EXC_CHUNK)) {
            const int64_t base = pos;
            const int64_t g0 = base - 16;  // global offset of window index 0
            for (int i = lane; i < EXC_WIN; i += 64) {
                const int64_t q = g0 + i;
                sb[i] = (q >= ds && q < de) ? A.bytes[q] : (uint8_t)0;
            }
            if (lane < EXC_WIN / 32 + 1) docm[lane] = 0;
            wave_sync();
            if (lane == 0) {
                if (ds >= g0 && ds < g0 + EXC_WIN) docm[(ds - g0) >> 5] |= 1u << ((ds - g0) & 31);
                if (de >= g0 && de < g0 + EXC_WIN) docm[(de - g0) >> 5] |= 1u << ((de - g0) & 31);
            }
            wave_sync();
            for (int i = lane; i < EXC_WIN; i += 64)
                scode[i] = (i >= 4 && i < EXC_WIN - 4) ? code_at(sb, docm, i) : (uint8_t)C_BAD;
            wave_sync();
#pragma unroll
            for (int r = 0; r < EXC_CHUNK / 64; r++) {
                const int64_t q = base + 64 * r + lane;
                const int wi = 16 + 64 * r + lane;
                bool st = (q <= de) && word_starts(scode, docm, wi);
                if (seams && T.seam_on && q < de && sb[wi] >= 0xE0u)  // a seam starts a word as well (k_tiles, phase 3)
                    st = st || !((T.seam_hi[sb[wi - 1]] >> (sb[wi] & 31u)) & 1u);
                cw.bits[r] = __ballot(st);
            }
            wave_sync();
            cw.base = base;
            cw.doc = d;
        }
        const int rel = (int)(pos - cw.base);
#pragma unroll
        for (int r = 0; r < EXC_CHUNK / 64; r++) {
            if (we >= 0 || 64 * (r + 1) <= rel) continue;
            unsigned long long m = cw.bits[r];
            if (rel > 64 * r) m &= ~0ull << (rel - 64 * r);
            if (m) we = cw.base + 64 * r + __builtin_ctzll(m);
        }
        pos = cw.base + EXC_CHUNK;
    }
    return we;
}

// d_exc_ends: the words whose end their tile could not see.  One wavefront per tile that has exception words (the list
// k_tiles made): for each such word of the tile the end is found and stored, and the word goes on the list of its length (exc_list_of:
// two .. sixteen lanes per word in k_exc_b, or d_exc's, a wavefront per word) --
// collected per wavefront, one atomic per flush and list.  A word over the reference's limit cuts its document (no list).
constexpr int ENDS_LIST = TILE_BYTES / 2 + 4;  // a tile has at most that many exception words
struct EndsLds {
    __attribute__((aligned(16))) uint8_t sb[EXC_WIN];
    uint8_t scode[EXC_WIN];
    uint32_t docm[EXC_WIN / 32 + 1];
    uint32_t lq[ENDS_LIST], lm[ENDS_LIST], lw[ENDS_LIST];
};
constexpr uint32_t ENDS_SHARE = 1;  // wavefronts that share the words of one tile (one: the splitter's window is reused from word to word)
__device__ __forceinline__ void d_exc_ends(const DevTables& T, const BatchArgs& A, const Workspace& W, uint32_t vblock,
                                           uint32_t vgrid, uint8_t* lds) {
    EndsLds& L = *reinterpret_cast<EndsLds*>(lds);
    uint32_t* const lq = L.lq;
    uint32_t* const lm = L.lm;
    uint32_t* const lw = L.lw;
    const int lane = threadIdx.x;
    const uint32_t n_tiles_exc = W.counters[CTR_EXC_TILES];
    // The lists' places are claimed once per WAVEFRONT, not per tile: the entries of its tiles wait in LDS (a tile's
    // fit behind what is there, or the lists are written out first).  One atomic per tile on the same words was
    // ~50 k same-address atomics for 800 k words of 70-120 letters -- at ~12 ns each most of k_exc_a's 0.65 ms.
    // (lq: lists 0 and 1 from its two ends, lm: lists 2 and 3, lw: d_exc's -- exc_list_of)
    uint32_t nl[5] = {0, 0, 0, 0, 0};  // (the same in every lane)
    auto lds_slot = [&](int list, uint32_t k) -> uint32_t* {
        return list == 0 ? lq + k : list == 1 ? lq + (ENDS_LIST - 1 - k) : list == 2 ? lm + k : list == 3 ? lm + (ENDS_LIST - 1 - k) : lw + k;
    };
    auto flush = [&]() {
        wave_sync();
#pragma unroll
        for (int l = 0; l < 5; l++) {
            if (nl[l] == 0) continue;
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(exc_list_count(W, l), nl[l]);
            at = __shfl(at, 0, 64);
            for (uint32_t i = lane; i < nl[l]; i += 64) *exc_list_slot(W, l, at + i) = *lds_slot(l, i);
            nl[l] = 0;
        }
        wave_sync();
    };
    for (uint32_t ti = vblock / ENDS_SHARE; ti < n_tiles_exc; ti += vgrid / ENDS_SHARE) {
        const uint32_t tile = W.exc_tiles[ti];
        const uint32_t first = W.tile_exc_first[tile], nexc = W.tile_nexc[tile];
        if (max(max(nl[0] + nl[1], nl[2] + nl[3]), nl[4]) + nexc > (uint32_t)ENDS_LIST) flush();
        // The tile's records sixty-four at a time, ONE LANE PER WORD of unknown length.  Its end is the first word start of
        // the tiles behind (tile_first_start: what every tile found among its own 1024 positions, seams and document starts
        // included -- my tile saw none between the word and its window's end): one load for a word that ends in the next
        // tile.  (Rounds 2-4 staged and classified the text again here, 256 positions at a time, a wavefront per word:
        // k_exc_a was 1.0 of 3.3 ms on CJK paragraphs without seams, 0.5 of 2.3 on words of 70-120 letters.)
        static_assert(ENDS_SHARE == 1, "one wavefront per tile");
        const unsigned long long below = (1ull << lane) - 1ull;
        for (uint32_t e0 = 0; e0 < nexc; e0 += 64) {
            const uint32_t idx = first + e0 + lane;
            const bool unk = e0 + lane < nexc && (int64_t)idx < W.cap_exc && W.exc[idx].len < 0;
            int list = -1;
            if (unk) {
                const int64_t ws = W.exc[idx].ws;
                int64_t we = -1;
                // (a word over the reference's limit of MAX_WORD_BYTES ends the search: it is refused below whatever its end)
                const int64_t u_end = min((int64_t)A.n_tiles, (int64_t)tile + 3 + MAX_WORD_BYTES / TILE_BYTES);
                for (int64_t u = (int64_t)tile + 1; u < u_end; u++) {
                    const uint32_t fs = W.tile_first_start[u];
                    if (fs != 0xFFFFu) { we = u * TILE_BYTES + fs; break; }
                }
                if (we < 0) we = u_end < A.n_tiles ? ws + MAX_WORD_BYTES + 1 : A.n_bytes;  // (no start within the limit / up to the text's end)
                if (we > A.n_bytes) we = A.n_bytes;
                const int64_t nb = we - ws;
                if (nb > MAX_WORD_BYTES) {
                    const int64_t d = doc_of(A, W, ws, tile), ds = A.offsets[d];
                    raise(A.err, HUTK_E_WORD_TOO_LARGE);
                    if (A.status) A.status[d] = HUTK_DOC_WORD_TOO_LARGE;
                    W.exc[idx].cnt = 0;
                    W.exc[idx].tok_base = -(ws - ds) - 1;  // where the document is cut (negative marks "no ids")
                } else {
                    W.exc[idx].len = (int32_t)nb;
                    // (the list by the length with the prefix, whether or not this word gets it: d_exc_group_fast<NW> takes its list whole)
                    list = exc_list_of(T, nb + T.n_prefix);
                }
            }
#pragma unroll
            for (int l = 0; l < 5; l++) {
                const unsigned long long bl = __ballot(list == l);
                if (list == l) *lds_slot(l, nl[l] + (uint32_t)__popcll(bl & below)) = idx;
                nl[l] += (uint32_t)__popcll(bl);
            }
        }
    }
    if (nl[0] | nl[1] | nl[2] | nl[3] | nl[4]) flush();
}

// d_exc: the words that need a whole wavefront (exc_wave; their lengths are known by now): first entry by block
// index, further ones from a device cursor.
// LU: units of the two LDS arrays -- EXC_LDS_UNITS (1024), or 2048 where the words of up to 1024 units have gone to
// d_exc_group_fast and the LDS they needed is free (k_exc_b<true>): words of up to 2046 units merge in LDS then, where at
// 1025 they used to fall to the arrays in HBM (CJK paragraphs of 1025..1200 bytes under a dense vocabulary: most of k_exc_b).
template <int LU = EXC_LDS_UNITS>
__device__ __forceinline__ void d_exc(const DevTables& T, const BatchArgs& A, const Workspace& W, uint32_t vblock,
                                      uint32_t vgrid, uint8_t* lds) {
    static_assert(LU == EXC_LDS_UNITS || LU == 2048, "bpe_wave_big's chunk arrays are EXC_LDS_UNITS entries of them");
    uint32_t* const Sl = reinterpret_cast<uint32_t*>(lds);
    uint32_t* const Ml = Sl + LU;

    const int lane = threadIdx.x & 63;  // (k_exc_b runs two of these per workgroup, each wavefront on its own: no s_barrier in here)
    const uint32_t n_list = W.counters[CTR_WAVE_COUNT];
    for (uint32_t round = 0;; round++) {
        uint32_t li = vblock;
        if (round) {
            if (lane == 0) li = vgrid + atomicAdd(&W.counters[CTR_WAVE_CURSOR], 1u);
            li = (uint32_t)__builtin_amdgcn_readfirstlane((int)li);
        }
        if (li >= n_list) break;
        const uint32_t idx = W.exc_wave[li];
        ExcRec rec = W.exc[idx];
        const int64_t ws = rec.ws;
        const int64_t d = T.has_prefix ? doc_of(A, W, ws, rec.tile) : 0;  // (needed for the prefix and its room in exc_tok only)
        const int64_t nb = rec.len;
        const bool docfirst = T.has_prefix && word_is_first(A, ws, A.offsets[d]);
        const bool with_prefix = T.has_prefix && docfirst;
        const bool alone = with_prefix && doc_begins_with_space(A, ws);  // core.c:365-366, 421-446
        const int kp = (with_prefix && !alone) ? T.n_prefix : 0;
        const int64_t gbase = ws * T.unit_scale + (int64_t)W.pad_per_doc * (docfirst ? d : d + 1);  // unit_scale slots per byte: room for an expanded word

        // unit count
        int64_t n_units;
        // units of the item that starts at byte i (0 inside a character): one, unless its replacement has several or none
        auto item_units = [&](int64_t i, uint32_t b) -> uint32_t {
            if (i >= nb || (!T.is_byte_encoder && is_cont(b))) return 0u;
            return (T.is_byte_encoder || T.item_direct[b]) ? T.item_units_off[b + 1] - T.item_units_off[b] : 1u;
        };
        if (T.has_multi) {
            int64_t cnt = 0;
            for (int64_t i0 = 0; i0 < nb; i0 += 64) {
                const int64_t i = i0 + lane;
                uint32_t c = item_units(i, i < nb ? A.bytes[ws + i] : 0x80u), tot;
                (void)wave_excl_scan(c, lane, &tot);
                cnt += tot;
            }
            n_units = cnt;
        } else if (T.is_byte_encoder) {
            n_units = nb;
        } else {
            int64_t cnt = 0;
            for (int64_t i0 = 0; i0 < nb; i0 += 64) {
                const int64_t i = i0 + lane;
                const bool lead = i < nb && !is_cont(A.bytes[ws + i]);
                cnt += __popcll(__ballot(lead));
            }
            n_units = cnt;
        }
        const int64_t n = n_units + kp;
        const bool in_lds = n <= (LU == EXC_LDS_UNITS ? EXC_LDS_UNITS : FAST_LDS_UNITS);
        LdsArr Sl_a{Sl}, Ml_a{Ml};
        HbmArr Sg_a{W.exc_sym + gbase}, Mg_a{W.exc_mrg + gbase};

        // initial symbols
        for (int i = lane; i < kp; i += 64) {
            if (in_lds) Sl_a.set(i, T.prefix_syms[i]); else Sg_a.set(i, T.prefix_syms[i]);
        }
        if (T.has_multi) {
            // expansion: every item writes its units behind those of the items in front of it
            int64_t ubase = kp;
            for (int64_t i0 = 0; i0 < nb; i0 += 64) {
                const int64_t i = i0 + lane;
                const uint32_t b = i < nb ? A.bytes[ws + i] : 0x80u;
                const uint32_t c = item_units(i, b);
                uint32_t tot;
                const int64_t u = ubase + wave_excl_scan(c, lane, &tot);
                if (i < nb && (T.is_byte_encoder || T.item_direct[b])) {
                    const uint32_t* units = T.item_units + T.item_units_off[b];
                    for (uint32_t k = 0; k < c; k++) {
                        if (in_lds) Sl_a.set(u + k, units[k]); else Sg_a.set(u + k, units[k]);
                    }
                } else if (c) {  // a multi-byte character without replacement
                    const int L = (b >= 0xF0u) ? 4 : (b >= 0xE0u) ? 3 : (b >= 0xC0u) ? 2 : 1;
                    uint32_t sym = SYM_UNK;
                    if (L == 1 || b >= 0xF8u || i + L > nb) {
                        raise(A.err, HUTK_E_INVALID_UTF8);
                    } else {
                        uint32_t packed = b | ((uint32_t)A.bytes[ws + i + 1] << 8);
                        if (L > 2) packed |= (uint32_t)A.bytes[ws + i + 2] << 16;
                        if (L > 3) packed |= (uint32_t)A.bytes[ws + i + 3] << 24;
                        sym = char_lookup(T, packed);
                    }
                    if (in_lds) Sl_a.set(u, sym); else Sg_a.set(u, sym);
                } else if (i == 0 && i < nb) {
                    raise(A.err, HUTK_E_INVALID_UTF8);  // a word cannot begin inside a character
                }
                ubase += tot;
            }
        } else if (T.is_byte_encoder) {
            for (int64_t i = lane; i < nb; i += 64) {
                const uint32_t sym = T.item_sym[A.bytes[ws + i]];
                if (in_lds) Sl_a.set(kp + i, sym); else Sg_a.set(kp + i, sym);
            }
        } else {
            int64_t ubase = kp;
            for (int64_t i0 = 0; i0 < nb; i0 += 64) {
                const int64_t i = i0 + lane;
                const uint32_t b = i < nb ? A.bytes[ws + i] : 0x80u;
                const bool lead = i < nb && !is_cont(b);
                const unsigned long long bal = __ballot(lead);
                if (lead) {
                    const int L = (b < 0x80u) ? 1 : (b >= 0xF0u) ? 4 : (b >= 0xE0u) ? 3 : 2;
                    uint32_t sym;
                    if (b >= 0xF8u || i + L > nb) {
                        raise(A.err, HUTK_E_INVALID_UTF8);
                        sym = SYM_UNK;
                    } else if (T.item_direct[b]) {
                        sym = T.item_sym[b];
                    } else if (L == 1) {
                        sym = SYM_UNK;
                    } else {
                        uint32_t packed = b | ((uint32_t)A.bytes[ws + i + 1] << 8);
                        if (L > 2) packed |= (uint32_t)A.bytes[ws + i + 2] << 16;
                        if (L > 3) packed |= (uint32_t)A.bytes[ws + i + 3] << 24;
                        sym = char_lookup(T, packed);
                    }
                    const int64_t u = ubase + __popcll(bal & ((1ull << lane) - 1ull));
                    if (in_lds) Sl_a.set(u, sym); else Sg_a.set(u, sym);
                } else if (i == 0 && i < nb) {
                    raise(A.err, HUTK_E_INVALID_UTF8);  // a word cannot begin inside a character
                }
                ubase += __popcll(bal);
            }
        }
        wave_wg_sync();

        // In LDS: short words by shifting the tail left after every merge (bpe_wave), longer ones by the same dead-unit
        // marks and per-chunk best keys as the words in HBM (chunks of 64 units, at most 16 of them: a merge costs three
        // chunk rescans instead of a shift of half the word, barriers and all)
        __shared__ uint32_t s_l1_all[2][2 * (LU / 64)];
        uint32_t* const s_l1 = s_l1_all[threadIdx.x >> 6];
        bool fast = false;  // (rank == symbol order: 32-bit keys, bpe_wave_fast)
        if (in_lds && T.rank_is_sym && n >= 2) fast = true;
        const int64_t left = !in_lds ? bpe_wave_big(T, Sg_a, Mg_a, Sl, Ml, n, lane)
                           : fast ? bpe_wave_fast(T, Sl, Ml, s_l1, (int)n, lane)
                           : n > EXC_SHIFT_MAX ? bpe_wave_big(T, Sl_a, Ml_a, s_l1, s_l1 + LU / 64, n, lane)
                                               : bpe_wave(T, Sl_a, Ml_a, n, lane);
        const int na = alone ? T.n_prefix_alone : 0;
        int32_t* out = W.exc_tok + gbase;
        for (int i = lane; i < na; i += 64) out[i] = T.prefix_alone_ids[i];
        for (int64_t i = lane; i < left; i += 64)
            out[na + i] = sym_to_id(T, in_lds ? Sl_a.get(i) : Sg_a.get(i));
        if (lane == 0) {
            rec.cnt = (uint32_t)(left + na);
            rec.len = (int32_t)nb;
            rec.tok_base = gbase;
            W.exc[idx] = rec;
            atomicAdd(&W.tile_count[rec.tile], rec.cnt);
        }
        wave_wg_sync();
    }
}

// The exception words in TWO launches (their kernels do nothing at all in most batches, and a launch is ~5 us):
//   k_exc_a  workgroups [0, n_medium): d_exc_lane / d_exc_medium, words of known length up to 63 bytes, one per lane;
//            the others: d_exc_ends, the lengths of the words whose end no tile saw, and the five lists by length for ...
//   k_exc_b  <true>: every workgroup walks d_exc_group_fast<2> .. <16>'s lists, then d_exc's;  <false>: workgroups
//            [0, EXB_QUAD / 2): d_exc_quad, sixteen lanes per word; the others: d_exc, a wavefront per word
// The two roles of a launch share one LDS area (a role's arrays would otherwise be allocated for every workgroup).
constexpr int EXA_MEDIUM16 = 2560, EXA_MEDIUM32 = 1280, EXA_ENDS = 4096, EXB_QUAD = 5120;
constexpr int EXB_WAVE = 4864;  // (19 per CU: what the role's 8.4 KB of LDS lets a CU hold; 4096: -6 % on words of 300-900 letters)
constexpr size_t cmax(size_t a, size_t b) { return a > b ? a : b; }
template <typename SymT>
__global__ __launch_bounds__(64) void k_exc_a(DevTables T, BatchArgs A, Workspace W, uint32_t n_medium) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[cmax(cmax(2 * MEDIUM_UNITS * 64 * sizeof(SymT), sizeof(EndsLds)),
                                                             sizeof(SymT) == 2 ? 64 * MEDIUM_ROW * 4 : 0)];
    if (W.counters[CTR_EXC] == 0) return;  // no exception word in this batch
    if (blockIdx.x < n_medium) {
        if (sizeof(SymT) == 2 && T.rank_is_sym) d_exc_lane(T, A, W, blockIdx.x, n_medium, lds);
        else d_exc_medium<SymT>(T, A, W, blockIdx.x, n_medium, lds);
    }
    else d_exc_ends(T, A, W, blockIdx.x - n_medium, gridDim.x - n_medium, lds);
}
constexpr size_t LANE_FAST_LDS = cmax(32 * (128 + 4) * 4, 16 * (256 + 4) * 4);  // d_exc_group_fast: 32 / 16 / 8 / 4 rows (the first the largest)
// k_exc_b<true> (16-bit symbols, rank == symbol order): 2304 workgroups of ONE wavefront, 16.5 KB of LDS each, nine per
// CU, all resident: each walks the four lists of d_exc_group_fast and then d_exc's (words beyond 1024 units, in the same
// LDS: up to 2046 units).  k_exc_b<false> (other vocabularies): workgroups of TWO wavefronts that never meet, 8 KB of LDS
// each (d_exc_quad, d_exc: 18 per CU) -- nothing in these roles is a workgroup barrier (wave_wg_sync).
constexpr size_t EXB_WAVE_LDS = cmax(2 * 4 * QUAD_UNITS * 4, 2 * EXC_LDS_UNITS * 4);  // per wavefront of d_exc_quad / d_exc<1024>
constexpr int EXB_FAST_WGS = 2304;
constexpr int EXB_EU = 5;  // resident wavefronts per SIMD k_exc_b<false> is compiled for
template <bool FAST>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(FAST ? 3 : EXB_EU))) void k_exc_b(DevTables T, BatchArgs A, Workspace W) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[FAST ? cmax(LANE_FAST_LDS, 2 * 2048 * 4) : 2 * EXB_WAVE_LDS];
    if (W.counters[CTR_EXC] == 0) return;
    const uint32_t wv = threadIdx.x >> 6;
    if (FAST) {
        d_exc_group_fast<2>(T, A, W, blockIdx.x, EXB_FAST_WGS, lds);
        wave_sync();
        d_exc_group_fast<4>(T, A, W, blockIdx.x, EXB_FAST_WGS, lds);
        wave_sync();
        d_exc_group_fast<8>(T, A, W, blockIdx.x, EXB_FAST_WGS, lds);
        wave_sync();
        d_exc_group_fast<16>(T, A, W, blockIdx.x, EXB_FAST_WGS, lds);
        wave_sync();
        d_exc<2048>(T, A, W, blockIdx.x, EXB_FAST_WGS, lds);
    } else if (blockIdx.x < (uint32_t)EXB_QUAD / 2) {
        d_exc_quad(T, A, W, 2 * blockIdx.x + wv, EXB_QUAD, lds + wv * EXB_WAVE_LDS);
    } else {
        d_exc<EXC_LDS_UNITS>(T, A, W, 2 * (blockIdx.x - EXB_QUAD / 2) + wv, EXB_WAVE, lds + wv * EXB_WAVE_LDS);
    }
}
