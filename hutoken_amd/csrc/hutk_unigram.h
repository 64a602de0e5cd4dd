// hutk_unigram.h -- Unigram encoding as `tokenizers` runs it (models.Unigram with byte_fallback off behind a Metaspace
// pre-tokenizer), as the kernels of hutk_unigram.hip run it: the fold of one source byte, the word rule, the vocabulary
// table with its probe, the update rule of the best path and the backtrack.  Compiled for the device AND for the host
// (tests/cpu/unigram_check.cpp runs the same functions chunk by chunk on the CPU, under the sanitizers;
// hutk_unigram_create builds the table with build_vocab), so it is plain C++ with IEEE f64 additions and no table blob.
//
// The rule (include/hutoken_amd.h states it in full):
//   * the FOLD writes the text the words are cut from.  U+2581 (bytes E2 96 81) is stored as the one byte 0x20 in the
//     text and in the keys: a space, a literal U+2581 and the prepended prefix all become 0x20.  Under F_COLLAPSE a
//     U+0020 behind a U+0020 is dropped first.  Without F_WS_SPLIT a 0x20 is put in front of a document (F_PREPEND)
//     unless it starts with a space or a U+2581; with F_WS_SPLIT every White_Space character is dropped and every
//     maximal run of other characters gets a 0x20 in front unless it starts with a U+2581.  A source byte becomes at
//     most two bytes and the folded text holds at most n_bytes + n_docs;
//   * a WORD starts at every 0x20 of the folded text and at a document's first folded byte, and ends at the next;
//   * the PIECES of a word are the best path of encode_optimized: see relax() and viterbi_word().
// A byte that strict UTF-8 rejects is a character of one byte (hutk_norm.h's decode); no key matches it.
//
// The source is read through a FLAG per byte: flag[p] != 0 where a document starts at p; so is the folded text.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "hutk_norm.h"

#define HUTK_UG_HD HUTK_NORM_HD

namespace hutk {
namespace ug {

constexpr int CHUNK_BYTES = 4096, SLICE_BYTES = 16, CHUNK_SLICES = CHUNK_BYTES / SLICE_BYTES;
constexpr int MAX_PIECE = 256;  // the longest piece a handle takes, in folded bytes
enum : uint32_t { F_PREPEND = 1, F_WS_SPLIT = 2, F_COLLAPSE = 4 };  // HUTK_UG_*
constexpr int32_t ID_START = 1 << 30, ID_MASK = ID_START - 1;  // an id in the workspace: | ID_START on a word's first
constexpr uint8_t SP = 0x20u;

struct Text {
    const uint8_t* bytes;
    const uint8_t* flag;  // [n + 1]
    int64_t n;
};

// ---- the fold ----
// a literal U+2581 at p, inside one document
HUTK_UG_HD bool meta_at(const Text& x, int64_t p) {
    return p + 2 < x.n && x.bytes[p] == 0xE2u && x.bytes[p + 1] == 0x96u && x.bytes[p + 2] == 0x81u && !x.flag[p + 1] && !x.flag[p + 2];
}
// is p the second or third byte of one
HUTK_UG_HD bool meta_tail(const Text& x, int64_t p) {
    const uint8_t b = x.bytes[p];
    return (b == 0x96u && p >= 1 && meta_at(x, p - 1)) || (b == 0x81u && p >= 2 && meta_at(x, p - 2));
}

// The length of the White_Space character (Rust's char::is_whitespace) that starts at p, 0: none.  Its lead byte is no
// continuation byte, so whenever these bytes lie in one document they are a well-formed character.
HUTK_UG_HD int ws_at(const Text& x, int64_t p) {
    const uint8_t b0 = x.bytes[p];
    if (b0 < 0x80u) return (b0 >= 0x09u && b0 <= 0x0Du) || b0 == SP ? 1 : 0;
    if (b0 != 0xC2u && (b0 < 0xE1u || b0 > 0xE3u)) return 0;
    if (p + 1 >= x.n || x.flag[p + 1]) return 0;
    const uint8_t b1 = x.bytes[p + 1];
    if (b0 == 0xC2u) return b1 == 0x85u || b1 == 0xA0u ? 2 : 0;
    if (p + 2 >= x.n || x.flag[p + 2]) return 0;
    const uint8_t b2 = x.bytes[p + 2];
    if (b0 == 0xE1u) return b1 == 0x9Au && b2 == 0x80u ? 3 : 0;
    if (b0 == 0xE3u) return b1 == 0x80u && b2 == 0x80u ? 3 : 0;
    if (b1 == 0x80u) return (b2 >= 0x80u && b2 <= 0x8Au) || b2 == 0xA8u || b2 == 0xA9u || b2 == 0xAFu ? 3 : 0;
    return b1 == 0x81u && b2 == 0x9Fu ? 3 : 0;
}
// byte p belongs to a White_Space character
HUTK_UG_HD bool ws_covers(const Text& x, int64_t p) {
    return ws_at(x, p) > 0 || (p >= 1 && ws_at(x, p - 1) >= 2) || (p >= 2 && ws_at(x, p - 2) >= 3);
}
// a White_Space character of p's document ends right in front of p
HUTK_UG_HD bool ws_before(const Text& x, int64_t p) {
    if (p < 1 || x.flag[p]) return false;
    return ws_at(x, p - 1) == 1 || (p >= 2 && ws_at(x, p - 2) == 2) || (p >= 3 && ws_at(x, p - 3) == 3);
}

// What source byte p folds to: 0, 1 or 2 bytes.
HUTK_UG_HD int fold_byte(const Text& x, int64_t p, uint32_t flags, uint8_t out[2]) {
    const uint8_t b = x.bytes[p];
    if (meta_tail(x, p)) return 0;
    const bool meta = meta_at(x, p);
    int n = 0;
    if (flags & F_WS_SPLIT) {
        if (ws_covers(x, p)) return 0;
        if ((x.flag[p] || ws_before(x, p)) && !meta) out[n++] = SP;
    } else {
        if ((flags & F_COLLAPSE) && b == SP && p > 0 && !x.flag[p] && x.bytes[p - 1] == SP) return 0;
        if (x.flag[p] && (flags & F_PREPEND) && b != SP && !meta) out[n++] = SP;
    }
    out[n++] = meta ? SP : b;
    return n;
}

// Bytes the source bytes [a, b) fold to; with dst: written there as well.
HUTK_UG_HD int64_t fold_range(const Text& x, int64_t a, int64_t b, uint32_t flags, uint8_t* dst) {
    int64_t out = 0;
    for (int64_t p = a; p < b; p++) {
        uint8_t f[2];
        const int n = fold_byte(x, p, flags, f);
        for (int i = 0; i < n; i++) {
            if (dst) dst[out] = f[i];
            out++;
        }
    }
    return out;
}

// ---- words of the folded text ----
HUTK_UG_HD bool word_starts(const Text& f, int64_t q) { return q < f.n && (f.bytes[q] == SP || f.flag[q]); }
HUTK_UG_HD bool word_ends(const Text& f, int64_t q) { return q >= f.n || f.bytes[q] == SP || f.flag[q]; }

// ---- the vocabulary: open addressing over the folded piece bytes, and the scores by id ----
struct Slot {
    uint32_t hash, key, len;  // key: offset of the bytes in the key blob
    int32_t id;               // < 0: the slot is empty
};
struct Back {  // the backpointer of a position: the piece that ends there on the best path so far
    int32_t id, len;
};
struct Vocab {
    const Slot* slots;
    const uint8_t* keys;
    const double* scores;   // [n_pieces]
    const uint64_t* lens;   // [256] by a key's first byte: bit min(len, 63) is set when a key of that length exists
    uint32_t mask;
    int32_t max_len;        // the longest key: no longer candidate can match
    int32_t unk;
    double unk_score;       // min(scores) - 10
};

constexpr uint32_t HASH_INIT = 2166136261u;
HUTK_UG_HD uint32_t hash_step(uint32_t h, uint32_t b) { return (h ^ b) * 16777619u; }
HUTK_UG_HD uint32_t hash_end(uint32_t h) {
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    return h ^ h >> 13;
}
inline uint32_t piece_hash(const uint8_t* b, int len) {
    uint32_t h = HASH_INIT;
    for (int i = 0; i < len; i++) h = hash_step(h, b[i]);
    return hash_end(h);
}
HUTK_UG_HD bool has_len(uint64_t lens, int len) { return (lens >> (len < 63 ? len : 63)) & 1u; }
// no key with this first byte is longer
HUTK_UG_HD int top_len(uint64_t lens, int max_len) {
    if (!lens) return 0;
    if (lens >> 63) return max_len;
    int t = 62;
    while (!((lens >> t) & 1u)) t--;
    return t;
}

// The id of the piece b[0 .. len) whose hash is h, or -1.  A slot counts only after its bytes have been compared.
HUTK_UG_HD int32_t find(const Vocab& V, uint32_t h, const uint8_t* b, int len) {
    for (uint32_t s = h & V.mask;; s = (s + 1) & V.mask) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 raw = *reinterpret_cast<const uint4*>(V.slots + s);
        const Slot e{raw.x, raw.y, raw.z, (int32_t)raw.w};
#else
        const Slot e = V.slots[s];
#endif
        if (e.id < 0) return -1;
        if (e.hash != h || e.len != (uint32_t)len) continue;
        const uint8_t* k = V.keys + e.key;
        int i = 0;
        while (i < len && k[i] == b[i]) i++;
        if (i == len) return e.id;
    }
}

// ---- the best path ----
// best[] is a ring of R >= max_len + 1 positions (R a power of two) that holds NaN where a position holds nothing yet.
// A candidate replaces what the position holds if it holds nothing or if the candidate is strictly greater: candidates
// arrive by rising start, so among equal scores the smallest start -- the longest last piece -- stays.
HUTK_UG_HD bool replaces(double cand, double cur) { return cur != cur || cand > cur; }

// The character that starts at q of a word that ends at end: its length (an ill-formed byte: 1).
HUTK_UG_HD int char_len(const uint8_t* bytes, int64_t q, int64_t end) {
    uint32_t cp;
    const int len = norm::decode(bytes, q, end, &cp);
    return len ? len : 1;
}

// The walk back over the word [ws, ws + n): every piece's id goes to its first byte, | ID_START on the word's first.
// An unknown id whose predecessor in the word is unknown is dropped (a line that sits at the unknown id counts as unknown).
HUTK_UG_HD void backtrack(const Back* bp, int32_t unk, int64_t ws, int64_t n, int32_t* tmp) {
    int64_t later_unk = -1;
    for (int64_t e = n; e > 0;) {
        const Back b = bp[ws + e];
        const int64_t st = e - b.len;
        const bool is_unk = b.id == unk;
        if (is_unk && later_unk >= 0) tmp[ws + later_unk] = -1;
        tmp[ws + st] = b.id | (st == 0 ? ID_START : 0);
        later_unk = is_unk ? st : -1;
        e = st;
    }
}

inline int ring_size(int max_len) {
    int r = 16;
    while (r < max_len + 1) r *= 2;
    return r;
}

// The word that starts at ws, in the plain form: one start after the other, every length of a start in turn.
// ring: R entries, all NaN on entry and on return.  bp: one entry per folded byte and one more.
inline void viterbi_word(const Vocab& V, const Text& f, int64_t ws, double* ring, int R, Back* bp, int32_t* tmp) {
    int64_t n = 1;
    while (!word_ends(f, ws + n)) n++;
    const uint8_t* w = f.bytes + ws;
    const double nan = std::nan("");
    auto relax = [&](int64_t e, double cand, int32_t id, int len) {
        double& cur = ring[e & (R - 1)];
        if (replaces(cand, cur)) cur = cand, bp[ws + e] = Back{id, len};
    };
    ring[0] = 0.0;
    for (int64_t s = 0; s < n;) {
        const double here = ring[s & (R - 1)];
        ring[s & (R - 1)] = nan;
        const int m = char_len(f.bytes, ws + s, ws + n);
        const uint64_t lens = V.lens[w[s]];
        const int64_t top = std::min<int64_t>(top_len(lens, V.max_len), n - s);
        bool single = false;
        uint32_t h = HASH_INIT;
        for (int len = 1; len <= top; len++) {
            h = hash_step(h, w[s + len - 1]);
            if (!has_len(lens, len)) continue;
            const int32_t id = find(V, hash_end(h), w + s, len);
            if (id < 0) continue;
            relax(s + len, V.scores[id] + here, id, len);
            single = single || len == m;
        }
        if (!single) relax(s + m, V.unk_score + here, V.unk, m);
        s += m;
    }
    ring[n & (R - 1)] = nan;
    backtrack(bp, V.unk, ws, n, tmp);
}

// a well-formed UTF-8 string
inline bool well_formed(const std::string& s) {
    for (size_t p = 0; p < s.size();) {
        uint32_t cp;
        const int len = norm::decode((const uint8_t*)s.data(), (int64_t)p, (int64_t)s.size(), &cp);
        if (!len) return false;
        p += (size_t)len;
    }
    return true;
}

// The table of a vocabulary, built on the host (hutk_unigram_create uploads it once).  Piece i of the n is
// bytes[offs[i] .. offs[i + 1]) with scores[i]; of two equal pieces the later id, with its own score, is the one found.
// A key is stored folded: a leading U+2581 as 0x20.  A piece that holds a real space, a U+2581 anywhere but at its
// start, or ill-formed UTF-8 can never match and is kept for its id alone.
// Returns 0, or 1 (a value the rule refuses) or 2 (arguments that make no sense) with the reason in *why.
struct VocabHost {
    std::vector<Slot> slots;
    std::vector<uint8_t> keys;
    std::vector<uint64_t> lens;
    int32_t max_len = 0;
    double unk_score = 0.0;
    Vocab view(const Slot* s, const uint8_t* k, const double* scores, const uint64_t* l, int32_t unk) const {
        return Vocab{s, k, scores, l, (uint32_t)(slots.size() - 1), max_len, unk, unk_score};
    }
};
inline int build_vocab(const uint8_t* bytes, const int64_t* offs, const double* scores, int64_t n, int64_t unk_id, VocabHost& out,
                       std::string* why) {
    if (n < 1 || n >= ID_START) return *why = "the vocabulary must hold 1 .. 2^30 - 1 pieces", 1;
    if (unk_id < 0 || unk_id >= n) return *why = "unk_id is no id of the vocabulary", 1;
    if (offs[0] != 0) return *why = "piece_offsets must start at 0", 2;
    const std::string meta = "\xE2\x96\x81";
    std::unordered_map<std::string, int32_t> ids;
    double low = 0.0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t a = offs[i], b = offs[i + 1];
        if (b < a) return *why = "piece_offsets must not fall", 2;
        if (b == a) return *why = "piece " + std::to_string(i) + " of the vocabulary is empty", 1;
        if (!std::isfinite(scores[i])) return *why = "the score of piece " + std::to_string(i) + " is not finite", 1;
        low = i == 0 ? scores[i] : std::min(low, scores[i]);
        std::string key((const char*)bytes + a, (size_t)(b - a));
        bool can_match = well_formed(key) && key.find(' ') == std::string::npos;
        size_t metas = 0;
        for (size_t at = key.find(meta); at != std::string::npos; at = key.find(meta, at + 3)) metas++;
        if (key.size() - 2 * metas > (size_t)MAX_PIECE)
            return *why = "piece " + std::to_string(i) + " is longer than " + std::to_string(MAX_PIECE) + " bytes", 1;
        if (metas > 1 || (metas == 1 && key.compare(0, 3, meta) != 0)) can_match = false;
        if (!can_match) continue;
        if (metas) key = " " + key.substr(3);
        ids[key] = (int32_t)i;
    }
    out.unk_score = low - 10.0;
    size_t slots = 16;  // a load of at most a half, 16 bytes a slot
    while (slots < 2 * ids.size() + 2) slots *= 2;
    out.slots.assign(slots, Slot{0, 0, 0, -1});
    out.lens.assign(256, 0);
    std::vector<std::pair<std::string, int32_t>> sorted(ids.begin(), ids.end());
    std::sort(sorted.begin(), sorted.end());  // (the layout does not depend on the hash map's order)
    for (auto& kv : sorted) {
        const int len = (int)kv.first.size();
        const uint32_t hsh = piece_hash((const uint8_t*)kv.first.data(), len);
        size_t s = hsh & (slots - 1);
        while (out.slots[s].id >= 0) s = (s + 1) & (slots - 1);
        out.slots[s] = Slot{hsh, (uint32_t)out.keys.size(), (uint32_t)len, kv.second};
        out.keys.insert(out.keys.end(), kv.first.begin(), kv.first.end());
        out.max_len = std::max(out.max_len, (int32_t)len);
        out.lens[(uint8_t)kv.first[0]] |= 1ull << (len < 63 ? len : 63);
    }
    if (out.keys.size() > 0xFFFFFFF0u) return *why = "the vocabulary is too large", 1;
    return 0;
}

}  // namespace ug
}  // namespace hutk
