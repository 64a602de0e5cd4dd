// hutk_wordpiece.h -- WordPiece as BERT runs it (normalizers.BertNormalizer -> pre_tokenizers.BertPreTokenizer ->
// models.WordPiece of the `tokenizers` package), as the kernels of hutk_wordpiece.hip run it: the class of a character,
// the fold of one character, the character grid, the word-start decision, the hash of a candidate piece and the probe
// with its byte comparison.  Compiled for the device AND for the host (tests/cpu/wordpiece_check.cpp runs the same
// functions chunk by chunk on the CPU, under the sanitizers), so it is plain integer C++ over a view of the table blob
// (hutoken_amd/wordpiece.py builds it; include/hutoken_amd.h and that module document the format; validate_blob()
// below is what hutk_wordpiece_create refuses a blob by).
//
// The rule (include/hutoken_amd.h states it in full):
//   * clean_text drops U+0000, U+FFFD and every Cc, Cf, Co character except \t \n \r, and maps the 25 White_Space
//     characters that remain to ' ';
//   * handle_chinese_chars makes a word of every code point of 4E00-9FFF, 3400-4DBF, 20000-2A6DF, 2A700-2B73F,
//     2B740-2B81F, 2B920-2CEAF, F900-FAFF, 2F800-2FA1F.  The sixth range starts at 2B920 as in `tokenizers`, not at
//     2B820 as in Google's BERT;
//   * strip_accents is NFD (hutk_norm.h, run by the caller) and then the loss of every Mn character;
//   * lowercase maps every character on its own (one or two characters out, no final-sigma rule).
// A byte that strict UTF-8 rejects is not covered by `tokenizers`, which takes str.  It is treated as hutk_norm.h's
// decode() treats it: one character of class "word" that stays as it is.
//
// The text is read through a FLAG per byte: flag[p] != 0 where a document starts at p.  A character never reaches
// across a document start, so a sequence that a document's end cuts short is ill-formed bytes, as in hutk_norm.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "hutk_norm.h"

#define HUTK_WP_HD HUTK_NORM_HD

namespace hutk {
namespace wp {

constexpr uint32_t MAGIC = 0x43505748u, VERSION = 1u, HEADER_WORDS = 32u, BLOCK_SHIFT = 7u;
enum : int { H_MAGIC = 0, H_VERSION, H_UNIDATA, H_BYTES, H_STAGE1_OFF, H_STAGE1_N, H_CLASS_OFF, H_CLASS_BLOCKS, H_SECOND_OFF,
             H_SECOND_N, H_BLOCK_SHIFT, H_CHAR_RATIO = 16, H_BYTE_RATIO16 = 20 };
enum : int { C_WORD = 0, C_SPACE, C_PUNCT, C_CJK, C_DROPPED, C_MARK };
enum : uint32_t { F_CLEAN = 1, F_CJK = 2, F_STRIP = 4, F_LOWER = 8 };  // HUTK_WP_*
// what one fold pass does (the strip_accents setting takes two passes with NFD between them)
enum : uint32_t { M_CLEAN = 1, M_MARKS = 2, M_LOWER = 4 };
constexpr int CHUNK_BYTES = 4096, SLICE_BYTES = 16, CHUNK_SLICES = CHUNK_BYTES / SLICE_BYTES;
constexpr uint32_t N_CP = 0x110000u, STAGE1_N = N_CP >> BLOCK_SHIFT;
constexpr uint32_t ILL = 0x80000000u;  // | the byte: the "code point" of an ill-formed byte
constexpr int MAX_PREFIX = 16;
constexpr int32_t MAX_WORD_CHARS = 1 << 20;    // the largest max_input_chars_per_word a handle takes
constexpr int32_t ID_START = 1 << 30, ID_MASK = ID_START - 1;  // a matched id in the workspace: | ID_START on a word's first

struct Tables {
    const uint16_t* stage1;
    const uint32_t* cls;
    const uint32_t* second;
};

// the packed text as the kernels see it
struct Text {
    const uint8_t* bytes;
    const uint8_t* flag;  // [n + 1]
    int64_t n;
};

HUTK_WP_HD uint32_t entry(const Tables& T, uint32_t cp) {
    if (cp >= N_CP) return C_WORD;  // (an ill-formed byte)
    return T.cls[((uint32_t)T.stage1[cp >> BLOCK_SHIFT] << BLOCK_SHIFT) | (cp & ((1u << BLOCK_SHIFT) - 1u))];
}

// the class the split goes by
HUTK_WP_HD int class_of(uint32_t e, uint32_t flags) { return (int)((flags & F_CLEAN) ? e & 7u : (e >> 24) & 7u); }
HUTK_WP_HD bool is_space(int c) { return c == C_SPACE; }
// a character that is a word of its own
HUTK_WP_HD bool is_alone(int c, uint32_t flags) { return c == C_PUNCT || (c == C_CJK && (flags & F_CJK)); }

// Where the document of the character at p ends, as far as a character can reach: the next document start or the text's end.
HUTK_WP_HD int64_t reach(const Text& x, int64_t p) {
    for (int j = 1; j <= 3; j++)
        if (p + j >= x.n || x.flag[p + j]) return p + j;
    return p + 4;
}

// The character at p (a character start): its length, and its code point or ILL | byte.
HUTK_WP_HD int char_at(const Text& x, int64_t p, uint32_t* cp) {
    const int len = norm::decode(x.bytes, p, reach(x, p), cp);
    if (len) return len;
    *cp = ILL | x.bytes[p];
    return 1;
}

// Is p the start of a character?  A continuation byte is none when a well-formed character that starts up to three
// bytes before it, in the same document, covers it.
HUTK_WP_HD bool is_char_start(const Text& x, int64_t p) {
    if ((x.bytes[p] & 0xC0u) != 0x80u || x.flag[p]) return true;
    for (int j = 1; j <= 3; j++) {
        const int64_t q = p - j;
        if (q < 0) return true;
        if ((x.bytes[q] & 0xC0u) != 0x80u) {
            uint32_t cp;
            return q + norm::decode(x.bytes, q, reach(x, q), &cp) <= p;
        }
        if (x.flag[q]) return true;  // a document that starts with continuation bytes
    }
    return true;
}

// The class of the character that ends right before p (p > 0, no document starts at p).
HUTK_WP_HD int class_before(const Tables& T, const Text& x, int64_t p, uint32_t flags) {
    for (int j = 1; j <= 4; j++) {
        const int64_t q = p - j;
        if (q < 0) break;
        if ((x.bytes[q] & 0xC0u) != 0x80u) {
            uint32_t cp;
            if (q + norm::decode(x.bytes, q, reach(x, q), &cp) == p) return class_of(entry(T, cp), flags);
            break;
        }
        if (x.flag[q]) break;
    }
    return C_WORD;  // the byte before p is ill-formed
}

// Does a word start at the character start p, whose class is c?
HUTK_WP_HD bool word_starts(const Tables& T, const Text& x, int64_t p, int c, uint32_t flags) {
    if (is_space(c)) return false;
    if (p == 0 || x.flag[p] || is_alone(c, flags)) return true;
    const int b = class_before(T, x, p, flags);
    return is_space(b) || is_alone(b, flags);
}

// The fold of one character under `mode`: 0, 1 or 2 code points out.
HUTK_WP_HD int fold_char(const Tables& T, uint32_t cp, uint32_t mode, uint32_t out[2]) {
    out[0] = cp;
    if (cp & ILL) return 1;
    const uint32_t e = entry(T, cp);
    if (mode & M_CLEAN) {
        if ((e & 7u) == C_DROPPED) return 0;
        if ((e & 7u) == C_SPACE) out[0] = 0x20u;
    }
    if ((mode & M_MARKS) && (e & 7u) == C_MARK) return 0;
    if (mode & M_LOWER) {
        out[0] = (cp + ((e >> 3) & 0x1FFFFFu)) & 0x1FFFFFu;  // (the table holds the distance: blocks without a mapping are equal)
        if (e >> 27) {
            out[1] = T.second[e >> 27];
            return 2;
        }
    }
    return 1;
}

HUTK_WP_HD int utf8_len(uint32_t cp) { return (cp & ILL) || cp < 0x80u ? 1 : cp < 0x800u ? 2 : cp < 0x10000u ? 3 : 4; }
HUTK_WP_HD int utf8_put(uint8_t* d, uint32_t cp) {
    if ((cp & ILL) || cp < 0x80u) {
        d[0] = (uint8_t)cp;
        return 1;
    }
    if (cp < 0x800u) {
        d[0] = (uint8_t)(0xC0u | cp >> 6), d[1] = (uint8_t)(0x80u | (cp & 0x3Fu));
        return 2;
    }
    if (cp < 0x10000u) {
        d[0] = (uint8_t)(0xE0u | cp >> 12), d[1] = (uint8_t)(0x80u | ((cp >> 6) & 0x3Fu)), d[2] = (uint8_t)(0x80u | (cp & 0x3Fu));
        return 3;
    }
    d[0] = (uint8_t)(0xF0u | cp >> 18), d[1] = (uint8_t)(0x80u | ((cp >> 12) & 0x3Fu));
    d[2] = (uint8_t)(0x80u | ((cp >> 6) & 0x3Fu)), d[3] = (uint8_t)(0x80u | (cp & 0x3Fu));
    return 4;
}

// Bytes the characters that start in [a, b) fold to; with dst: written there as well.
HUTK_WP_HD int64_t fold_range(const Tables& T, const Text& x, int64_t a, int64_t b, uint32_t mode, uint8_t* dst) {
    int64_t out = 0;
    for (int64_t p = a; p < b; p++) {
        if (!is_char_start(x, p)) continue;
        uint32_t cp, f[2];
        (void)char_at(x, p, &cp);
        const int n = fold_char(T, cp, mode, f);
        for (int i = 0; i < n; i++) out += dst ? utf8_put(dst + out, f[i]) : utf8_len(f[i]);
    }
    return out;
}

// ---- the vocabulary: open addressing over (piece bytes, initial / continuation) ----
struct Slot {
    uint32_t hash, key, len_kind;  // key: offset of the bytes in the key blob; len_kind: length << 1 | continuation
    int32_t id;                    // < 0: the slot is empty
};
struct Vocab {
    const Slot* slots;
    const uint8_t* keys;
    uint32_t mask;
    int32_t max_len[2];  // the longest key of either kind: no longer candidate can match
};

HUTK_WP_HD uint32_t piece_hash(const uint8_t* b, int len, int kind) {
    uint32_t h = 2166136261u ^ (uint32_t)kind;
    for (int i = 0; i < len; i++) h = (h ^ b[i]) * 16777619u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    return h ^ h >> 13;
}

// The id of the piece b[0 .. len) of the kind, or -1.  A slot counts only after its bytes have been compared.
HUTK_WP_HD int32_t probe(const Vocab& V, const uint8_t* b, int len, int kind) {
    const uint32_t h = piece_hash(b, len, kind), lk = (uint32_t)len << 1 | (uint32_t)kind;
    for (uint32_t s = h & V.mask;; s = (s + 1) & V.mask) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 raw = *reinterpret_cast<const uint4*>(V.slots + s);
        const Slot e{raw.x, raw.y, raw.z, (int32_t)raw.w};
#else
        const Slot e = V.slots[s];
#endif
        if (e.id < 0) return -1;
        if (e.hash != h || e.len_kind != lk) continue;
        const uint8_t* k = V.keys + e.key;
        int i = 0;
        while (i < len && k[i] == b[i]) i++;
        if (i == len) return e.id;
    }
}

inline uint32_t blob_word(const uint8_t* blob, size_t at) {
    return (uint32_t)blob[at] | (uint32_t)blob[at + 1] << 8 | (uint32_t)blob[at + 2] << 16 | (uint32_t)blob[at + 3] << 24;
}

// Every offset and index of the blob is checked before anything reads through them.
inline bool validate_blob(const uint8_t* blob, int64_t n, uint32_t (&h)[HEADER_WORDS], std::string* why) {
    auto fail = [&](const char* m) {
        if (why) *why = m;
        return false;
    };
    if (!blob || n < (int64_t)(4 * HEADER_WORDS) || (n & 3)) return fail("the blob is shorter than its header or no multiple of 4 bytes");
    for (uint32_t i = 0; i < HEADER_WORDS; i++) h[i] = blob_word(blob, 4 * i);
    if (h[H_MAGIC] != MAGIC || h[H_VERSION] != VERSION) return fail("wrong magic or version");
    if ((int64_t)h[H_BYTES] != n || h[H_BLOCK_SHIFT] != BLOCK_SHIFT) return fail("wrong size or block shift");
    if (h[H_STAGE1_N] != STAGE1_N || h[H_CLASS_BLOCKS] < 1 || h[H_CLASS_BLOCKS] > 65535 || h[H_SECOND_N] < 1 || h[H_SECOND_N] > 32)
        return fail("wrong section sizes");
    const uint64_t sect[3][2] = {{h[H_STAGE1_OFF], 2ull * h[H_STAGE1_N]},
                                 {h[H_CLASS_OFF], (4ull * h[H_CLASS_BLOCKS]) << BLOCK_SHIFT},
                                 {h[H_SECOND_OFF], 4ull * h[H_SECOND_N]}};
    for (auto& s : sect)
        if ((s[0] & 3) || s[0] < 4 * HEADER_WORDS || s[0] + s[1] > (uint64_t)n) return fail("a section lies outside the blob");
    for (uint32_t i = 0; i < STAGE1_N; i++) {
        const size_t at = h[H_STAGE1_OFF] + 2 * (size_t)i;
        if (((uint32_t)blob[at] | (uint32_t)blob[at + 1] << 8) >= h[H_CLASS_BLOCKS])
            return fail("a stage-one entry names a block the blob does not hold");
    }
    for (uint32_t cp = 0; cp < N_CP; cp++) {  // the word of every code point, through stage one (checked above)
        const size_t s1 = h[H_STAGE1_OFF] + 2 * (size_t)(cp >> BLOCK_SHIFT);
        const uint32_t b = (uint32_t)blob[s1] | (uint32_t)blob[s1 + 1] << 8;
        const uint32_t w = blob_word(blob, h[H_CLASS_OFF] + 4 * (size_t)((b << BLOCK_SHIFT) | (cp & ((1u << BLOCK_SHIFT) - 1u))));
        if ((w & 7u) > C_MARK || ((w >> 24) & 7u) > C_MARK || ((cp + ((w >> 3) & 0x1FFFFFu)) & 0x1FFFFFu) >= N_CP || (w >> 27) >= h[H_SECOND_N])
            return fail("a class word holds a class, a code point or an index out of range");
    }
    for (uint32_t i = 0; i < h[H_SECOND_N]; i++)
        if (blob_word(blob, h[H_SECOND_OFF] + 4 * (size_t)i) >= N_CP) return fail("a second character is no code point");
    for (int s = 0; s < 4; s++)
        if (h[H_CHAR_RATIO + s] < 1 || h[H_CHAR_RATIO + s] > 4 || h[H_BYTE_RATIO16 + s] < 16 || h[H_BYTE_RATIO16 + s] > 64)
            return fail("a ratio out of range");
    return true;
}

// blob: where the sections are read from (the device copy for the kernels)
inline Tables tables_of(const uint8_t* blob, const uint32_t (&h)[HEADER_WORDS]) {
    Tables T;
    T.stage1 = reinterpret_cast<const uint16_t*>(blob + h[H_STAGE1_OFF]);
    T.cls = reinterpret_cast<const uint32_t*>(blob + h[H_CLASS_OFF]);
    T.second = reinterpret_cast<const uint32_t*>(blob + h[H_SECOND_OFF]);
    return T;
}

// The table of a vocabulary, built on the host (hutk_wordpiece_create uploads it once).  Line i of the n lines is
// bytes[offs[i] .. offs[i + 1]) and its id is i; of two equal lines the later id wins; a line of more than
// 4 * max_chars bytes can never match and is kept for its id alone.  Every line is a candidate for a word's first
// piece; one that starts with the prefix and goes on is, without the prefix, a candidate for the later ones as well.
// Returns 0, or 1 (a value the rule refuses) or 2 (arguments that make no sense) with the reason in *why.
struct VocabHost {
    std::vector<Slot> slots;
    std::vector<uint8_t> keys;
    int32_t max_len[2] = {0, 0};
    int32_t unk = -1;
    Vocab view(const Slot* s, const uint8_t* k) const { return Vocab{s, k, (uint32_t)(slots.size() - 1), {max_len[0], max_len[1]}}; }
};
inline int build_vocab(const uint8_t* bytes, const int64_t* offs, int64_t n, const std::string& unk, const std::string& prefix,
                       int32_t max_chars, VocabHost& out, std::string* why) {
    if (n < 1 || n >= ID_START) return *why = "the vocabulary must hold 1 .. 2^30 - 1 lines", 1;
    if (prefix.size() > (size_t)MAX_PREFIX) return *why = "the prefix is longer than 16 bytes", 1;
    if (max_chars < 0 || max_chars > MAX_WORD_CHARS) return *why = "max_input_chars_per_word must lie in 0 .. 2^20", 1;
    if (offs[0] != 0) return *why = "vocab_offsets must start at 0", 2;
    const int64_t longest = 4 * (int64_t)max_chars;
    std::unordered_map<std::string, int32_t> ids[2];
    for (int64_t i = 0; i < n; i++) {
        const int64_t a = offs[i], b = offs[i + 1];
        if (b < a) return *why = "vocab_offsets must not fall", 2;
        if (b == a) return *why = "line " + std::to_string(i) + " of the vocabulary is empty", 1;
        const std::string line((const char*)bytes + a, (size_t)(b - a));
        if (line == unk) out.unk = (int32_t)i;
        if (b - a <= longest) ids[0][line] = (int32_t)i;
        if (line.size() > prefix.size() && line.compare(0, prefix.size(), prefix) == 0 && (int64_t)(line.size() - prefix.size()) <= longest)
            ids[1][line.substr(prefix.size())] = (int32_t)i;
    }
    if (out.unk < 0) return *why = "unk_token \"" + unk + "\" is not in the vocabulary", 1;
    // sized for the L2, not for HBM: a load of at most a half, 16 bytes a slot
    size_t slots = 16;
    while (slots < 2 * (ids[0].size() + ids[1].size()) + 2) slots *= 2;
    out.slots.assign(slots, Slot{0, 0, 0, -1});
    for (int kind = 0; kind < 2; kind++) {
        std::vector<std::pair<std::string, int32_t>> sorted(ids[kind].begin(), ids[kind].end());
        std::sort(sorted.begin(), sorted.end());  // (the layout does not depend on the hash map's order)
        for (auto& kv : sorted) {
            const uint32_t hsh = piece_hash((const uint8_t*)kv.first.data(), (int)kv.first.size(), kind);
            size_t s = hsh & (slots - 1);
            while (out.slots[s].id >= 0) s = (s + 1) & (slots - 1);
            out.slots[s] = Slot{hsh, (uint32_t)out.keys.size(), (uint32_t)kv.first.size() << 1 | (uint32_t)kind, kv.second};
            out.keys.insert(out.keys.end(), kv.first.begin(), kv.first.end());
            out.max_len[kind] = std::max(out.max_len[kind], (int32_t)kv.first.size());
        }
    }
    if (out.keys.size() > 0xFFFFFFF0u) return *why = "the vocabulary is too large", 1;
    return 0;
}

}  // namespace wp
}  // namespace hutk
