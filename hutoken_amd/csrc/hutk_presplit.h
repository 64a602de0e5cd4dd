// hutk_presplit.h -- the word split of the GPT-2, cl100k (Llama 3) and Qwen2 pre-tokenisers as a rule over character
// classes, as the kernels of hutk_presplit.hip run it.  Compiled for the device AND for the host
// (tests/cpu/presplit_check.cpp runs the same classification, carries and decisions on the CPU, under the sanitizers), so
// it is plain integer C++ over a view of the table blob (hutoken_amd/pretokenize.py builds it; include/hutoken_amd.h and
// that module document the format; validate_blob() below is what hutk_pretokenizer_create refuses a blob by).
//
// Contract: bit p of the output is set where regex.findall(pattern, document) starts a match,
//   gpt2    's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
//   cl100k  (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
//   qwen2   cl100k with \p{N} in place of \p{N}{1,3}
// over d.decode("utf-8", "surrogateescape"): a byte that strict UTF-8 rejects (hutk_norm.h, decode()) is one character
// that is neither letter, number nor whitespace.  Documents are independent.
//
// The rule.  Every character gets a CODE (class, which letter of a contraction it can be); whether a word starts at a
// character is a function of the codes of at most four characters before and two behind it, plus two values that are
// not local and are carried along (fwd_step, bwd_step):
//   forward   how many digits of the run the character stands in came before it, mod 3 (\p{N}{1,3}); and whether it
//             follows an "other" run with nothing but newlines in between (the [\r\n]* tail swallows those);
//   backward  whether a newline lies ahead in the whitespace run the character stands in (\s*[\r\n]+ runs to the LAST one).
// Both are finite-state, so a slice, a chunk and any stretch of text is summarised by a map over the states (five forward,
// two backward) and maps compose: slices are scanned inside a chunk, chunks by one workgroup in between two passes.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "hutk_norm.h"  // the UTF-8 rule: norm::decode

#define HUTK_PS_HD HUTK_NORM_HD

namespace hutk {
namespace presplit {

enum : int { PRESET_GPT2 = 0, PRESET_CL100K = 1, PRESET_QWEN2 = 2, N_PRESETS = 3 };
constexpr int CHUNK_BYTES = 4096, SLICE_BYTES = 16;
// a chunk is staged with BACK bytes in front and AHEAD bytes behind it; characters are classified from CLS_HALO bytes in
// front to CLS_HALO bytes behind (a decision reads four characters back, the contraction ones of at most two bytes, and
// two ahead; classifying a byte reads three bytes either way)
constexpr int BACK = 32, AHEAD = 32, CLS_HALO = 16;

constexpr uint32_t MAGIC = 0x4B545048u /* "HPTK" */, VERSION = 1u, HEADER_WORDS = 16u, BLOCK_SHIFT = 7u;
enum : int { H_MAGIC = 0, H_VERSION, H_UNIDATA, H_BYTES, H_STAGE1_OFF, H_STAGE1_N, H_BLOCKS_OFF, H_BLOCKS_N, H_BLOCK_SHIFT };
constexpr uint32_t N_CP = 0x110000u, STAGE1_N = N_CP >> BLOCK_SHIFT, BLOCK_WORDS = (1u << BLOCK_SHIFT) / 16u;
enum : uint32_t { T_OTHER = 0, T_LETTER = 1, T_NUMBER = 2, T_SPACE = 3 };  // the two bits of a code point

struct Tables {
    const uint16_t* stage1;  // [STAGE1_N] block of code point c: stage1[c >> 7]
    const uint32_t* blocks;  // BLOCK_WORDS words a block, two bits a code point
};

// ---- codes: bits 0..2 the class, bits 3..6 which contraction letter, bit 7: that letter as the lower-case ASCII one ----
enum : uint32_t { C_NONE = 0, C_L = 1, C_N = 2, C_O = 3, C_WS = 4, C_SP = 5, C_NL = 6, C_APOS = 7 };
enum : uint32_t { K_S = 1, K_T, K_R, K_E, K_V, K_M, K_LL, K_D };
HUTK_PS_HD uint32_t cls_of(uint32_t code) { return code & 7u; }
HUTK_PS_HD uint32_t letter_of(uint32_t code) { return (code >> 3) & 15u; }
HUTK_PS_HD bool is_ws(uint32_t cls) { return cls == C_WS || cls == C_SP || cls == C_NL; }
HUTK_PS_HD bool is_other(uint32_t cls) { return cls == C_O || cls == C_APOS; }

// ASCII: a 128-entry table of two bits, held in four constants
constexpr uint64_t ascii_row(int row) {
    uint64_t w = 0;
    for (int i = 0; i < 32; i++) {
        const int c = row * 32 + i;
        const uint64_t t = (c >= 9 && c <= 13) || c == 32 ? T_SPACE : (c >= '0' && c <= '9') ? T_NUMBER
                           : ((c | 32) >= 'a' && (c | 32) <= 'z') ? T_LETTER : T_OTHER;
        w |= t << (2 * i);
    }
    return w;
}
constexpr uint64_t ASCII0 = ascii_row(0), ASCII1 = ascii_row(1), ASCII2 = ascii_row(2), ASCII3 = ascii_row(3);

HUTK_PS_HD uint32_t ascii_code(uint32_t b) {
    const uint64_t row = b < 32u ? ASCII0 : b < 64u ? ASCII1 : b < 96u ? ASCII2 : ASCII3;
    const uint32_t t = (uint32_t)(row >> (2u * (b & 31u))) & 3u;
    if (t == T_NUMBER) return C_N;
    if (t == T_SPACE) return b == 32u ? C_SP : (b == 10u || b == 13u) ? C_NL : C_WS;
    if (t == T_OTHER) return b == 0x27u ? C_APOS : C_O;
    const uint32_t lo = b | 32u;
    const uint32_t k = lo == 's' ? K_S : lo == 't' ? K_T : lo == 'r' ? K_R : lo == 'e' ? K_E : lo == 'v' ? K_V
                       : lo == 'm' ? K_M : lo == 'l' ? K_LL : lo == 'd' ? K_D : 0u;
    return C_L | k << 3 | (k && b == lo ? 0x80u : 0u);
}

HUTK_PS_HD uint32_t cp_code(const Tables& T, uint32_t cp) {
    if (cp < 0x80u) return ascii_code(cp);
    const uint32_t w = T.blocks[(uint32_t)T.stage1[cp >> BLOCK_SHIFT] * BLOCK_WORDS + ((cp & ((1u << BLOCK_SHIFT) - 1u)) >> 4)];
    const uint32_t t = (w >> (2u * (cp & 15u))) & 3u;
    if (t == T_LETTER) return cp == 0x17Fu ? C_L | K_S << 3 : C_L;  // (?i:s) also matches U+017F; no other letter has such a partner
    return t == T_NUMBER ? C_N : t == T_SPACE ? C_WS : C_O;
}

// ---- the staged window of one chunk: index i is byte w0 + i of the batch ----
struct Win {
    const uint8_t* raw;   // the bytes, zero outside the batch
    uint8_t* code;        // the codes; 0: no character starts here
    const uint32_t* doc;  // bit i: a document starts at (or the batch ends at) byte w0 + i
};
HUTK_PS_HD bool docbit(const Win& W, int i) { return (W.doc[i >> 5] >> (i & 31)) & 1u; }

// the code of the byte at i (inside the batch): 0 when it continues a well-formed character
HUTK_PS_HD uint32_t classify_byte(const Tables& T, const Win& W, int i) {
    const uint32_t b = W.raw[i];
    if (b < 0x80u) return ascii_code(b);
    if ((b & 0xC0u) == 0x80u) {
        for (int j = 1; j <= 3; j++) {  // the nearest byte in front that is no continuation byte decides (norm::spill)
            if (docbit(W, i - j + 1)) break;
            const uint32_t bq = W.raw[i - j];
            if ((bq & 0xC0u) == 0x80u) continue;
            int room = 4;
            for (int k = 1; k <= 3; k++)
                if (docbit(W, i - j + k)) { room = k; break; }
            uint32_t cp;
            if (i - j + norm::decode(W.raw, i - j, i - j + room, &cp) > i) return C_NONE;
            break;
        }
        return C_O;
    }
    int room = 4;
    for (int k = 1; k <= 3; k++)
        if (docbit(W, i + k)) { room = k; break; }
    uint32_t cp;
    return norm::decode(W.raw, i, i + room, &cp) ? cp_code(T, cp) : C_O;
}

// index of the character in front of the one at i, -1: i starts its document
HUTK_PS_HD int prev_char(const Win& W, int i) {
    if (docbit(W, i)) return -1;
    for (int j = 1; j <= 4; j++)
        if (W.code[i - j]) return i - j;
    return -1;
}
// ... and of the one behind it, -1: its document ends there
HUTK_PS_HD int next_char(const Win& W, int i) {
    for (int j = 1; j <= 4; j++) {
        if (docbit(W, i + j)) return -1;
        if (W.code[i + j]) return i + j;
    }
    return -1;
}
HUTK_PS_HD uint32_t cls_at(const Win& W, int i) { return i < 0 ? (uint32_t)C_NONE : cls_of(W.code[i]); }

// the apostrophe at q begins a match (it is not inside an "other" run) and a contraction follows: its letters, else 0
HUTK_PS_HD int contraction_at(const Win& W, int preset, int q) {
    const uint32_t pc = cls_at(W, prev_char(W, q));
    if (is_other(pc) || pc == C_SP) return 0;
    const int n1 = next_char(W, q);
    if (n1 < 0) return 0;
    const uint32_t c1 = W.code[n1], k1 = letter_of(c1);
    if (cls_of(c1) != C_L || !k1 || (preset == PRESET_GPT2 && !(c1 & 0x80u))) return 0;
    if (k1 == K_S || k1 == K_T || k1 == K_M || k1 == K_D) return 1;
    const int n2 = next_char(W, n1);
    if (n2 < 0) return 0;
    const uint32_t c2 = W.code[n2], k2 = letter_of(c2);
    if (cls_of(c2) != C_L || !k2 || (preset == PRESET_GPT2 && !(c2 & 0x80u))) return 0;
    return ((k1 == K_R || k1 == K_V) && k2 == K_E) || (k1 == K_LL && k2 == K_LL) ? 2 : 0;
}

enum : int { ROLE_NONE = 0, ROLE_LETTER = 1, ROLE_AFTER = 2 };
// the character at i is a letter of a contraction (no word starts there) or the first one behind it (one does)
HUTK_PS_HD int contraction_role(const Win& W, int preset, int i) {
    const int p1 = prev_char(W, i);
    if (p1 < 0) return ROLE_NONE;
    if (cls_of(W.code[p1]) == C_APOS) return contraction_at(W, preset, p1) ? ROLE_LETTER : ROLE_NONE;
    if (cls_of(W.code[p1]) != C_L || !letter_of(W.code[p1])) return ROLE_NONE;
    const int p2 = prev_char(W, p1);
    if (p2 < 0) return ROLE_NONE;
    if (cls_of(W.code[p2]) == C_APOS) {
        const int n = contraction_at(W, preset, p2);
        return n == 2 ? ROLE_LETTER : n == 1 ? ROLE_AFTER : ROLE_NONE;
    }
    if (cls_of(W.code[p2]) != C_L || !letter_of(W.code[p2])) return ROLE_NONE;
    const int p3 = prev_char(W, p2);
    if (p3 < 0 || cls_of(W.code[p3]) != C_APOS) return ROLE_NONE;
    return contraction_at(W, preset, p3) == 2 ? ROLE_AFTER : ROLE_NONE;
}

// ---- the carried values ----
// forward states: 0 nothing; 1, 2, 3: the last character was the (3k+1)th, (3k+2)th, (3k+3)th digit of its run; 4: it was
// an "other" character or a newline that such a character's match swallowed
enum : uint32_t { F_NONE = 0, F_D1 = 1, F_D2 = 2, F_D3 = 3, F_SWALLOW = 4, F_STATES = 5 };
HUTK_PS_HD uint32_t fwd_step(uint32_t s, uint32_t cls) {
    if (cls == C_N) return s == F_D1 ? F_D2 : s == F_D2 ? F_D3 : F_D1;
    if (is_other(cls)) return F_SWALLOW;
    return cls == C_NL && s == F_SWALLOW ? F_SWALLOW : F_NONE;
}
// backward: 1 = a newline lies ahead in the whitespace run (seen from the character in front of this one)
HUTK_PS_HD uint32_t bwd_step(uint32_t v, uint32_t cls) { return cls == C_NL ? 1u : (cls == C_WS || cls == C_SP) ? v : 0u; }

// maps over the states: three bits per forward state, one bit per backward one
constexpr uint32_t FMAP_IDENT = 0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12, FMAP_RESET = 0u, BMAP_IDENT = 2u, BMAP_RESET = 0u;
HUTK_PS_HD uint32_t fmap_get(uint32_t m, uint32_t s) { return (m >> (3u * s)) & 7u; }
HUTK_PS_HD uint32_t fmap_then(uint32_t first, uint32_t second) {
    uint32_t r = 0;
    for (uint32_t s = 0; s < F_STATES; s++) r |= fmap_get(second, fmap_get(first, s)) << (3u * s);
    return r;
}
HUTK_PS_HD uint32_t bmap_get(uint32_t m, uint32_t v) { return (m >> v) & 1u; }
HUTK_PS_HD uint32_t bmap_then(uint32_t first, uint32_t second) { return bmap_get(second, bmap_get(first, 0)) | bmap_get(second, bmap_get(first, 1)) << 1; }
// a chunk's two maps in one word, and the two values that enter a chunk
HUTK_PS_HD uint32_t maps_pack(uint32_t f, uint32_t b) { return f | b << 16; }
HUTK_PS_HD uint32_t carry_pack(uint32_t fwd_state, uint32_t bwd_value) { return fwd_state | bwd_value << 8; }

// the forward map of the bytes [i0, i1), left to right
HUTK_PS_HD uint32_t slice_fmap(const Win& W, int i0, int i1) {
    uint32_t m = FMAP_IDENT;
    for (int i = i0; i < i1; i++) {
        const uint32_t c = W.code[i];
        if (!c) continue;
        if (docbit(W, i)) m = FMAP_RESET;
        uint32_t r = 0;
        for (uint32_t s = 0; s < F_STATES; s++) r |= fwd_step(fmap_get(m, s), cls_of(c)) << (3u * s);
        m = r;
    }
    return m;
}
// the backward map of the same bytes, right to left
HUTK_PS_HD uint32_t slice_bmap(const Win& W, int i0, int i1) {
    uint32_t m = BMAP_IDENT;
    for (int i = i1 - 1; i >= i0; i--) {
        if (docbit(W, i + 1)) m = BMAP_RESET;
        const uint32_t c = W.code[i];
        if (c) m = bwd_step(bmap_get(m, 0), cls_of(c)) | bwd_step(bmap_get(m, 1), cls_of(c)) << 1;
    }
    return m;
}

// a word starts at the character at i: fwd = the forward state in front of it, ahead = the backward value behind it
HUTK_PS_HD bool starts_word(const Win& W, int preset, int i, uint32_t fwd, uint32_t ahead) {
    const int p = prev_char(W, i);
    if (p < 0) return true;
    const int role = contraction_role(W, preset, i);
    if (role) return role == ROLE_AFTER;
    const uint32_t c = cls_of(W.code[i]), pc = cls_of(W.code[p]);
    if (is_ws(c)) {
        if (preset != PRESET_GPT2) {
            if (c == C_NL) return pc == C_L || pc == C_N;  // behind an "other" run it is swallowed, inside a run it is no start
            if (pc == C_NL) return fwd == F_SWALLOW || !ahead;  // the run begins here, or its last newline is right in front
        }
        if (!is_ws(pc)) return true;
        const int n = next_char(W, i);  // the last of a run gives itself to what follows
        return n >= 0 && !is_ws(cls_of(W.code[n]));
    }
    if (is_other(c)) return !is_other(pc) && pc != C_SP;
    if (preset == PRESET_GPT2) return pc != c && pc != C_SP;
    if (c == C_N) return preset == PRESET_QWEN2 || (fwd != F_D1 && fwd != F_D2);
    // a letter under cl100k / qwen2: one character that is no newline, letter or number in front joins the run, when a match begins at it
    if (pc == C_L) return false;
    if (pc == C_N || pc == C_NL) return true;
    if (is_ws(pc)) return false;  // (the last of a whitespace run always begins a match)
    const uint32_t ppc = cls_at(W, prev_char(W, p));
    return is_other(ppc) || ppc == C_SP;  // the "other" character belongs to a run of its own
}

// the 16 start bits of the slice [i0, i0 + 16): fwd = the state in front of it, ahead = the value behind it
HUTK_PS_HD uint32_t slice_starts(const Win& W, int preset, int i0, int n, uint32_t fwd, uint32_t ahead) {
    uint32_t ahead_bits = 0, out = 0;
    for (int i = i0 + n - 1; i >= i0; i--) {
        if (docbit(W, i + 1)) ahead = 0;
        const uint32_t c = W.code[i];
        if (!c) continue;
        ahead_bits |= ahead << (i - i0);
        ahead = bwd_step(ahead, cls_of(c));
    }
    for (int i = i0; i < i0 + n; i++) {
        const uint32_t c = W.code[i];
        if (!c) continue;
        if (docbit(W, i)) fwd = F_NONE;
        if (starts_word(W, preset, i, fwd, (ahead_bits >> (i - i0)) & 1u)) out |= 1u << (i - i0);
        fwd = fwd_step(fwd, cls_of(c));
    }
    return out;
}

// ---- the blob ----
inline uint32_t blob_word(const uint8_t* blob, size_t at) {
    uint32_t v;
    std::memcpy(&v, blob + at, 4);
    return v;
}
// Every offset and index is checked before anything reads through it (the two-bit entries have no bad value).
inline bool validate_blob(const uint8_t* blob, int64_t n, uint32_t (&h)[HEADER_WORDS], std::string* why) {
    auto bad = [&](const char* m) {
        *why = std::string("pre-tokeniser tables: ") + m;
        return false;
    };
    if (!blob || n < (int64_t)(4 * HEADER_WORDS)) return bad("shorter than the header");
    for (uint32_t i = 0; i < HEADER_WORDS; i++) h[i] = blob_word(blob, 4 * (size_t)i);
    if (h[H_MAGIC] != MAGIC) return bad("wrong magic");
    if (h[H_VERSION] != VERSION) return bad("unknown format version");
    if ((int64_t)h[H_BYTES] != n) return bad("the size in the header is not the size of the blob (truncated?)");
    if (h[H_BLOCK_SHIFT] != BLOCK_SHIFT || h[H_STAGE1_N] != STAGE1_N) return bad("unexpected stage-one geometry");
    const uint64_t size = (uint64_t)n;
    auto section = [&](int off, uint64_t bytes) {
        const uint64_t o = h[off];
        return o % 4 == 0 && o >= 4 * HEADER_WORDS && o <= size && bytes <= size - o;
    };
    const uint64_t blocks = h[H_BLOCKS_N];
    if (!section(H_STAGE1_OFF, 2ull * STAGE1_N)) return bad("stage one lies outside the blob");
    if (blocks == 0 || blocks > 65535 || !section(H_BLOCKS_OFF, blocks * BLOCK_WORDS * 4)) return bad("the class blocks lie outside the blob");
    for (uint32_t i = 0; i < STAGE1_N; i++) {
        uint16_t b;
        std::memcpy(&b, blob + h[H_STAGE1_OFF] + 2 * (size_t)i, 2);
        if (b >= blocks) return bad("a stage-one entry names a block that is not there");
    }
    return true;
}
inline Tables tables_of(const uint8_t* blob, const uint32_t (&h)[HEADER_WORDS]) {
    return Tables{reinterpret_cast<const uint16_t*>(blob + h[H_STAGE1_OFF]), reinterpret_cast<const uint32_t*>(blob + h[H_BLOCKS_OFF])};
}

}  // namespace presplit
}  // namespace hutk
