// hutk_norm.h -- Unicode normalisation (NFC, NFD, NFKC, NFKD) of packed UTF-8, as the kernels of hutk_normalize.hip run
// it: the UTF-8 validity rule, the segment rule and the per-segment normaliser.  Compiled for the device AND for the
// host (tests/cpu/norm_check.cpp runs the same chunk, slice and segment logic on the CPU, under the sanitizers), so it
// is plain integer C++ over a view of the table blob (hutoken_amd/normalize.py builds it; include/hutoken_amd.h and that
// module document the format; validate_blob() below is what hutk_normalizer_create refuses a blob by).
//
// Contract: the output document is
//     d.decode("utf-8", "surrogateescape") -> unicodedata.normalize(F, .) -> .encode("utf-8", "surrogateescape")
// A byte that strict UTF-8 rejects (decode() returns 0) is carried as the escape value 0xDC00 + byte: a starter that no
// table knows, written back as that one byte.
//
// Ownership.  The packed text is cut into chunks of CHUNK_BYTES and those into slices of SLICE_BYTES; a SEGMENT starts at
// a document start, at an ill-formed byte or at a character that is a safe boundary under the form, and ends where the
// next one starts.  A segment belongs to the slice its first byte lies in: slice_run() walks the characters that start
// in its slice, skips those that belong to an earlier segment, and follows a segment it owns to its end, wherever that
// is -- but never across the document's end.  Segments are independent, so every slice's output depends on the text alone.
//
// A segment is decomposed (rd_next: a reader that yields the fully decomposed code points one by one and can be copied,
// so a stretch can be walked again), reordered and composed per "starter + run of marks":
//   * a run of up to RUN_BUF marks is sorted in a private buffer (one and two marks: in registers);
//   * a longer run is never stored: for_sorted() walks it once per combining class, in ascending order, and the composed
//     starter is found by one such sorted walk before anything is written, the marks that stay by a second one.
// So the result is exact at any length.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HUTK_NORM_HD __host__ __device__ inline
#else
#define HUTK_NORM_HD inline
#endif
#include <cstring>
#include <string>

namespace hutk {
namespace norm {

enum : int { FORM_NFC = 0, FORM_NFD = 1, FORM_NFKC = 2, FORM_NFKD = 3, N_FORMS = 4 };  // bit 0: no composition; bit 1: compatibility
constexpr int CHUNK_BYTES = 4096, SLICE_BYTES = 16, CHUNK_SLICES = CHUNK_BYTES / SLICE_BYTES;
constexpr int RUN_BUF = 16;  // marks of one run that are sorted in a buffer

constexpr uint32_t MAGIC = 0x4D524E48u, VERSION = 1u, HEADER_WORDS = 32u, BLOCK_SHIFT = 7u, PAIR_EMPTY = 0xFFFFFFFFu;
enum : int {
    H_MAGIC = 0, H_VERSION, H_UNIDATA, H_BYTES, H_STAGE1_OFF, H_STAGE1_N, H_PROPS_OFF, H_PROPS_BLOCKS, H_DECOMP_OFF, H_DECOMP_N,
    H_PAIRS_OFF, H_PAIR_SLOTS, H_PAIRS_N, H_BLOCK_SHIFT, H_LEAD = 16, H_RATIO = 20, H_FIRST_CP = 24
};
constexpr uint32_t N_CP = 0x110000u, STAGE1_N = N_CP >> BLOCK_SHIFT, MAX_DECOMP = 18u;
constexpr uint32_t E_CP = 0x1FFFFFu, E_SECOND = 1u << 21, E_CCC_SHIFT = 24;  // a decomposed entry: code point | flags | ccc
constexpr uint32_t P_SECOND = 1u << 12;
constexpr uint32_t S_BASE = 0xAC00u, S_COUNT = 11172u, L_BASE = 0x1100u, V_BASE = 0x1161u, T_BASE = 0x11A7u;
constexpr uint32_t ESCAPE = 0xDC00u;  // + the ill-formed byte
constexpr uint32_t NONE = 0xFFFFFFFFu;

// the blob's sections (host or device pointers) and what the form needs of the header
struct Tables {
    const uint16_t* stage1;
    const uint32_t* props;
    const uint32_t* decomp;
    const uint32_t* pairs;
    uint32_t pair_mask;
};

struct Text {
    const uint8_t* bytes;
    const int64_t* offs;  // [n_docs + 1]
    int64_t n_docs, n_bytes;
    uint32_t lead;        // the form's first unstable lead byte: a character that starts below it is stable and a boundary
    int form;
};

// Length of the well-formed character at p (its document ends at `end`) and its scalar value; 0: the byte is one that
// Python's strict decoder rejects -- a lone continuation byte, C0, C1, F5..FF, an overlong form, an encoded surrogate, a
// value above U+10FFFF, a sequence the document's end cuts short.  U+0000 is a character like any other.
HUTK_NORM_HD int decode(const uint8_t* b, int64_t p, int64_t end, uint32_t* cp) {
    const uint32_t b0 = b[p];
    if (b0 < 0x80u) {
        *cp = b0;
        return 1;
    }
    if (b0 < 0xC2u || b0 > 0xF4u) return 0;
    const int len = b0 < 0xE0u ? 2 : b0 < 0xF0u ? 3 : 4;
    if (p + len > end) return 0;
    uint32_t lo = 0x80u, hi = 0xBFu;
    if (b0 == 0xE0u) lo = 0xA0u;
    else if (b0 == 0xEDu) hi = 0x9Fu;
    else if (b0 == 0xF0u) lo = 0x90u;
    else if (b0 == 0xF4u) hi = 0x8Fu;
    const uint32_t b1 = b[p + 1];
    if (b1 < lo || b1 > hi) return 0;
    uint32_t c = (len == 2 ? b0 & 0x1Fu : len == 3 ? b0 & 0x0Fu : b0 & 0x07u) << 6 | (b1 & 0x3Fu);
    for (int i = 2; i < len; i++) {
        const uint32_t bi = b[p + i];
        if ((bi & 0xC0u) != 0x80u) return 0;
        c = c << 6 | (bi & 0x3Fu);
    }
    *cp = c;
    return len;
}

// How many bytes at p .. continue a well-formed character that starts before p, inside the document [ds, de).  The
// nearest byte in front of p that is no continuation byte is the start of a character or an ill-formed byte whatever
// stands before it, so three bytes of look-back place every slice on the character grid.
HUTK_NORM_HD int spill(const uint8_t* b, int64_t p, int64_t ds, int64_t de) {
    if (p >= de || (b[p] & 0xC0u) != 0x80u) return 0;
    for (int j = 1; j <= 3; j++) {
        const int64_t q = p - j;
        if (q < ds) return 0;
        if ((b[q] & 0xC0u) == 0x80u) continue;
        uint32_t cp;
        const int len = decode(b, q, de, &cp);
        return q + len > p ? (int)(q + len - p) : 0;
    }
    return 0;
}

HUTK_NORM_HD void props(const Tables& T, uint32_t cp, uint32_t* w0, uint32_t* w1) {
    const uint32_t at = (((uint32_t)T.stage1[cp >> BLOCK_SHIFT] << BLOCK_SHIFT) | (cp & ((1u << BLOCK_SHIFT) - 1u))) * 2u;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint2 w = *reinterpret_cast<const uint2*>(T.props + at);
    *w0 = w.x;
    *w1 = w.y;
#else
    *w0 = T.props[at];
    *w1 = T.props[at + 1];
#endif
}

// composed forms: ccc 0 and quick check Yes; decomposed forms: ccc 0 and a decomposition that begins with a starter
HUTK_NORM_HD bool safe_boundary(uint32_t w0, int form) {
    if (w0 & 0xFFu) return false;
    if (!(form & 1)) return (w0 >> (8 + form)) & 1u;
    return ((w0 >> (form & 2 ? 24 : 16)) & 0xFFu) == 0;
}

HUTK_NORM_HD uint32_t pair_hash(uint32_t a, uint32_t b) { return ((a * 31u + b) * 0x9E3779B1u) >> 12; }

// the primary composite of a + b, 0: none.  Hangul by arithmetic, the rest from the pair table.
HUTK_NORM_HD uint32_t compose(const Tables& T, uint32_t a, uint32_t b) {
    if (a - L_BASE < 19u) return b - V_BASE < 21u ? S_BASE + ((a - L_BASE) * 21u + (b - V_BASE)) * 28u : 0u;
    if (a - S_BASE < S_COUNT && b - (T_BASE + 1u) < 27u) return (a - S_BASE) % 28u == 0 ? a + (b - T_BASE) : 0u;
    for (uint32_t s = pair_hash(a, b) & T.pair_mask;; s = (s + 1u) & T.pair_mask) {  // (validate_blob: an empty slot exists)
        const uint32_t* e = T.pairs + 4u * s;
        if (e[0] == PAIR_EMPTY) return 0u;
        if (e[0] == a && e[1] == b) return e[2];
    }
}

// ---- where the output goes: counted, compared with the input (did the segment change?), or written ----
struct CountSink {
    int64_t pos = 0;
    bool same = true;
    const uint8_t* in = nullptr;
    int64_t ip = 0, iend = 0;
    HUTK_NORM_HD void begin(const uint8_t* bytes, int64_t s, int64_t q) { in = bytes, ip = s, iend = q, same = true; }
    HUTK_NORM_HD void put(uint32_t v) {
        same = same && ip < iend && in[ip] == v;
        ip++;
        pos++;
    }
    HUTK_NORM_HD void copy(const uint8_t*, int64_t s, int64_t q) { pos += q - s, ip = iend = q, same = true; }
    HUTK_NORM_HD bool end() const { return same && ip == iend; }
};
struct WriteSink {
    uint8_t* out;
    int64_t cap;
    int64_t pos;
    HUTK_NORM_HD void begin(const uint8_t*, int64_t, int64_t) {}
    HUTK_NORM_HD void put(uint32_t v) {
        if (pos < cap) out[pos] = (uint8_t)v;
        pos++;
    }
    HUTK_NORM_HD void copy(const uint8_t* bytes, int64_t s, int64_t q) {
        for (; s < q; s++) put(bytes[s]);
    }
    HUTK_NORM_HD bool end() const { return true; }
};

template <class Sink>
HUTK_NORM_HD void put_cp(Sink& o, uint32_t c) {
    if (c < 0x80u) o.put(c);
    else if (c < 0x800u) o.put(0xC0u | c >> 6), o.put(0x80u | (c & 0x3Fu));
    else if (c - ESCAPE - 0x80u < 0x80u) o.put(c - ESCAPE);
    else if (c < 0x10000u) o.put(0xE0u | c >> 12), o.put(0x80u | ((c >> 6) & 0x3Fu)), o.put(0x80u | (c & 0x3Fu));
    else o.put(0xF0u | c >> 18), o.put(0x80u | ((c >> 12) & 0x3Fu)), o.put(0x80u | ((c >> 6) & 0x3Fu)), o.put(0x80u | (c & 0x3Fu));
}

// ---- the reader: the fully decomposed code points of bytes[p, end), one entry (code point | flags | ccc) a call ----
struct Reader {
    int64_t p, end;
    const uint32_t* dec;  // entries of the character under way; null with k < n: a Hangul syllable
    uint32_t k, n, hs;
};

HUTK_NORM_HD bool rd_next(const Tables& T, int form, const uint8_t* bytes, Reader& r, uint32_t* e) {
    if (r.k < r.n) {
        if (r.dec) *e = r.dec[r.k];
        else *e = (r.k == 1 ? V_BASE + (r.hs % 588u) / 28u : T_BASE + r.hs % 28u) | E_SECOND;
        r.k++;
        return true;
    }
    if (r.p >= r.end) return false;
    uint32_t cp;
    const int len = decode(bytes, r.p, r.end, &cp);
    if (len == 0) {
        *e = ESCAPE + bytes[r.p];
        r.p++;
        return true;
    }
    r.p += len;
    r.k = r.n = 0;
    if (cp < 0xA0u) {  // (below every form's first unstable code point)
        *e = cp;
        return true;
    }
    if (cp - S_BASE < S_COUNT) {
        r.dec = nullptr, r.hs = cp - S_BASE, r.k = 1, r.n = 2u + (r.hs % 28u != 0);
        *e = L_BASE + r.hs / 588u;
        return true;
    }
    uint32_t w0, w1;
    props(T, cp, &w0, &w1);
    const uint32_t idx = form & 2 ? w1 >> 16 : w1 & 0xFFFFu;
    if (!idx) {
        *e = cp | (w0 & P_SECOND ? E_SECOND : 0u) | (w0 & 0xFFu) << E_CCC_SHIFT;
        return true;
    }
    r.dec = T.decomp + idx + 1;
    r.n = T.decomp[idx];
    r.k = 1;
    *e = r.dec[0];
    return true;
}

// f(entry) for the n marks of the run that begins with e0 and continues at reader r0, in canonical order: ascending
// combining class, equal classes in the order of the text.  minc: the smallest class among them.
template <class F>
HUTK_NORM_HD void for_sorted(const Tables& T, int form, const uint8_t* bytes, const Reader& r0, uint32_t e0, uint32_t n, uint32_t minc, F&& f) {
    if (n == 1) {
        f(e0);
        return;
    }
    Reader w = r0;
    uint32_t x = e0;
    if (n == 2) {
        uint32_t y = 0;
        rd_next(T, form, bytes, w, &y);
        if ((y >> E_CCC_SHIFT) < (x >> E_CCC_SHIFT)) f(y), f(x);
        else f(x), f(y);
        return;
    }
    if (n <= (uint32_t)RUN_BUF) {
        uint32_t buf[RUN_BUF];
        for (uint32_t i = 0; i < n; i++) {  // insertion sort: stable
            uint32_t j = i;
            for (; j > 0 && (buf[j - 1] >> E_CCC_SHIFT) > (x >> E_CCC_SHIFT); j--) buf[j] = buf[j - 1];
            buf[j] = x;
            if (i + 1 < n) rd_next(T, form, bytes, w, &x);
        }
        for (uint32_t i = 0; i < n; i++) f(buf[i]);
        return;
    }
    for (uint32_t cur = minc; cur < 256u;) {  // no buffer: one walk of the run per class that occurs in it
        uint32_t nxt = 256u;
        w = r0, x = e0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t c = x >> E_CCC_SHIFT;
            if (c == cur) f(x);
            else if (c > cur && c < nxt) nxt = c;
            if (i + 1 < n) rd_next(T, form, bytes, w, &x);
        }
        cur = nxt;
    }
}

// The normal form of the segment bytes[s, q) into the sink.  The decomposed segment is a sequence of "starter, run of
// marks" (the first may lack the starter).  Decomposed forms: the starter, then the marks in canonical order.  Composed
// forms: the starter takes, in canonical order, every mark it has a composite with and that no mark of the same class
// left behind blocks; when no mark is left, it takes the next starter too if the two have a composite (Hangul L + V and
// LV + T, U+09C7 + U+09BE ..) and goes on with that starter's marks.
template <class Sink>
HUTK_NORM_HD void normalise_segment(const Tables& T, int form, const uint8_t* bytes, int64_t s, int64_t q, Sink& out) {
    const bool composing = !(form & 1);
    Reader r{s, q, nullptr, 0u, 0u, 0u};
    uint32_t e = 0;
    bool have = rd_next(T, form, bytes, r, &e);
    while (have) {
        uint32_t S = NONE;
        if ((e >> E_CCC_SHIFT) == 0) {
            S = e & E_CP;
            have = rd_next(T, form, bytes, r, &e);
        }
        for (;;) {
            const Reader r0 = r;  // the run of marks: its first entry e0, the rest behind r0
            const uint32_t e0 = e;
            uint32_t n = 0, minc = 256u;
            while (have && (e >> E_CCC_SHIFT) != 0) {
                n++;
                if ((e >> E_CCC_SHIFT) < minc) minc = e >> E_CCC_SHIFT;
                have = rd_next(T, form, bytes, r, &e);
            }
            if (!composing || S == NONE) {
                if (S != NONE) put_cp(out, S);
                if (n) for_sorted(T, form, bytes, r0, e0, n, minc, [&](uint32_t x) { put_cp(out, x & E_CP); });
                break;
            }
            uint32_t C = S, left = 0, lastc = 0;
            auto take = [&](uint32_t x) -> bool {  // does the starter take this mark?
                const uint32_t c = x >> E_CCC_SHIFT;
                if ((x & E_SECOND) && !(left && lastc == c)) {
                    const uint32_t y = compose(T, C, x & E_CP);
                    if (y) {
                        C = y;
                        return true;
                    }
                }
                left++;
                lastc = c;
                return false;
            };
            if (n) for_sorted(T, form, bytes, r0, e0, n, minc, [&](uint32_t x) { (void)take(x); });
            if (left == 0 && have && (e & E_SECOND)) {  // (e is a starter here: the run ended at it)
                const uint32_t y = compose(T, C, e & E_CP);
                if (y) {
                    S = y;
                    have = rd_next(T, form, bytes, r, &e);
                    continue;
                }
            }
            put_cp(out, C);
            if (left) {
                C = S, left = 0, lastc = 0;
                for_sorted(T, form, bytes, r0, e0, n, minc, [&](uint32_t x) {
                    if (!take(x)) put_cp(out, x & E_CP);
                });
            }
            break;
        }
    }
}

// Is the character at p (inside its document, which ends at de) the start of a segment?  *len: its length, one for an
// ill-formed byte; *stable: it is its own normal form when it is a segment of its own.
HUTK_NORM_HD bool char_starts_segment(const Tables& T, const Text& x, int64_t p, int64_t de, int* len, bool* stable) {
    const uint32_t b0 = x.bytes[p];
    uint32_t cp;
    const int l = decode(x.bytes, p, de, &cp);
    *len = l ? l : 1;
    *stable = true;
    if (l == 0 || b0 < x.lead) return true;  // no table is touched below the form's first unstable lead byte
    uint32_t w0, w1;
    props(T, cp, &w0, &w1);
    *stable = (w0 >> (8 + x.form)) & 1u;
    return safe_boundary(w0, x.form);
}

// The segments that start in bytes[a, e) (a slice; d: the document that holds a, offs[d] <= a < offs[d + 1]) into the sink.
// mark(p, bytes this call has put out before p) at every segment start that a document starts at (and at others, where
// it costs nothing); changed[d] = 1 when a segment's output differs from its input (asked of a CountSink only; null: not
// wanted).  has_high: some byte of the slice is at or above the form's first unstable lead byte.  Without one, and with
// the character behind the slice below it too, every character of the slice is a stable segment of its own: the
// slice's output is its input from its first character to the end of its last, and no table is touched.
template <class Sink, class Mark>
HUTK_NORM_HD void slice_run(const Tables& T, const Text& x, int64_t d, int64_t a, int64_t e, bool has_high, Sink& out, Mark&& mark,
                            uint8_t* changed) {
    int64_t ds = x.offs[d], de = x.offs[d + 1];
    const int64_t pos0 = out.pos;
    int64_t p = a + spill(x.bytes, a, ds, de);
    if (!has_high) {
        int64_t d2 = d, ds2 = ds, de2 = de;  // the document that holds the slice's last byte
        while (e - 1 >= de2) {
            d2++;
            ds2 = de2;
            de2 = x.offs[d2 + 1];
        }
        const int64_t q = e + spill(x.bytes, e, ds2, de2);
        if (q >= x.n_bytes || x.bytes[q] < x.lead) {
            if (p >= q) return;
            if (p == ds) mark(p, 0);
            for (int64_t i = d; i < d2;) {  // the documents that start inside the slice (empty ones share a place)
                i++;
                const int64_t s = x.offs[i];
                if (s >= p && s < e) mark(s, s - p);
            }
            out.copy(x.bytes, p, q);
            return;
        }
    }
    while (p < e) {
        while (p >= de) {  // (p < n_bytes = offs[n_docs]: d stays below n_docs)
            d++;
            ds = de;
            de = x.offs[d + 1];
        }
        int len;
        bool stable;
        bool starts = char_starts_segment(T, x, p, de, &len, &stable);
        if (!starts && p != ds) {  // part of a segment that an earlier slice owns
            p += len;
            continue;
        }
        int64_t q = p + len;
        while (q < de) {
            int l2;
            bool st2;
            if (char_starts_segment(T, x, q, de, &l2, &st2)) break;
            q += l2;
        }
        mark(p, out.pos - pos0);
        if (q == p + len && stable) out.copy(x.bytes, p, q);  // one stable character: by far the most common segment
        else {
            out.begin(x.bytes, p, q);
            normalise_segment(T, x.form, x.bytes, p, q, out);
            if (changed && !out.end()) changed[d] = 1;
        }
        p = q;
    }
}

// ---- what a chunk needs of its edges (one lane of the kernel, and the host check, call these) ----
// first i in [0, n] with offs[i] >= v (offs[n] >= v by the caller's clamp)
HUTK_NORM_HD int64_t first_doc_at_or_after(const int64_t* offs, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (offs[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// bytes at the chunk edge P that belong to a character begun before it; dfirst = first_doc_at_or_after(P)
HUTK_NORM_HD int edge_spill(const Text& x, int64_t P, int64_t dfirst) {
    if (P <= 0 || P >= x.n_bytes || x.offs[dfirst] == P) return 0;
    return spill(x.bytes, P, x.offs[dfirst - 1], x.offs[dfirst]);
}
// the document that holds byte a among those of a chunk: docs [dlo, dhi) start inside the chunk, dlo - 1 reaches into it
HUTK_NORM_HD int64_t doc_of_byte(const int64_t* offs, int64_t dlo, int64_t dhi, int64_t a) {
    int64_t lo = dlo, hi = dhi;  // the number of documents in [dlo, dhi) that start at or before a
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (offs[mid] <= a) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// ---- the blob on the host: checked in full before anything reads through it ----
inline uint32_t blob_word(const uint8_t* blob, size_t at) {
    uint32_t v;
    std::memcpy(&v, blob + at, 4);
    return v;
}

// Every offset, count and index of the blob; false with a message when one does not fit.  On success `h` holds the header.
inline bool validate_blob(const uint8_t* blob, int64_t n, uint32_t (&h)[HEADER_WORDS], std::string* why) {
    auto bad = [&](const char* m) {
        *why = std::string("normaliser tables: ") + m;
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
    const uint64_t blocks = h[H_PROPS_BLOCKS], dn = h[H_DECOMP_N], slots = h[H_PAIR_SLOTS];
    if (!section(H_STAGE1_OFF, 2ull * STAGE1_N)) return bad("stage one lies outside the blob");
    if (blocks == 0 || blocks > 65535 || h[H_PROPS_OFF] % 8 || !section(H_PROPS_OFF, blocks << (BLOCK_SHIFT + 3))) return bad("the property blocks lie outside the blob");
    if (dn == 0 || dn > 65535 || !section(H_DECOMP_OFF, 4 * dn)) return bad("the decompositions lie outside the blob");
    if (slots < 2 || (slots & (slots - 1)) || slots > (1u << 20) || !section(H_PAIRS_OFF, 16 * slots)) return bad("the pair table lies outside the blob or is no power of two");
    for (uint32_t i = 0; i < STAGE1_N; i++) {
        uint16_t b;
        std::memcpy(&b, blob + h[H_STAGE1_OFF] + 2 * (size_t)i, 2);
        if (b >= blocks) return bad("a stage-one entry names a block that is not there");
    }
    const size_t dec = h[H_DECOMP_OFF];
    auto entry_ok = [&](uint32_t idx) {
        if (idx == 0) return true;
        if (idx >= dn) return false;
        const uint32_t len = blob_word(blob, dec + 4 * (size_t)idx);
        if (len < 1 || len > MAX_DECOMP || idx + len >= dn) return false;
        for (uint32_t k = 1; k <= len; k++)
            if ((blob_word(blob, dec + 4 * (size_t)(idx + k)) & E_CP) >= N_CP) return false;
        return true;
    };
    for (uint64_t i = 0; i < blocks << BLOCK_SHIFT; i++) {
        const uint32_t w1 = blob_word(blob, h[H_PROPS_OFF] + 8 * (size_t)i + 4);
        if (!entry_ok(w1 & 0xFFFFu) || !entry_ok(w1 >> 16)) return bad("a decomposition offset or length leaves the table");
    }
    uint64_t filled = 0;
    for (uint64_t s = 0; s < slots; s++) {
        const size_t at = h[H_PAIRS_OFF] + 16 * (size_t)s;
        const uint32_t a = blob_word(blob, at), b = blob_word(blob, at + 4), c = blob_word(blob, at + 8);
        if (a == PAIR_EMPTY) continue;
        if (a >= N_CP || b >= N_CP || c >= N_CP || c == 0) return bad("a composite pair holds no code point");
        filled++;
    }
    if (filled != h[H_PAIRS_N] || filled >= slots) return bad("the pair table's count is wrong or it has no empty slot");
    for (int f = 0; f < N_FORMS; f++) {
        if (h[H_LEAD + f] < 0xC2u || h[H_LEAD + f] > 0xF4u) return bad("a form's first unstable lead byte is no lead byte");
        if (h[H_RATIO + f] < 1 || h[H_RATIO + f] > 4 * MAX_DECOMP) return bad("a form's expansion ratio is out of range");
    }
    return true;
}

inline Tables tables_of(const uint8_t* blob, const uint32_t (&h)[HEADER_WORDS]) {
    Tables t;
    t.stage1 = reinterpret_cast<const uint16_t*>(blob + h[H_STAGE1_OFF]);
    t.props = reinterpret_cast<const uint32_t*>(blob + h[H_PROPS_OFF]);
    t.decomp = reinterpret_cast<const uint32_t*>(blob + h[H_DECOMP_OFF]);
    t.pairs = reinterpret_cast<const uint32_t*>(blob + h[H_PAIRS_OFF]);
    t.pair_mask = h[H_PAIR_SLOTS] - 1u;
    return t;
}

}  // namespace norm
}  // namespace hutk
