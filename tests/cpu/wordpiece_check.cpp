// wordpiece_check.cpp -- the WordPiece rule of hutoken_amd/csrc/hutk_wordpiece.h on the CPU (tests/test_wordpiece_cpu.py
// builds this with -fsanitize=address,undefined and runs it as a child process).  The kernels of hutk_wordpiece.hip call
// the same functions; what is restated here is only their orchestration -- a chunk's slices in order, the scans, a
// word's candidate ends from the longest down -- with the chunk size as an argument, so short texts cross many edges.
//
//   wordpiece_check validate BLOB             exit 0: the blob is accepted; exit 3 and a message: refused
//   wordpiece_check fold BLOB CASE OUT        one fold pass over a packed batch
//   wordpiece_check match BLOB CASE OUT       split and match over a folded batch
//
// fold CASE:  int64 mode, pad (0/1), chunk, n_docs, n_bytes, int64 offsets[n_docs + 1], uint8 bytes[n_bytes]
// fold OUT:   int64 total, int64 out_offsets[n_docs + 1], uint8 bytes[total]
// match CASE: int64 flags, max_chars, chunk, n_vocab, n_vocab_bytes, n_unk, n_prefix, n_docs, n_bytes,
//             int64 vocab_offsets[n_vocab + 1], uint8 vocab[n_vocab_bytes], unk[n_unk], prefix[n_prefix],
//             int64 offsets[n_docs + 1], uint8 bytes[n_bytes]
// match OUT:  int64 total, int64 out_offsets[n_docs + 1], int32 ids[total], int32 word_ids[total]
// exit 5 and a message: the vocabulary is refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hutk_wordpiece.h"

namespace W = hutk::wp;

static bool read_file(const char* path, std::vector<uint8_t>& v) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    const bool ok = n == 0 || std::fread(v.data(), 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return ok;
}

struct Reader {
    const std::vector<uint8_t>& raw;
    size_t at = 0;
    int64_t i64() {
        int64_t v;
        need(8);
        std::memcpy(&v, raw.data() + at, 8);
        at += 8;
        return v;
    }
    void need(size_t n) {
        if (at + n > raw.size()) {
            std::fprintf(stderr, "wordpiece_check: the case file is cut short\n");
            std::exit(2);
        }
    }
    std::vector<int64_t> i64s(size_t n) {
        std::vector<int64_t> v(n);
        need(8 * n);
        if (n) std::memcpy(v.data(), raw.data() + at, 8 * n);
        at += 8 * n;
        return v;
    }
    std::vector<uint8_t> bytes(size_t n) {  // (its own allocation: a read past it is caught)
        need(n);
        std::vector<uint8_t> v(raw.begin() + (long)at, raw.begin() + (long)(at + n));
        at += n;
        return v;
    }
};

static void check_offsets(const std::vector<int64_t>& offs, int64_t n_bytes) {
    bool ok = offs[0] == 0 && offs.back() == n_bytes;
    for (size_t i = 0; i + 1 < offs.size(); i++) ok = ok && offs[i + 1] >= offs[i];
    if (!ok) std::exit(2);
}

static std::vector<uint8_t> flags_of(const std::vector<int64_t>& offs, int64_t n) {
    std::vector<uint8_t> flag((size_t)n + 1, 0);
    for (size_t i = 0; i + 1 < offs.size(); i++) flag[(size_t)offs[i]] = 1;
    return flag;
}

// what k_wp_fold_count, the scan, k_wp_fold_write and k_wp_fold_docs do
static int fold(const W::Tables& T, Reader& in, const char* out_path) {
    const uint32_t mode = (uint32_t)in.i64();
    const bool pad = in.i64() != 0;
    const int64_t chunk = in.i64(), n_docs = in.i64(), n_bytes = in.i64();
    if (chunk < W::SLICE_BYTES || chunk % W::SLICE_BYTES || n_docs < 0 || n_bytes < 0) return 2;
    const std::vector<int64_t> offs = in.i64s((size_t)n_docs + 1);
    const std::vector<uint8_t> bytes = in.bytes((size_t)n_bytes);
    check_offsets(offs, n_bytes);
    const std::vector<uint8_t> flag = flags_of(offs, n_bytes);
    const W::Text x{bytes.data(), flag.data(), n_bytes};
    const int64_t slices = chunk / W::SLICE_BYTES, n_chunks = (n_bytes + chunk - 1) / chunk;
    std::vector<int64_t> base((size_t)n_chunks + 1, 0), slice((size_t)(n_chunks * slices), 0);
    for (int64_t k = 0; k < n_chunks; k++) {
        int64_t sum = 0;
        for (int64_t t = 0; t < slices; t++) {
            const int64_t a = k * chunk + t * W::SLICE_BYTES, e = a + W::SLICE_BYTES < n_bytes ? a + W::SLICE_BYTES : n_bytes;
            slice[(size_t)(k * slices + t)] = sum;
            if (a < e) sum += W::fold_range(T, x, a, e, mode, nullptr);
        }
        base[(size_t)k] = sum;
    }
    int64_t total = 0;
    for (int64_t k = 0; k <= n_chunks; k++) {
        const int64_t v = k < n_chunks ? base[(size_t)k] : 0;
        base[(size_t)k] = total;
        total += v;
    }
    const int64_t end = pad ? n_bytes : total;
    if (total > end) return 4;
    std::vector<uint8_t> out((size_t)end, 0x20);
    for (int64_t k = 0; k < n_chunks; k++)
        for (int64_t t = 0; t < slices; t++) {
            const int64_t a = k * chunk + t * W::SLICE_BYTES, e = a + W::SLICE_BYTES < n_bytes ? a + W::SLICE_BYTES : n_bytes;
            if (a >= e) continue;
            const int64_t to = base[(size_t)k] + slice[(size_t)(k * slices + t)];
            const int64_t n = W::fold_range(T, x, a, e, mode, nullptr);
            if (to + n > total) return 4;
            std::vector<uint8_t> piece((size_t)n + 1);  // (written on its own: a slice that writes more than it counted is caught)
            if (W::fold_range(T, x, a, e, mode, piece.data()) != n) return 4;
            std::memcpy(out.data() + to, piece.data(), (size_t)n);
        }
    std::vector<int64_t> oo((size_t)n_docs + 1, end);
    for (int64_t d = 0; d < n_docs; d++) {
        const int64_t o = offs[(size_t)d];
        if (o >= n_bytes) {
            oo[(size_t)d] = total;
            continue;
        }
        const int64_t k = o / chunk, s0 = o & ~(int64_t)(W::SLICE_BYTES - 1);
        oo[(size_t)d] = base[(size_t)k] + slice[(size_t)(k * slices + (s0 - k * chunk) / W::SLICE_BYTES)] + W::fold_range(T, x, s0, o, mode, nullptr);
    }
    FILE* f = std::fopen(out_path, "wb");
    if (!f) return 2;
    std::fwrite(&end, 8, 1, f);
    std::fwrite(oo.data(), 8, oo.size(), f);
    if (!out.empty()) std::fwrite(out.data(), 1, out.size(), f);
    std::fclose(f);
    return 0;
}

// what match_word does, the group's lanes one after the other
static void match_word(const W::Tables& T, const W::Text& x, const W::Vocab& V, uint32_t flags, int32_t max_chars, int32_t unk,
                       int64_t ws, std::vector<int32_t>& tmp) {
    constexpr int GROUP = 8;
    uint32_t cp;
    int len = W::char_at(x, ws, &cp);
    int64_t p = ws + len;
    int chars = 1;
    if (!W::is_alone(W::class_of(W::entry(T, cp), flags), flags)) {
        while (chars <= max_chars && p < x.n && !x.flag[p]) {
            len = W::char_at(x, p, &cp);
            const int c = W::class_of(W::entry(T, cp), flags);
            if (W::is_space(c) || W::is_alone(c, flags)) break;
            p += len;
            chars++;
        }
    }
    if (chars > max_chars) {
        tmp[(size_t)ws] = unk | W::ID_START;
        return;
    }
    const int wl = (int)(p - ws);
    const uint8_t* w = x.bytes + ws;
    int s = 0, np = 0;
    while (s < wl) {
        const int kind = s > 0;
        const int top = wl - s < V.max_len[kind] ? wl : s + V.max_len[kind];
        int hit_end = -1;
        int32_t hit_id = -1;
        for (int base = top; base > s && hit_end < 0; base -= GROUP)
            for (int gl = 0; gl < GROUP && hit_end < 0; gl++) {
                const int e = base - gl;
                if (e > s && (e == wl || W::is_char_start(x, ws + e))) {
                    const int32_t id = W::probe(V, w + s, e - s, kind);
                    if (id >= 0) hit_end = e, hit_id = id;
                }
            }
        if (hit_end < 0) {
            for (int j = 1; j < np; j++) tmp[(size_t)(ws + j)] = -1;
            tmp[(size_t)ws] = unk | W::ID_START;
            return;
        }
        tmp[(size_t)(ws + np)] = hit_id | (np ? 0 : W::ID_START);
        np++;
        s = hit_end;
    }
}

static int match(const W::Tables& T, Reader& in, const char* out_path) {
    const uint32_t flags = (uint32_t)in.i64();
    const int32_t max_chars = (int32_t)in.i64();
    const int64_t chunk = in.i64(), n_vocab = in.i64(), n_vocab_bytes = in.i64(), n_unk = in.i64(), n_prefix = in.i64();
    const int64_t n_docs = in.i64(), n_bytes = in.i64();
    if (chunk < W::SLICE_BYTES || chunk % W::SLICE_BYTES || n_docs < 0 || n_bytes < 0 || n_vocab < 0) return 2;
    const std::vector<int64_t> voffs = in.i64s((size_t)n_vocab + 1);
    const std::vector<uint8_t> vocab = in.bytes((size_t)n_vocab_bytes), unk = in.bytes((size_t)n_unk), prefix = in.bytes((size_t)n_prefix);
    const std::vector<int64_t> offs = in.i64s((size_t)n_docs + 1);
    const std::vector<uint8_t> bytes = in.bytes((size_t)n_bytes);
    check_offsets(offs, n_bytes);
    W::VocabHost vh;
    std::string why;
    if (W::build_vocab(vocab.data(), voffs.data(), n_vocab, std::string(unk.begin(), unk.end()), std::string(prefix.begin(), prefix.end()),
                       max_chars, vh, &why)) {
        std::fprintf(stderr, "refused: %s\n", why.c_str());
        return 5;
    }
    const std::vector<uint8_t> keys(vh.keys);  // (exactly as long as the keys: the probe reads no byte behind them)
    const W::Vocab V = vh.view(vh.slots.data(), keys.data());
    const std::vector<uint8_t> flag = flags_of(offs, n_bytes);
    const W::Text x{bytes.data(), flag.data(), n_bytes};
    std::vector<int32_t> tmp((size_t)n_bytes, -1);
    // k_wp_match: the word starts of a chunk, then its words
    for (int64_t c0 = 0; c0 < n_bytes; c0 += chunk) {
        std::vector<int64_t> starts;
        for (int64_t p = c0; p < c0 + chunk && p < n_bytes; p++) {
            if (!W::is_char_start(x, p)) continue;
            uint32_t cp;
            (void)W::char_at(x, p, &cp);
            if (W::word_starts(T, x, p, W::class_of(W::entry(T, cp), flags), flags)) starts.push_back(p);
        }
        for (int64_t ws : starts) match_word(T, x, V, flags, max_chars, vh.unk, ws, tmp);
    }
    // k_wp_count .. k_wp_write
    std::vector<int32_t> ids, wids;
    std::vector<int64_t> oo((size_t)n_docs + 1, 0);
    int64_t d = 0, word = 0, word_base = 0;
    for (int64_t p = 0; p <= n_bytes; p++) {
        while (d <= n_docs && offs[(size_t)d] == p) {
            if (d < n_docs) word_base = word;
            oo[(size_t)d++] = (int64_t)ids.size();
        }
        if (p == n_bytes) break;
        const int32_t v = tmp[(size_t)p];
        if (v < 0) continue;
        word += (v & W::ID_START) != 0;
        ids.push_back(v & W::ID_MASK);
        wids.push_back((int32_t)(word - 1 - word_base));
    }
    FILE* f = std::fopen(out_path, "wb");
    if (!f) return 2;
    const int64_t total = (int64_t)ids.size();
    std::fwrite(&total, 8, 1, f);
    std::fwrite(oo.data(), 8, oo.size(), f);
    if (total) std::fwrite(ids.data(), 4, ids.size(), f);
    if (total) std::fwrite(wids.data(), 4, wids.size(), f);
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: wordpiece_check validate BLOB | fold BLOB CASE OUT | match BLOB CASE OUT\n");
        return 2;
    }
    std::vector<uint8_t> blob;
    if (!read_file(argv[2], blob)) {
        std::fprintf(stderr, "wordpiece_check: cannot read %s\n", argv[2]);
        return 2;
    }
    uint32_t h[W::HEADER_WORDS];
    std::string why;
    if (!W::validate_blob(blob.data(), (int64_t)blob.size(), h, &why)) {
        std::fprintf(stderr, "refused: %s\n", why.c_str());
        return 3;
    }
    const std::string cmd(argv[1]);
    if (cmd == "validate") return 0;
    if ((cmd != "fold" && cmd != "match") || argc != 5) return 2;
    const W::Tables T = W::tables_of(blob.data(), h);
    std::vector<uint8_t> raw;
    if (!read_file(argv[3], raw)) return 2;
    Reader in{raw};
    return cmd == "fold" ? fold(T, in, argv[4]) : match(T, in, argv[4]);
}
