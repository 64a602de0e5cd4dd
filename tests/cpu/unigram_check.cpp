// unigram_check.cpp -- the Unigram rule of hutoken_amd/csrc/hutk_unigram.h on the CPU (tests/test_unigram_cpu.py builds
// this with -fsanitize=address,undefined and runs it as a child process).  The kernels of hutk_unigram.hip call the same
// functions; what is restated here is only their orchestration -- a chunk's slices in order, the scans, a chunk's words
// one after the other in the plain form of the best path -- with the chunk size as an argument, so short texts cross
// many edges.
//
//   unigram_check CASE        exit 0: the ids, offsets and word ids are the expected ones; stdout: "folded N ids M"
//                             exit 1 and a message: a difference;  exit 5 and a message: the vocabulary is refused
//
// CASE: int64 flags, chunk, unk_id, n_pieces, n_piece_bytes, n_docs, n_bytes, n_expect,
//       int64 piece_offsets[n_pieces + 1], double scores[n_pieces], uint8 pieces[n_piece_bytes],
//       int64 offsets[n_docs + 1], uint8 bytes[n_bytes],
//       int64 expect_offsets[n_docs + 1], int32 expect_ids[n_expect], int32 expect_word_ids[n_expect]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hutk_unigram.h"

namespace U = hutk::ug;

struct Reader {
    std::vector<uint8_t> raw;
    size_t at = 0;
    void need(size_t n) {
        if (at + n > raw.size()) {
            std::fprintf(stderr, "unigram_check: the case file is cut short\n");
            std::exit(2);
        }
    }
    int64_t i64() {
        int64_t v;
        need(8);
        std::memcpy(&v, raw.data() + at, 8);
        at += 8;
        return v;
    }
    template <class T>
    std::vector<T> take(size_t n) {  // (its own allocation: a read past it is caught)
        std::vector<T> v(n);
        need(sizeof(T) * n);
        if (n) std::memcpy(v.data(), raw.data() + at, sizeof(T) * n);
        at += sizeof(T) * n;
        return v;
    }
};

static std::vector<uint8_t> flags_of(const std::vector<int64_t>& offs, int64_t n) {
    std::vector<uint8_t> flag((size_t)n + 1, 0);
    for (size_t i = 0; i + 1 < offs.size(); i++) flag[(size_t)offs[i]] = 1;
    return flag;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: unigram_check CASE\n");
        return 2;
    }
    Reader in;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        in.raw.resize((size_t)n);
        const bool ok = n == 0 || std::fread(in.raw.data(), 1, (size_t)n, f) == (size_t)n;
        std::fclose(f);
        if (!ok) return 2;
    }
    const uint32_t flags = (uint32_t)in.i64();
    const int64_t chunk = in.i64(), unk_id = in.i64(), n_pieces = in.i64(), n_piece_bytes = in.i64(), n_docs = in.i64(), n_bytes = in.i64(),
                  n_expect = in.i64();
    if (chunk < U::SLICE_BYTES || chunk % U::SLICE_BYTES || n_docs < 0 || n_bytes < 0 || n_pieces < 0 || n_piece_bytes < 0 || n_expect < 0) return 2;
    const std::vector<int64_t> poffs = in.take<int64_t>((size_t)n_pieces + 1);
    const std::vector<double> scores = in.take<double>((size_t)n_pieces);
    const std::vector<uint8_t> pieces = in.take<uint8_t>((size_t)n_piece_bytes);
    const std::vector<int64_t> offs = in.take<int64_t>((size_t)n_docs + 1);
    const std::vector<uint8_t> bytes = in.take<uint8_t>((size_t)n_bytes);
    const std::vector<int64_t> want_oo = in.take<int64_t>((size_t)n_docs + 1);
    const std::vector<int32_t> want_ids = in.take<int32_t>((size_t)n_expect), want_wids = in.take<int32_t>((size_t)n_expect);
    bool sound = offs[0] == 0 && offs.back() == n_bytes;
    for (size_t i = 0; i + 1 < offs.size(); i++) sound = sound && offs[i + 1] >= offs[i];
    if (!sound) return 2;

    U::VocabHost vh;
    std::string why;
    if (U::build_vocab(pieces.data(), poffs.data(), scores.data(), n_pieces, unk_id, vh, &why)) {
        std::fprintf(stderr, "refused: %s\n", why.c_str());
        return 5;
    }
    const std::vector<uint8_t> keys(vh.keys);  // (exactly as long as the keys: the probe reads no byte behind them)
    const U::Vocab V = vh.view(vh.slots.data(), keys.data(), scores.data(), vh.lens.data(), (int32_t)unk_id);

    // k_ug_fold_count, the scan, k_ug_fold_write, k_ug_fold_docs
    const std::vector<uint8_t> flag = flags_of(offs, n_bytes);
    const U::Text x{bytes.data(), flag.data(), n_bytes};
    const int64_t slices = chunk / U::SLICE_BYTES, n_chunks = (n_bytes + chunk - 1) / chunk;
    std::vector<int64_t> base((size_t)n_chunks + 1, 0), slice((size_t)(n_chunks * slices), 0);
    int64_t total = 0;
    for (int64_t k = 0; k < n_chunks; k++) {
        int64_t sum = 0;
        for (int64_t t = 0; t < slices; t++) {
            const int64_t a = k * chunk + t * U::SLICE_BYTES, e = a + U::SLICE_BYTES < n_bytes ? a + U::SLICE_BYTES : n_bytes;
            slice[(size_t)(k * slices + t)] = sum;
            if (a < e) sum += U::fold_range(x, a, e, flags, nullptr);
        }
        base[(size_t)k] = total;
        total += sum;
    }
    base[(size_t)n_chunks] = total;
    if (total > n_bytes + n_docs) {
        std::fprintf(stderr, "the folded text holds %lld bytes, more than n_bytes + n_docs\n", (long long)total);
        return 1;
    }
    std::vector<uint8_t> folded((size_t)total);
    for (int64_t k = 0; k < n_chunks; k++)
        for (int64_t t = 0; t < slices; t++) {
            const int64_t a = k * chunk + t * U::SLICE_BYTES, e = a + U::SLICE_BYTES < n_bytes ? a + U::SLICE_BYTES : n_bytes;
            if (a >= e) continue;
            const int64_t to = base[(size_t)k] + slice[(size_t)(k * slices + t)];
            const int64_t n = U::fold_range(x, a, e, flags, nullptr);
            std::vector<uint8_t> piece((size_t)n + 1);  // (written on its own: a slice that writes more than it counted is caught)
            if (to + n > total || U::fold_range(x, a, e, flags, piece.data()) != n) return 4;
            std::memcpy(folded.data() + to, piece.data(), (size_t)n);
        }
    std::vector<int64_t> foffs((size_t)n_docs + 1, total);
    for (int64_t d = 0; d < n_docs; d++) {
        const int64_t o = offs[(size_t)d];
        if (o >= n_bytes) continue;
        const int64_t k = o / chunk, s0 = o & ~(int64_t)(U::SLICE_BYTES - 1);
        foffs[(size_t)d] = base[(size_t)k] + slice[(size_t)(k * slices + (s0 - k * chunk) / U::SLICE_BYTES)] + U::fold_range(x, s0, o, flags, nullptr);
    }
    const std::vector<uint8_t> fflag = flags_of(foffs, total);
    const U::Text f{folded.data(), fflag.data(), total};

    // k_ug_lattice: the word starts of a chunk, then its words
    std::vector<int32_t> tmp((size_t)total, -1);
    std::vector<U::Back> bp((size_t)total + 1, U::Back{-1, 0});
    const int R = U::ring_size(vh.max_len);
    std::vector<double> ring((size_t)R, std::nan(""));
    for (int64_t c0 = 0; c0 < total; c0 += chunk)
        for (int64_t p = c0; p < c0 + chunk && p < total; p++)
            if (U::word_starts(f, p)) {
                U::viterbi_word(V, f, p, ring.data(), R, bp.data(), tmp.data());
                for (double v : ring)
                    if (v == v) {
                        std::fprintf(stderr, "the ring is not empty behind the word at %lld\n", (long long)p);
                        return 1;
                    }
            }

    // k_ug_count .. k_ug_write
    std::vector<int32_t> ids, wids;
    std::vector<int64_t> oo((size_t)n_docs + 1, 0);
    int64_t d = 0, word = 0, word_base = 0;
    for (int64_t p = 0; p <= total; p++) {
        while (d <= n_docs && foffs[(size_t)d] == p) {
            if (d < n_docs) word_base = word;
            oo[(size_t)d++] = (int64_t)ids.size();
        }
        if (p == total) break;
        const int32_t v = tmp[(size_t)p];
        if (v < 0) continue;
        word += (v & U::ID_START) != 0;
        ids.push_back(v & U::ID_MASK);
        wids.push_back((int32_t)(word - 1 - word_base));
    }
    if ((int64_t)ids.size() > n_bytes + n_docs) {
        std::fprintf(stderr, "%zu ids, more than n_bytes + n_docs\n", ids.size());
        return 1;
    }
    if (oo != want_oo) {
        for (size_t i = 0; i < oo.size(); i++)
            if (oo[i] != want_oo[i]) {
                std::fprintf(stderr, "out_offsets[%zu] is %lld, expected %lld\n", i, (long long)oo[i], (long long)want_oo[i]);
                break;
            }
        return 1;
    }
    if ((int64_t)ids.size() != n_expect) {
        std::fprintf(stderr, "%zu ids, expected %lld\n", ids.size(), (long long)n_expect);
        return 1;
    }
    for (size_t i = 0; i < ids.size(); i++)
        if (ids[i] != want_ids[i] || wids[i] != want_wids[i]) {
            std::fprintf(stderr, "id %zu is %d (word %d), expected %d (word %d)\n", i, ids[i], wids[i], want_ids[i], want_wids[i]);
            return 1;
        }
    std::printf("folded %lld ids %zu\n", (long long)total, ids.size());
    return 0;
}
