// norm_check.cpp -- the normaliser of hutoken_amd/csrc/hutk_norm.h on the CPU (tests/test_normalize_cpu.py builds this
// with -fsanitize=address,undefined and runs it as a child process).  The kernels of hutk_normalize.hip call the same
// functions; what is restated here is only their orchestration: a chunk's byte test, its slices in order, the scan.
//
//   norm_check validate BLOB            exit 0: the blob is accepted; exit 3 and a message: refused
//   norm_check chunk                    prints the chunk size
//   norm_check run BLOB CASE PREFIX     the packed batch of CASE under all four forms -> PREFIX.0 .. PREFIX.3
//
// CASE:   int64 n_docs, int64 n_bytes, int64 offsets[n_docs + 1], uint8 bytes[n_bytes]
// result: int64 total, int64 out_offsets[n_docs + 1], uint8 changed[n_docs], uint8 bytes[total]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hutk_norm.h"

namespace N = hutk::norm;

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

static bool has_high(const N::Text& x, int64_t a, int64_t e) {
    for (int64_t p = a; p < e; p++)
        if (x.bytes[p] >= x.lead) return true;
    return false;
}

struct Result {
    std::vector<int64_t> out_offs;
    std::vector<uint8_t> changed, out;
};

// what k_norm_sizes, the scan, k_norm_docs and k_norm_write do, chunk by chunk and slice by slice
static void run(const N::Tables& T, const N::Text& x, Result& r) {
    const int64_t n_chunks = (x.n_bytes + N::CHUNK_BYTES - 1) / N::CHUNK_BYTES;
    r.out_offs.assign((size_t)x.n_docs + 1, 0);
    r.changed.assign((size_t)x.n_docs, 0);
    std::vector<int64_t> base((size_t)n_chunks + 1, 0);
    std::vector<uint8_t> clean((size_t)n_chunks, 0);
    std::vector<int> sp((size_t)n_chunks + 1, 0);
    for (int pass = 0; pass < 2; pass++) {
        for (int64_t k = 0; k < n_chunks; k++) {
            const int64_t c0 = k * N::CHUNK_BYTES, c1 = c0 + N::CHUNK_BYTES < x.n_bytes ? c0 + N::CHUNK_BYTES : x.n_bytes;
            const int64_t dlo = N::first_doc_at_or_after(x.offs, x.n_docs, c0), dhi = N::first_doc_at_or_after(x.offs, x.n_docs, c1);
            if (pass == 0) {
                const int sp0 = N::edge_spill(x, c0, dlo), sp1 = N::edge_spill(x, c1, dhi);
                bool dirty = c1 + sp1 < x.n_bytes && x.bytes[c1 + sp1] >= x.lead;
                for (int64_t p = c0; p < c1; p++) dirty = dirty || x.bytes[p] >= x.lead;
                sp[(size_t)k] = sp0;
                clean[(size_t)k] = !dirty;
                if (!dirty) {
                    base[(size_t)k] = (c1 + sp1) - (c0 + sp0);
                    for (int64_t d = dlo; d < dhi; d++) r.out_offs[(size_t)d] = x.offs[d] - (c0 + sp0);
                    continue;
                }
                int64_t excl[N::CHUNK_SLICES + 1];
                std::vector<uint16_t> emit(N::CHUNK_BYTES, 0xFFFF);
                int64_t sum = 0;
                for (int t = 0; t < N::CHUNK_SLICES; t++) {
                    excl[t] = sum;
                    const int64_t a = c0 + (int64_t)t * N::SLICE_BYTES, e = a + N::SLICE_BYTES < c1 ? a + N::SLICE_BYTES : c1;
                    if (a >= c1) continue;
                    N::CountSink sink;
                    N::slice_run(T, x, N::doc_of_byte(x.offs, dlo, dhi, a), a, e, has_high(x, a, e), sink,
                                 [&](int64_t p, int64_t before) { emit[(size_t)(p - c0)] = (uint16_t)before; }, r.changed.data());
                    sum += sink.pos;
                }
                base[(size_t)k] = sum;
                for (int64_t d = dlo; d < dhi; d++) {
                    const int64_t i = x.offs[d] - c0;
                    if (emit[(size_t)i] == 0xFFFF) {
                        std::fprintf(stderr, "norm_check: document %lld starts at no segment start\n", (long long)d);
                        std::exit(4);
                    }
                    r.out_offs[(size_t)d] = excl[i / N::SLICE_BYTES] + emit[(size_t)i];
                }
            } else {
                if (clean[(size_t)k]) {
                    const int64_t from = c0 + sp[(size_t)k], n = base[(size_t)k + 1] - base[(size_t)k];
                    for (int64_t i = 0; i < n; i++) r.out[(size_t)(base[(size_t)k] + i)] = x.bytes[from + i];
                    continue;
                }
                int64_t at = base[(size_t)k];
                for (int t = 0; t < N::CHUNK_SLICES; t++) {
                    const int64_t a = c0 + (int64_t)t * N::SLICE_BYTES, e = a + N::SLICE_BYTES < c1 ? a + N::SLICE_BYTES : c1;
                    if (a >= c1) continue;
                    N::WriteSink sink{r.out.data(), (int64_t)r.out.size(), at};
                    N::slice_run(T, x, N::doc_of_byte(x.offs, dlo, dhi, a), a, e, has_high(x, a, e), sink, [](int64_t, int64_t) {}, nullptr);
                    at = sink.pos;
                }
                if (at != base[(size_t)k + 1]) {
                    std::fprintf(stderr, "norm_check: chunk %lld wrote %lld bytes, counted %lld\n", (long long)k,
                                 (long long)(at - base[(size_t)k]), (long long)(base[(size_t)k + 1] - base[(size_t)k]));
                    std::exit(4);
                }
            }
        }
        if (pass == 0) {
            int64_t sum = 0;
            for (int64_t k = 0; k <= n_chunks; k++) {
                const int64_t v = k < n_chunks ? base[(size_t)k] : 0;
                base[(size_t)k] = sum;
                sum += v;
            }
            const int64_t total = base[(size_t)n_chunks];
            for (int64_t d = 0; d < x.n_docs; d++)
                r.out_offs[(size_t)d] = x.offs[d] >= x.n_bytes ? total : base[(size_t)(x.offs[d] / N::CHUNK_BYTES)] + r.out_offs[(size_t)d];
            r.out_offs[(size_t)x.n_docs] = total;
            r.out.assign((size_t)total, 0);
        }
    }
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "chunk") {
        std::printf("%d\n", N::CHUNK_BYTES);
        return 0;
    }
    if (argc < 3) {
        std::fprintf(stderr, "usage: norm_check validate BLOB | chunk | run BLOB CASE PREFIX\n");
        return 2;
    }
    std::vector<uint8_t> blob;
    if (!read_file(argv[2], blob)) {
        std::fprintf(stderr, "norm_check: cannot read %s\n", argv[2]);
        return 2;
    }
    uint32_t h[N::HEADER_WORDS];
    std::string why;
    if (!N::validate_blob(blob.data(), (int64_t)blob.size(), h, &why)) {
        std::fprintf(stderr, "refused: %s\n", why.c_str());
        return 3;
    }
    if (std::string(argv[1]) == "validate") return 0;
    if (std::string(argv[1]) != "run" || argc != 5) return 2;
    const N::Tables T = N::tables_of(blob.data(), h);
    std::vector<uint8_t> raw;
    if (!read_file(argv[3], raw) || raw.size() < 16) return 2;
    int64_t n_docs, n_bytes;
    std::memcpy(&n_docs, raw.data(), 8);
    std::memcpy(&n_bytes, raw.data() + 8, 8);
    if (n_docs < 0 || n_bytes < 0 || raw.size() != 16 + 8 * ((size_t)n_docs + 1) + (size_t)n_bytes) return 2;
    std::vector<int64_t> offs((size_t)n_docs + 1);
    std::memcpy(offs.data(), raw.data() + 16, 8 * offs.size());
    std::vector<uint8_t> bytes(raw.begin() + 16 + 8 * (long)offs.size(), raw.end());  // (its own allocation: a read past it is caught)
    if (offs[0] != 0 || offs[(size_t)n_docs] != n_bytes) return 2;
    for (int64_t i = 0; i < n_docs; i++)
        if (offs[(size_t)i + 1] < offs[(size_t)i]) return 2;
    for (int form = 0; form < N::N_FORMS; form++) {
        N::Text x{bytes.data(), offs.data(), n_docs, n_bytes, h[N::H_LEAD + form], form};
        Result r;
        run(T, x, r);
        const std::string path = std::string(argv[4]) + "." + std::to_string(form);
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f) return 2;
        const int64_t total = (int64_t)r.out.size();
        std::fwrite(&total, 8, 1, f);
        std::fwrite(r.out_offs.data(), 8, r.out_offs.size(), f);
        if (!r.changed.empty()) std::fwrite(r.changed.data(), 1, r.changed.size(), f);
        if (!r.out.empty()) std::fwrite(r.out.data(), 1, r.out.size(), f);
        std::fclose(f);
    }
    return 0;
}
