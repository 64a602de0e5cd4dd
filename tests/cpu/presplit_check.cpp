// presplit_check -- the rule of hutoken_amd/csrc/hutk_presplit.h on the CPU, chunk by chunk as the kernels of
// hutk_presplit.hip run it (classify, per-slice maps, per-chunk maps, the scan over the chunks, the write pass), with the
// chunk size as an argument so that small texts cross many chunk edges.  Built with -fsanitize=address,undefined by
// tests/test_presplit_cpu.py and run as a program.
//
//   presplit_check run BLOB CASES CHUNK_BYTES    CASES: records of
//        u32 preset, u32 n_docs, u64 offsets[n_docs + 1], u8 bytes[n_bytes], u8 expected[n_bytes] (1: a word starts)
//     prints "cases N mismatches M" (and the first few that differ); exit status 0 when M == 0
//   presplit_check validate BLOB                 prints "ok" or "refused: why"; exit status 0 or 3
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "hutk_presplit.h"

namespace P = hutk::presplit;

static std::vector<uint8_t> read_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Chunk {
    std::vector<uint8_t> raw, code;
    std::vector<uint32_t> doc;
    P::Win W;
    int64_t c0, c1;
};

// what the kernels stage for one chunk: bytes, document bits and codes of [c0 - BACK, c0 + chunk + AHEAD)
static void stage(const P::Tables& T, const uint8_t* bytes, const std::vector<int64_t>& offs, int64_t n_bytes, int64_t k, int chunk, Chunk& C) {
    const int len = P::BACK + chunk + P::AHEAD;
    C.c0 = k * chunk;
    C.c1 = C.c0 + chunk < n_bytes ? C.c0 + chunk : n_bytes;
    const int64_t w0 = C.c0 - P::BACK;
    C.raw.assign((size_t)len, 0);
    C.code.assign((size_t)len, 0);
    C.doc.assign((size_t)(len + 31) / 32, 0);
    for (int i = 0; i < len; i++)
        if (w0 + i >= 0 && w0 + i < n_bytes) C.raw[(size_t)i] = bytes[w0 + i];
    for (int64_t o : offs)
        if (o >= w0 && o < w0 + len) C.doc[(size_t)((o - w0) >> 5)] |= 1u << ((o - w0) & 31);
    C.W = P::Win{C.raw.data(), C.code.data(), C.doc.data()};
    for (int64_t p = C.c0 - P::CLS_HALO; p < C.c0 + chunk + P::CLS_HALO; p++)
        if (p >= 0 && p < n_bytes) C.code[(size_t)(p - w0)] = (uint8_t)P::classify_byte(T, C.W, (int)(p - w0));
}

static std::vector<uint8_t> split(const P::Tables& T, int preset, const uint8_t* bytes, const std::vector<int64_t>& offs, int chunk) {
    const int64_t n_bytes = offs.back();
    const int64_t n_chunks = n_bytes / chunk + 1;
    const int slices = chunk / P::SLICE_BYTES;
    std::vector<uint32_t> maps((size_t)n_chunks), carry((size_t)n_chunks, P::carry_pack(P::F_NONE, 0));
    Chunk C;
    auto slice_range = [&](int s, int& i0, int& n) {
        const int64_t at = C.c0 + (int64_t)s * P::SLICE_BYTES;
        i0 = P::BACK + s * P::SLICE_BYTES;
        n = at >= C.c1 ? 0 : C.c1 - at < P::SLICE_BYTES ? (int)(C.c1 - at) : P::SLICE_BYTES;
    };
    if (preset != P::PRESET_GPT2) {
        for (int64_t k = 0; k < n_chunks; k++) {  // the carry pass
            stage(T, bytes, offs, n_bytes, k, chunk, C);
            uint32_t f = P::FMAP_IDENT, b = P::BMAP_IDENT;
            for (int s = 0; s < slices; s++) {
                int i0, n;
                slice_range(s, i0, n);
                f = P::fmap_then(f, P::slice_fmap(C.W, i0, i0 + n));
            }
            for (int s = slices - 1; s >= 0; s--) {
                int i0, n;
                slice_range(s, i0, n);
                b = P::bmap_then(b, P::slice_bmap(C.W, i0, i0 + n));
            }
            maps[(size_t)k] = P::maps_pack(f, b);
        }
        uint32_t fs = P::F_NONE, bv = 0;  // the scan over the chunks
        for (int64_t k = 0; k < n_chunks; k++) {
            carry[(size_t)k] = fs;
            fs = P::fmap_get(maps[(size_t)k] & 0xFFFFu, fs);
        }
        for (int64_t k = n_chunks - 1; k >= 0; k--) {
            carry[(size_t)k] = P::carry_pack(carry[(size_t)k], bv);
            bv = P::bmap_get(maps[(size_t)k] >> 16, bv);
        }
    }
    std::vector<uint8_t> out((size_t)n_bytes, 0);
    for (int64_t k = 0; k < n_chunks; k++) {  // the write pass
        stage(T, bytes, offs, n_bytes, k, chunk, C);
        std::vector<uint32_t> fin((size_t)slices), bin((size_t)slices);
        uint32_t f = carry[(size_t)k] & 0xFFu, b = carry[(size_t)k] >> 8;
        for (int s = 0; s < slices; s++) {
            int i0, n;
            slice_range(s, i0, n);
            fin[(size_t)s] = f;
            f = P::fmap_get(P::slice_fmap(C.W, i0, i0 + n), f);
        }
        for (int s = slices - 1; s >= 0; s--) {
            int i0, n;
            slice_range(s, i0, n);
            bin[(size_t)s] = b;
            b = P::bmap_get(P::slice_bmap(C.W, i0, i0 + n), b);
        }
        for (int s = 0; s < slices; s++) {
            int i0, n;
            slice_range(s, i0, n);
            const uint32_t bits = P::slice_starts(C.W, preset, i0, n, fin[(size_t)s], bin[(size_t)s]);
            for (int j = 0; j < n; j++) out[(size_t)(C.c0 + s * P::SLICE_BYTES + j)] = (bits >> j) & 1u;
        }
    }
    return out;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: presplit_check run BLOB CASES CHUNK_BYTES | validate BLOB\n");
        return 2;
    }
    const std::vector<uint8_t> blob = read_file(argv[2]);
    uint32_t head[P::HEADER_WORDS];
    std::string why;
    const bool ok = P::validate_blob(blob.data(), (int64_t)blob.size(), head, &why);
    if (std::strcmp(argv[1], "validate") == 0) {
        std::printf("%s\n", ok ? "ok" : ("refused: " + why).c_str());
        return ok ? 0 : 3;
    }
    if (!ok || argc < 5) {
        std::fprintf(stderr, "bad blob or arguments: %s\n", why.c_str());
        return 2;
    }
    // (the sections are read in place: copy them to aligned storage of their own type)
    std::vector<uint16_t> stage1(P::STAGE1_N);
    std::vector<uint32_t> blocks((size_t)head[P::H_BLOCKS_N] * P::BLOCK_WORDS);
    std::memcpy(stage1.data(), blob.data() + head[P::H_STAGE1_OFF], stage1.size() * 2);
    std::memcpy(blocks.data(), blob.data() + head[P::H_BLOCKS_OFF], blocks.size() * 4);
    const P::Tables T{stage1.data(), blocks.data()};
    const std::vector<uint8_t> cases = read_file(argv[3]);
    const int chunk = std::atoi(argv[4]);
    if (chunk < 32 || chunk % 32) {
        std::fprintf(stderr, "CHUNK_BYTES must be a multiple of 32\n");
        return 2;
    }
    size_t at = 0;
    long n_cases = 0, bad = 0;
    auto need = [&](size_t n) {
        if (cases.size() - at < n) {
            std::fprintf(stderr, "truncated case file\n");
            std::exit(2);
        }
    };
    while (at < cases.size()) {
        need(8);
        uint32_t preset, n_docs;
        std::memcpy(&preset, &cases[at], 4);
        std::memcpy(&n_docs, &cases[at + 4], 4);
        at += 8;
        need(8 * ((size_t)n_docs + 1));
        std::vector<int64_t> offs((size_t)n_docs + 1);
        std::memcpy(offs.data(), &cases[at], 8 * offs.size());
        at += 8 * offs.size();
        const size_t n = (size_t)offs.back();
        need(2 * n);
        const std::vector<uint8_t> bytes(cases.begin() + (long)at, cases.begin() + (long)(at + n));  // (a copy: exact bounds)
        const uint8_t* want = cases.data() + at + n;
        at += 2 * n;
        const std::vector<uint8_t> got = split(T, (int)preset, bytes.data(), offs, chunk);
        n_cases++;
        if (n && std::memcmp(got.data(), want, n) != 0) {
            if (++bad <= 5) {
                std::printf("case %ld preset %u:", n_cases - 1, preset);
                for (size_t i = 0; i < n; i++) std::printf(" %02x%s", bytes[i], got[i] != want[i] ? (got[i] ? "[+]" : "[-]") : want[i] ? "|" : "");
                std::printf("\n");
            }
        }
    }
    std::printf("cases %ld mismatches %ld\n", n_cases, bad);
    return bad ? 1 : 0;
}
