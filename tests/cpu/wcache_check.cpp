// wcache_check.cpp -- host fuzz of the word cache's slot layout, key packing and hash (hutoken_amd/csrc/hutk_wcache.h)
// with a host model of what the kernels do with them: insert as k_finish's d_learn does (claim a slot through its tag
// word, first slot of the bucket, then the second, else drop), look up as k_tiles does (both slots of the bucket, the
// whole key and the length compared).  Built with -fsanitize=address,undefined and run on the host.
//   wcache_check <n_keys> <seed> <log2_buckets>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "hutk_wcache.h"

using namespace hutk;

namespace {

uint64_t rng_state;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

struct Table {
    uint32_t log2;
    std::vector<wc::Slot> slots;
    std::vector<uint32_t> tags;
    uint32_t entries = 0;
    explicit Table(uint32_t l) : log2(l), slots((size_t)2 << l), tags((size_t)2 << l, 0u) {
        for (auto& s : slots) memset(&s, 0, sizeof s);
    }
    // d_learn: 1 inserted, 0 listed twice (its tag is there), -1 dropped (bucket full), -2 not cacheable
    int insert(const wc::Slot& cand) {
        uint32_t k[wc::KEY_DWORDS];
        for (int j = 0; j < wc::KEY_DWORDS; j++) k[j] = cand.w[j];
        if (!wc::cacheable(wc::slot_nb(cand.w[7]), wc::slot_n(cand.w[7]))) return -2;
        const uint32_t h = wc::hash(k), tag = wc::tag_of(k), slot0 = 2u * wc::bucket_of(h, log2);
        for (uint32_t s = slot0; s < slot0 + 2u; s++) {
            if (tags[s] == 0u) {  // (the compare-and-swap)
                tags[s] = tag;
                slots[s] = cand;
                entries++;
                return 1;
            }
            if (tags[s] == tag) return 0;
        }
        return -1;
    }
    // k_tiles: the key from nine dwords read at the word's first byte (whatever follows the word in them), both slots
    const wc::Slot* lookup(const uint8_t* bytes_with_tail, int nb) const {
        if (nb < wc::MIN_BYTES || nb > wc::KEY_BYTES) return nullptr;
        uint32_t k[wc::KEY_DWORDS];
        memcpy(k, bytes_with_tail, sizeof k);
        wc::make_key(k, nb);
        const uint32_t slot0 = 2u * wc::bucket_of(wc::hash(k), log2);
        for (uint32_t s = slot0; s < slot0 + 2u; s++) {
            uint32_t sk[wc::KEY_DWORDS];
            for (int j = 0; j < wc::KEY_DWORDS; j++) sk[j] = slots[s].w[j];
            if (wc::key_hit(sk, k)) return &slots[s];
        }
        return nullptr;
    }
};

int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            if (fails++ < 20) printf("line %d: %s\n", __LINE__, #c); \
        }                                                            \
    } while (0)

struct Word {
    std::string bytes;
    std::vector<uint16_t> syms;
};

Word random_word(int nb_lo, int nb_hi, int alphabet) {
    Word w;
    const int nb = nb_lo + (int)(rnd() % (uint32_t)(nb_hi - nb_lo + 1));
    for (int i = 0; i < nb; i++) w.bytes.push_back((char)(1 + rnd() % (uint32_t)alphabet));  // (no 0x00: the input has none)
    const int n_max = nb < wc::MAX_IDS ? nb : wc::MAX_IDS;
    const int n = 1 + (int)(rnd() % (uint32_t)n_max);
    for (int i = 0; i < n; i++) w.syms.push_back((uint16_t)(rnd() % 0xFFF0u));
    return w;
}

// the word's bytes followed by 40 bytes of other text, as the kernel's nine-dword read sees them
std::vector<uint8_t> with_tail(const std::string& s) {
    std::vector<uint8_t> v(s.begin(), s.end());
    for (int i = 0; i < 40; i++) v.push_back((uint8_t)(1 + rnd() % 255u));
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    const int n_keys = argc > 1 ? atoi(argv[1]) : 20000;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    const uint32_t log2 = argc > 3 ? (uint32_t)atoi(argv[3]) : 10;

    // 1. pack / unpack round trip, and the limits on both sides
    for (int it = 0; it < n_keys; it++) {
        const Word w = random_word(2, 30, 255);
        wc::Slot s;
        CHECK(wc::pack(s, (const uint8_t*)w.bytes.data(), (int)w.bytes.size(), w.syms.data(), (int)w.syms.size()));
        uint8_t b[32];
        uint16_t y[16];
        int nb = 0, n = 0;
        CHECK(wc::unpack(s, b, &nb, y, &n));
        CHECK(nb == (int)w.bytes.size() && n == (int)w.syms.size());
        CHECK(memcmp(b, w.bytes.data(), (size_t)nb) == 0 && memcmp(y, w.syms.data(), (size_t)n * 2) == 0);
        // the key the kernel builds from the text equals the packed one
        const std::vector<uint8_t> t = with_tail(w.bytes);
        uint32_t k[wc::KEY_DWORDS];
        memcpy(k, t.data(), sizeof k);
        wc::make_key(k, nb);
        for (int j = 0; j < 7; j++) CHECK(k[j] == s.w[j]);
        CHECK(k[7] == (s.w[7] & 0x00FFFFFFu));
    }
    {
        wc::Slot s;
        memset(&s, 0xAB, sizeof s);
        const wc::Slot before = s;
        uint8_t bytes[40];
        uint16_t syms[40];
        for (int i = 0; i < 40; i++) { bytes[i] = (uint8_t)('a' + i % 26); syms[i] = (uint16_t)i; }
        CHECK(!wc::pack(s, bytes, 31, syms, 5));   // 31 bytes
        CHECK(!wc::pack(s, bytes, 1, syms, 1));    // 1 byte
        CHECK(!wc::pack(s, bytes, 30, syms, 17));  // 17 ids
        CHECK(!wc::pack(s, bytes, 30, syms, 0));   // no id
        CHECK(!wc::pack(s, bytes, 4, syms, 5));    // more ids than bytes
        CHECK(memcmp(&s, &before, sizeof s) == 0);
        CHECK(wc::pack(s, bytes, 30, syms, 16) && wc::pack(s, bytes, 2, syms, 2) && wc::pack(s, bytes, 2, syms, 1));
        CHECK(wc::cacheable(30, 16) && !wc::cacheable(31, 16) && !wc::cacheable(30, 17) && !wc::cacheable(1, 1));
        // a record that claims a length or a count beyond the limits is refused by the inserter and by the reader
        Table t(2);
        CHECK(wc::pack(s, bytes, 30, syms, 16));
        wc::Slot bad = s;
        bad.w[7] = (bad.w[7] & 0x0000FFFFu) | (31u << 16) | (16u << 24);
        CHECK(t.insert(bad) == -2);
        bad.w[7] = (s.w[7] & 0x00FFFFFFu) | (17u << 24);
        CHECK(t.insert(bad) == -2);
        CHECK(t.entries == 0);
        uint32_t k[wc::KEY_DWORDS], sk[wc::KEY_DWORDS];
        for (int j = 0; j < wc::KEY_DWORDS; j++) { k[j] = s.w[j]; sk[j] = bad.w[j]; }
        CHECK(!wc::key_hit(sk, k));  // (17 ids in the slot)
        for (int j = 0; j < wc::KEY_DWORDS; j++) sk[j] = 0;
        uint32_t zero[wc::KEY_DWORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
        CHECK(!wc::key_hit(sk, zero));  // an empty slot matches nothing, not even an all-zero key
    }

    // 2. a table under load: a lookup returns the word's own result or nothing
    {
        Table t(log2);
        std::map<std::string, Word> truth;
        std::vector<Word> words;
        int dropped = 0;
        for (int it = 0; it < n_keys; it++) {
            Word w = random_word(2, 30, it % 3 == 0 ? 3 : 255);  // (a small alphabet: many prefixes of one another)
            if (it % 7 == 0 && !words.empty()) {  // a zero-padded prefix of an earlier word, and one byte more of it
                const Word& o = words[rnd() % words.size()];
                if (o.bytes.size() > 2) {
                    w.bytes = o.bytes.substr(0, 2 + rnd() % (o.bytes.size() - 2));
                    if (w.syms.size() > w.bytes.size()) w.syms.resize(w.bytes.size());
                }
            }
            if (truth.count(w.bytes)) w = truth[w.bytes];  // (a word has one encoding)
            wc::Slot s;
            CHECK(wc::pack(s, (const uint8_t*)w.bytes.data(), (int)w.bytes.size(), w.syms.data(), (int)w.syms.size()));
            const uint32_t entries_before = t.entries;
            const std::vector<wc::Slot> snapshot = it % 64 == 0 ? t.slots : std::vector<wc::Slot>();
            const int r = t.insert(s);
            CHECK(r >= -1);
            if (r == 1) truth[w.bytes] = w;
            if (r != 1) CHECK(t.entries == entries_before);
            if (r == -1) {
                dropped++;
                if (!snapshot.empty()) CHECK(memcmp(snapshot.data(), t.slots.data(), snapshot.size() * sizeof(wc::Slot)) == 0);  // nothing overwritten
            }
            CHECK(t.entries <= t.slots.size());
            words.push_back(w);
        }
        size_t hits = 0;
        for (const Word& w : words) {
            const std::vector<uint8_t> text = with_tail(w.bytes);
            const wc::Slot* s = t.lookup(text.data(), (int)w.bytes.size());
            if (!s) continue;
            hits++;
            uint8_t b[32];
            uint16_t y[16];
            int nb = 0, n = 0;
            CHECK(wc::unpack(*s, b, &nb, y, &n));
            CHECK(nb == (int)w.bytes.size() && memcmp(b, w.bytes.data(), (size_t)nb) == 0);
            const Word& tw = truth[w.bytes];
            CHECK(n == (int)tw.syms.size() && memcmp(y, tw.syms.data(), (size_t)n * 2) == 0);
            // the same bytes asked for with another length: a different key
            if (nb > 2) {
                const wc::Slot* p = t.lookup(text.data(), nb - 1);
                if (p) CHECK(wc::slot_nb(p->w[7]) == nb - 1);
            }
            if (nb < 30) {
                const wc::Slot* p = t.lookup(text.data(), nb + 1);
                if (p) CHECK(wc::slot_nb(p->w[7]) == nb + 1 && memcmp(p->w, text.data(), (size_t)nb + 1) == 0);
            }
        }
        // every inserted word is found
        for (auto& kv : truth) {
            const std::vector<uint8_t> text = with_tail(kv.first);
            CHECK(t.lookup(text.data(), (int)kv.first.size()) != nullptr);
        }
        CHECK(t.lookup((const uint8_t*)"abcdefghijklmnopqrstuvwxyzabcdefghijklmnopqrstuvwxyz", 31) == nullptr);
        CHECK(t.lookup((const uint8_t*)"abcdefghijklmnopqrstuvwxyzabcdefghijklmnopqrstuvwxyz", 1) == nullptr);
        printf("keys %d entries %u of %zu dropped %d hits %zu\n", n_keys, t.entries, t.slots.size(), dropped, hits);
    }

    // 3. a full bucket drops: one bucket (log2 = 0), three distinct words
    {
        Table t(0);
        int placed = 0, dropped = 0;
        for (int it = 0; it < 50; it++) {
            const Word w = random_word(2, 30, 255);
            wc::Slot s;
            wc::pack(s, (const uint8_t*)w.bytes.data(), (int)w.bytes.size(), w.syms.data(), (int)w.syms.size());
            const std::vector<wc::Slot> snapshot = t.slots;
            const int r = t.insert(s);
            placed += r == 1;
            dropped += r == -1;
            if (r != 1) CHECK(memcmp(snapshot.data(), t.slots.data(), snapshot.size() * sizeof(wc::Slot)) == 0);
        }
        CHECK(placed == 2 && t.entries == 2 && dropped >= 47);
    }
    printf("mismatches %d\n", fails);
    return fails ? 1 : 0;
}
