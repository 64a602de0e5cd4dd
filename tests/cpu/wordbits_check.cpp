// wordbits_check.cpp -- host check of the start-bit arithmetic of k_tiles' word rounds (hutoken_amd/csrc/hutk_wordbits.h)
// against a loop over the positions, on random 32-bit patterns of every density.  Built with
// -fsanitize=address,undefined and run on the host.
//   wordbits_check <n_patterns> <seed>
#include <cstdio>
#include <cstdlib>

#include "hutk_wordbits.h"

using namespace hutk;

namespace {

uint64_t rng_state;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

bool bit(uint32_t f, int p) { return p < 32 && ((f >> p) & 1u); }

template <int KEY>
long check(uint32_t f32) {
    long bad = 0;
    uint32_t one = 0, within = 0;
    for (int j = 0; j < 16; j++) {
        if (bit(f32, j + 1)) one |= 1u << j;
        for (int d = 1; d <= KEY; d++)
            if (bit(f32, j + d)) within |= 1u << j;
    }
    bad += wb::one_byte(f32) != one;
    bad += wb::within<KEY>(f32) != within;
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 100000;
    rng_state = argc > 2 ? (uint64_t)atoll(argv[2]) : 1;
    long bad = 0;
    for (long i = 0; i < n; i++) {
        uint32_t f = rnd();
        switch (i & 3) {  // dense, even, sparse, very sparse
            case 0: f |= rnd(); break;
            case 2: f &= rnd(); break;
            case 3: f &= rnd() & rnd() & rnd(); break;
        }
        bad += check<12>(f) + check<14>(f) + check<9>(f) + check<16>(f);
    }
    for (int p = 0; p < 32; p++) bad += check<12>(1u << p) + check<14>(1u << p);  // a single start at every position
    bad += check<14>(0u) + check<14>(~0u);
    printf("patterns %ld mismatches %ld\n", n, bad);
    return bad != 0;
}
