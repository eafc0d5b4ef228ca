// pop_bits_check.cpp -- kh_pop_beats of krust_amd/csrc/unitig_bits.h (what pop_decide_kernel runs per parallel candidate) and the
// 64 x 64 -> 128 product under it: a grid of KMERS values (1 .. 2^31 - 1) and count sums (0, 2^32, 2^63 and 2^64 - 1 among them, so
// that the products pass 2^64 and the sums compare as stored), pairs whose products are EQUAL with different KMERS, full ties, and
// random triples (KMERS, COUNT_SUM, index) from a fixed generator.  One line per pair, both directions:
// "kmers_b sum_b idx_b kmers_i sum_i idx_i beats(b, i) beats(i, b)", and first "mul a b hi lo" lines for the product itself;
// tests/test_pop_bits.py holds all of it to Python integers.  Pure host code with its own main: compiled and run there (once more
// with -fsanitize=address,undefined), no device and no library needed.
#include <cstdio>

#include "../krust_amd/csrc/unitig_bits.h"

static unsigned long long lines = 0;

static void pair(uint64_t kb, uint64_t sb, uint32_t ib, uint64_t ki, uint64_t si, uint32_t ii) {
    printf("%llu %llu %u %llu %llu %u %d %d\n", (unsigned long long)kb, (unsigned long long)sb, ib, (unsigned long long)ki, (unsigned long long)si, ii,
           kh_pop_beats(kb, sb, ib, ki, si, ii) ? 1 : 0, kh_pop_beats(ki, si, ii, kb, sb, ib) ? 1 : 0);
    ++lines;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    const uint64_t kmers[] = {1, 2, 3, 21, 42, 0x7FFFFFFEull, 0x7FFFFFFFull};
    const uint64_t sums[] = {0, 1, 6, 1ull << 32, (1ull << 32) + 1, 1ull << 63, ~0ull - 1, ~0ull};
    const uint64_t factors[] = {0, 1, 3, 0xFFFFFFFFull, 1ull << 32, (1ull << 32) + 1, 0x7FFFFFFFull, 1ull << 63, ~0ull - 1, ~0ull};
    for (uint64_t a : factors)
        for (uint64_t b : factors) {
            uint64_t hi, lo;
            kh_mul_64x64(a, b, &hi, &lo);
            printf("mul %llu %llu %llu %llu\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)hi, (unsigned long long)lo);
        }
    const uint32_t idx[][2] = {{0, 1}, {1, 0}, {0x7FFFFFFEu, 3}};
    for (uint64_t kb : kmers)
        for (uint64_t sb : sums)
            for (uint64_t ki : kmers)
                for (uint64_t si : sums)
                    for (const auto &ix : idx) pair(kb, sb, ix[0], ki, si, ix[1]);
    // equal products, different KMERS: sum = m * kmers on both sides, up to products past 2^64
    const uint64_t means[] = {0, 1, 5, 1ull << 31, (1ull << 33) - 1};
    for (uint64_t m : means)
        for (uint64_t kb : kmers)
            for (uint64_t ki : kmers) {
                pair(kb, m * kb, 7, ki, m * ki, 4);
                pair(kb, m * kb, 4, ki, m * ki, 7);
            }
    // random triples: all 64 bits of the sum, KMERS below 2^31, and short ranges where ties happen
    for (int r = 0; r < 4000; ++r) {
        const bool tight = (r & 1) != 0;
        const uint64_t kb = tight ? 1 + rnd() % 4 : 1 + rnd() % 0x7FFFFFFFull, ki = tight ? 1 + rnd() % 4 : 1 + rnd() % 0x7FFFFFFFull;
        const uint64_t sb = tight ? rnd() % 12 : rnd(), si = tight ? rnd() % 12 : rnd();
        const uint32_t ib = (uint32_t)(rnd() % 0x7FFFFFFFull), ii = (uint32_t)(rnd() % 0x7FFFFFFFull);
        pair(kb, sb, ib, ki, si, ib == ii ? ii ^ 1u : ii);
    }
    printf("pop_bits_check ok %llu\n", lines);
    return 0;
}
