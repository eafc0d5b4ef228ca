// clip_bits_check.cpp -- kh_clip_beats of krust_amd/csrc/unitig_bits.h (what clip_decide_kernel runs per rival) on a grid of KMERS
// values, count sums (0, 2^32 and 2^64 - 1 among them), both candidate flags and equal and unequal indices: one line per point,
// "kmers_b sum_b idx_b cand_b kmers_i sum_i idx_i result", which tests/test_clip_bits.py holds to the comparator in Python.  Pure
// host code with its own main: compiled and run there (once more with -fsanitize=address,undefined), no device and no library needed.
#include <cstdio>

#include "../krust_amd/csrc/unitig_bits.h"

int main() {
    const uint64_t kmers[] = {1, 2, 21, 22, 1ull << 32, ~0ull};
    const uint64_t sums[] = {0, 1, 1ull << 32, (1ull << 32) + 1, ~0ull};
    const uint32_t idx[][2] = {{0, 1}, {1, 0}, {5, 5}, {0x7FFFFFFEu, 3}};
    unsigned long long lines = 0;
    for (uint64_t kb : kmers)
        for (uint64_t sb : sums)
            for (uint64_t ki : kmers)
                for (uint64_t si : sums)
                    for (const auto &ix : idx)
                        for (int cb = 0; cb < 2; ++cb) {
                            printf("%llu %llu %u %d %llu %llu %u %d\n", (unsigned long long)kb, (unsigned long long)sb, ix[0], cb, (unsigned long long)ki,
                                   (unsigned long long)si, ix[1], kh_clip_beats(kb, sb, ix[0], cb != 0, ki, si, ix[1]) ? 1 : 0);
                            ++lines;
                        }
    printf("clip_bits_check ok %llu\n", lines);
    return 0;
}
