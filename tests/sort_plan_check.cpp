// CPU check of the radix sort's pass plan (krust_amd/csrc/sort.hip.h: sort_passes / sort_pass_shift / sort_pass_bits; built and run by
// tests/test_sort_plan.py; no GPU, no HIP): for every k = 1..32 the passes cover the bits 0 .. 2k - 1 of a key exactly once, no bit
// at or above 2k, in ascending order (an LSD sort takes the least significant digit first), with at most SORT_DIGIT_BITS bits each,
// and there are ceil(2k / 8) of them -- the number sort.hip.h documents.
#include <cstdio>

#define KH_SORT_HOST_ONLY 1
#include "../krust_amd/csrc/sort.hip.h"

int main() {
    int failures = 0;
    for (uint32_t k = 1; k <= 32; ++k) {
        const uint32_t passes = kh::sort_passes(k);
        if (passes != (2 * k + 7) / 8) {
            printf("FAIL k=%u: %u passes, documented %u\n", k, passes, (2 * k + 7) / 8);
            ++failures;
        }
        uint32_t seen[64] = {0};
        uint32_t next = 0;
        for (uint32_t p = 0; p < passes; ++p) {
            const uint32_t shift = kh::sort_pass_shift(k, p), bits = kh::sort_pass_bits(k, p);
            if (bits < 1 || bits > kh::SORT_DIGIT_BITS || shift != next) {
                printf("FAIL k=%u pass %u: shift %u bits %u (expected to start at bit %u)\n", k, p, shift, bits, next);
                ++failures;
            }
            for (uint32_t b = shift; b < shift + bits; ++b) {
                if (b >= 64 || b >= 2 * k) {
                    printf("FAIL k=%u pass %u: covers bit %u, at or above 2k\n", k, p, b);
                    ++failures;
                } else {
                    ++seen[b];
                }
            }
            next = shift + bits;
        }
        for (uint32_t b = 0; b < 2 * k; ++b)
            if (seen[b] != 1) {
                printf("FAIL k=%u: bit %u covered %u times\n", k, b, seen[b]);
                ++failures;
            }
    }
    if (failures) return 1;
    printf("SORT_PLAN_OK 32\n");
    return 0;
}
