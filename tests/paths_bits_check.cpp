// paths_bits_check.cpp -- krust_amd/csrc/paths_bits.h through a plain host compiler: kh_path_continues, kh_path_is_place and the row
// packing on a grid of word pairs, one line per pair for tests/test_paths_ref.py to hold against the Python predicate:
//   <a> <b> <continues(a, b)> <is_place(a)> <run_state(a)> <run_offset(a)>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../krust_amd/csrc/paths_bits.h"

int main() {
    const uint64_t his[] = {0, 1, 2, 3, 34, 35, 0xFFFFFFFCull, 0xFFFFFFFDull, 0xFFFFFFFEull, 0xFFFFFFFFull};
    const uint64_t los[] = {0, 1, 2, 7, 8, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFEull, 0xFFFFFFFFull};
    std::vector<uint64_t> words;
    for (uint64_t h : his)
        for (uint64_t l : los) words.push_back((h << 32) | l);
    uint64_t x = 0x9E3779B97F4A7C15ull;  // and pairs one step apart in either direction, from random places
    size_t n = 0;
    auto line = [&](uint64_t a, uint64_t b) {
        printf("%llu %llu %d %d %u %u\n", (unsigned long long)a, (unsigned long long)b, kh_path_continues(a, b), kh_path_is_place(a),
               kh_run_state(a), kh_run_offset(a));
        ++n;
    };
    for (uint64_t a : words)
        for (uint64_t b : words) line(a, b);
    for (int i = 0; i < 2000; ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        const uint64_t a = x & 0x0000FFFF0000FFFFull;
        line(a, a + 1);
        line(a, a - 1);
        line(a, a);
        line(a, (a ^ (1ull << 32)) + 1);
    }
    printf("paths_bits_check ok %zu\n", n);
    return 0;
}
