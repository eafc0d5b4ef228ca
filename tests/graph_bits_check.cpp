// graph_bits_check.cpp -- the neighbour arithmetic of krust_amd/csrc/graph_bits.h (what graph.hip runs per key) compiled for the
// host: reads "k key" lines (decimal) from stdin and prints "valid n0 .. n7" per line -- valid: kh_graph_key_valid, n0..n3 the
// right neighbours by A, C, G, T, n4..n7 the left ones.  tests/test_graph_masks_ref.py compares them with string arithmetic.
#include <cinttypes>
#include <cstdio>

#include "../krust_amd/csrc/graph_bits.h"

int main() {
    unsigned k;
    uint64_t x;
    while (scanf("%u %" SCNu64, &k, &x) == 2) {
        if (k < 1 || k > 32) return 2;
        uint64_t nb[8];
        kh_graph_neighbours(x, k, nb);
        printf("%d", kh_graph_key_valid(x, k) ? 1 : 0);
        for (int j = 0; j < 8; ++j) printf(" %" PRIu64, nb[j]);
        printf("\n");
    }
    return 0;
}
