// graph_bits.h -- the de Bruijn neighbours of a packed canonical k-mer (include/kmerhip.h, "de Bruijn graph degrees"), shared by
// graph.hip and by a plain host compiler (tests/graph_bits_check.cpp compares it with string arithmetic for every k).
//
// For a canonical key x with string s, r = kh_revcomp(x, k) and m = kh_kmask(k):
//   right neighbour by letter c:  s[1:] + c    forward ((x << 2) | c) & m           reverse (r >> 2) | ((3 - c) << 2(k-1))
//   left neighbour by letter c:   c + s[:-1]   forward (x >> 2) | (c << 2(k-1))     reverse ((r << 2) | (3 - c)) & m
// and the neighbour's key is the smaller of the two.  One reverse complement per key; no shift reaches 64 at k = 32.
#pragma once
#include "kmer_bits.h"

// Is `x` a canonical key of this k: no bit at or above 2k, and not greater than its reverse complement.
KH_HD bool kh_graph_key_valid(uint64_t x, uint32_t k) {
    return (x & ~kh_kmask(k)) == 0 && x <= kh_revcomp(x, k);
}

// nb[c] = the canonical key of the right neighbour by letter c, nb[4 + c] = of the left neighbour: the bit order of the mask
// (KH_GRAPH_RIGHT(c) = 1 << c, KH_GRAPH_LEFT(c) = 16 << c).
KH_HD void kh_graph_neighbours(uint64_t x, uint32_t k, uint64_t nb[8]) {
    const uint64_t m = kh_kmask(k), r = kh_revcomp(x, k);
    const uint32_t top = 2 * (k - 1);
    const uint64_t rf = (x << 2) & m, rr = r >> 2;  // right: the forward string loses its first letter, the reverse its last
    const uint64_t lf = x >> 2, lr = (r << 2) & m;  // left: the other way round
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t c = 0; c < 4; ++c) {
        const uint64_t f0 = rf | c, r0 = rr | ((uint64_t)(3u - c) << top);
        const uint64_t f1 = lf | ((uint64_t)c << top), r1 = lr | (3u - c);
        nb[c] = f0 < r0 ? f0 : r0;
        nb[4 + c] = f1 < r1 ? f1 : r1;
    }
}
