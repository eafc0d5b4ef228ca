// locate_bits.h -- the place word of kh_unitigs_locate* (include/kmerhip.h, "LOCATED on the live unitigs"), shared by locate.hip
// and by a plain host compiler.
//
// A place is (u, sign, j): the k-mer is node j of unitig u's reported reading, read as the reading spells it (sign 0) or as its
// reverse complement (sign 1).  2 * u + sign is the state number of a link word's halves (unitig_bits.h).
#pragma once
#include "kmer_bits.h"

#define KH_LOC_NONE 0xFFFFFFFFFFFFFFFFull  // a slot of the place map that holds no node of S

// What the index stores for node j of unitig u: o = 1 when the reading spells the reverse complement of the node's canonical string.
KH_HD uint64_t kh_loc_word(uint32_t u, uint32_t o, uint32_t j) { return ((uint64_t)(2u * u + o) << 32) | (uint64_t)j; }

// What a window reports for the map's word m: strand = 1 when the window's letters are the reverse complement of its canonical
// string.  The window reads the place as the reading does (+) iff both took the same strand: a palindrome took 0 both times.
// Without a select (locate_kernel is short of the scalar registers that eight compare masks take): the high word of a place is
// at most 2^32 - 3, so a = the carry out of (high word + 1) is 1 for KH_LOC_NONE alone -- that word stays as it is and loses 1.
KH_HD uint64_t kh_loc_result(uint64_t m, uint32_t strand) {
    const uint64_t a = ((m >> 32) + 1ull) >> 32;
    return (m ^ (((uint64_t)strand & ~a) << 32)) - a;
}
