// support_bits.h -- the crossings of kh_unitigs_link_support* (include/kmerhip.h, "READ SUPPORT PER LINK"), shared by support.hip and
// by a plain host compiler: when two consecutive rows of one record are a crossing, the word it is looked up with, that word's mirror.
#pragma once
#include "paths_bits.h"

// Row i ends where row i + 1 begins: no window start lies between them.
KH_HD int kh_sup_adjacent(uint32_t qend_i, uint32_t qstart_next) { return qend_i == qstart_next; }

// The word of a crossing from the run with state a into the run with state b: the encoding of a link word.
KH_HD uint64_t kh_sup_word(uint32_t a, uint32_t b) { return ((uint64_t)a << 32) | (uint64_t)b; }

// The crossing that the same read gives when it is reverse-complemented: b reversed into a reversed.
KH_HD uint64_t kh_sup_mirror(uint64_t w) { return (((w & 0xFFFFFFFFull) ^ 1ull) << 32) | ((w >> 32) ^ 1ull); }
