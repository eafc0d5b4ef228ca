// unitig_bits.h -- the oriented-successor arithmetic of the unitig construction (include/kmerhip.h, "unitigs of a count table"),
// shared by unitig.hip and by a plain host compiler (tests/unitig_bits_check.cpp compares it with string arithmetic for every k,
// tests/unitig_links_check.cpp the link word and the enter sign, tests/clip_bits_check.cpp the tip-clipping comparator and
// tests/pop_bits_check.cpp the bubble-popping comparator at the end of this file).
//
// An oriented node is (x, sign): sign 0 = (x, +) spells x's canonical string s, sign 1 = (x, -) spells rc(s).  As a state number it
// is 2 * id + sign with id = the rank of x among the nodes, so rev() is ^ 1.
// The successor by letter c of a node that spells w is t = w[1:] + c; it is entered as (canon(t), +) if t is the canonical string,
// else as (canon(t), -).  Which bit of the kh_graph_* mask says that this successor exists:
//   sign 0: t = s[1:] + c                       -> the right neighbour by c:      bit c
//   sign 1: t = rc(s)[1:] + c = rc(c' + s[:-1]) -> the left neighbour by c' = 3-c: bit 4 + (3 - c)
#pragma once
#include "kmer_bits.h"

#define KH_UNI_NONE 0xFFFFFFFFu  // no compactable link out of this state

// A string equal to its reverse complement (even k only; x is canonical, so this is the tie of the canonical choice).
KH_HD bool kh_unitig_palindrome(uint64_t x, uint32_t k) { return kh_revcomp(x, k) == x; }

// The four mask bits of the successors of (x, sign): the out-degree is their popcount.
KH_HD uint32_t kh_unitig_out_bits(uint32_t mask, uint32_t sign) { return sign ? (mask >> 4) & 15u : mask & 15u; }

// The letter c that bit j of kh_unitig_out_bits stands for.
KH_HD uint32_t kh_unitig_letter_of_bit(uint32_t j, uint32_t sign) { return sign ? 3u - j : j; }

// What (x, sign) spells, packed.
KH_HD uint64_t kh_unitig_spell(uint64_t x, uint32_t k, uint32_t sign) { return sign ? kh_revcomp(x, k) : x; }

// The successor of (x, sign) by letter c: *y = its canonical key, *ysign = the sign it is entered with (0 when t is y's string:
// a palindrome is entered as +), *ypal = whether it is a palindrome.
KH_HD void kh_unitig_successor(uint64_t x, uint32_t k, uint32_t sign, uint32_t c, uint64_t *y, uint32_t *ysign, bool *ypal) {
    const uint64_t w = kh_unitig_spell(x, k, sign);
    const uint64_t t = ((w << 2) | c) & kh_kmask(k);
    const uint64_t rt = kh_revcomp(t, k);
    *y = t < rt ? t : rt;
    *ysign = t > rt ? 1u : 0u;
    *ypal = t == rt;
}

// A link between a node and itself is never compacted: the homopolymer loop u -> u and the hairpin u -> rev(u).
KH_HD bool kh_unitig_self_link(uint64_t x, uint64_t y) { return x == y; }

// The ASCII letter at position i (0 = first) of a packed k-letter string.
KH_HD uint8_t kh_unitig_letter(uint64_t w, uint32_t k, uint32_t i) {
    return (uint8_t)((0x54474341u >> (8u * (uint32_t)((w >> (2u * (k - 1u - i))) & 3u))) & 0xFFu);  // "ACGT"
}

// ---- links between unitigs (include/kmerhip.h, kh_unitigs_links_*) ----------------------------------------------------------
// One word per link: 2 * from_unitig + from_sign in the high half, 2 * to_unitig + to_sign in the low half (+ = 0, - = 1).
KH_HD uint64_t kh_unitig_link_word(uint32_t from, uint32_t from_sign, uint32_t to, uint32_t to_sign) {
    return ((uint64_t)(2u * from + from_sign) << 32) | (uint64_t)(2u * to + to_sign);
}

#define KH_UNI_ENTER_NONE 2u  // the node entered lies at neither end of its unitig: never (include/kmerhip.h)

// The sign a unitig of L nodes is entered with through the oriented node (y, ysign), y being the node at position pos of its
// reported reading with sign rsign there: + if (y, ysign) is the reading's first oriented node, - if it is rev() of its last.
// The first is tested first, so that a palindrome (L = 1, entered as + by kh_unitig_successor) is always entered as +.
KH_HD uint32_t kh_unitig_enter_sign(uint32_t pos, uint32_t L, uint32_t rsign, uint32_t ysign) {
    if (pos == 0u && ysign == rsign) return 0u;
    if (pos + 1u == L && ysign != rsign) return 1u;
    return KH_UNI_ENTER_NONE;
}

// ---- tip clipping (include/kmerhip.h, kh_clip_tips_into; tests/clip_bits_check.cpp) -------------------------------------------------
// Whether rival b beats candidate i (b != i): any unitig that is no candidate does; a candidate does by the greater
// (KMERS, COUNT_SUM), the sum as the row stores it, and at a tie by the smaller index.
KH_HD bool kh_clip_beats(uint64_t kmers_b, uint64_t sum_b, uint32_t idx_b, bool cand_b, uint64_t kmers_i, uint64_t sum_i, uint32_t idx_i) {
    if (!cand_b) return true;
    if (kmers_b != kmers_i) return kmers_b > kmers_i;
    if (sum_b != sum_i) return sum_b > sum_i;
    return idx_b < idx_i;
}

// ---- bubble popping (include/kmerhip.h, kh_pop_bubbles_into; tests/pop_bits_check.cpp) -----------------------------------------------
// a * b as (hi, lo), from the four products of the 32-bit halves: the same text for the device and for a plain host compiler.
KH_HD void kh_mul_64x64(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo) {
    const uint64_t a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);  // (below 3 * 2^32)
    *lo = (p00 & 0xFFFFFFFFull) | (mid << 32);
    *hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);  // (the product is below 2^128: no carry out)
}

// Whether parallel candidate b beats candidate i (b != i): by the greater mean count COUNT_SUM / KMERS, compared exactly as the
// 128-bit products COUNT_SUM_b * KMERS_i and COUNT_SUM_i * KMERS_b (the sums as the rows store them), then by the greater KMERS,
// then by the smaller index.
KH_HD bool kh_pop_beats(uint64_t kmers_b, uint64_t sum_b, uint32_t idx_b, uint64_t kmers_i, uint64_t sum_i, uint32_t idx_i) {
    uint64_t bh, bl, ih, il;
    kh_mul_64x64(sum_b, kmers_i, &bh, &bl);
    kh_mul_64x64(sum_i, kmers_b, &ih, &il);
    if (bh != ih) return bh > ih;
    if (bl != il) return bl > il;
    if (kmers_b != kmers_i) return kmers_b > kmers_i;
    return idx_b < idx_i;
}
