// paths_bits.h -- the run rows of kh_unitigs_paths* (include/kmerhip.h, "RUN-COMPRESSED PATHS"), shared by paths.hip and by a plain
// host compiler: when one located word continues another, and what a run's first word puts into its row.
#pragma once
#include "locate_bits.h"

// The two specials of kh_unitigs_locate* are the two largest words; everything below is a place.
KH_HD int kh_path_is_place(uint64_t w) { return w < 0xFFFFFFFFFFFFFFFEull; }

// b, the word of window start i + 1, continues a, the word of window start i: both are places of the same unitig read with the same
// sign (one high word), and the offset moves by one -- up for +, down for -.  Offsets are compared without wrapping: nothing
// continues offset 0 downwards.  A link crossing (the closing link of a circle, a turn of a homopolymer loop) is no continuation.
KH_HD int kh_path_continues(uint64_t a, uint64_t b) {
    const uint64_t la = a & 0xFFFFFFFFull, lb = b & 0xFFFFFFFFull;
    const int step = ((a >> 32) & 1ull) ? lb + 1ull == la : la + 1ull == lb;
    return kh_path_is_place(a) && kh_path_is_place(b) && (a >> 32) == (b >> 32) && step;
}

// A run's row from the word of its first window: KH_RUN_STATE and KH_RUN_OFFSET.
KH_HD uint32_t kh_run_state(uint64_t first) { return (uint32_t)(first >> 32); }
KH_HD uint32_t kh_run_offset(uint64_t first) { return (uint32_t)(first & 0xFFFFFFFFull); }
