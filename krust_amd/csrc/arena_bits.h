// arena_bits.h -- the LDS bin geometry of the arena level 2 (partition.hip.h part2_arena_kernel), in BYTES: the bucket counters
// count bytes, a rank comes back from its atomic as the payload's byte offset in the bin, and the store address is one
// shift-add (power-of-two bucket counts) or one 24-bit multiply-add on top of it.  Shared with a plain host compiler like
// geom_bits.h: tests/arena_bits_check.cpp walks every geometry the arena path can get.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KH_ARENA_HD __host__ __device__ __forceinline__
#else
#define KH_ARENA_HD inline
#endif

namespace kh {

constexpr uint32_t ARENA_WORD = 16;  // bytes a flush moves per lane and instruction

// bytes all bins of a workgroup hold together: 128 KiB, 144 KiB in the 768-bucket instance (what the CU's 160 KiB leave there)
KH_ARENA_HD constexpr uint32_t arena_total_bytes(int nbk) { return nbk == 768 ? 144u << 10 : 128u << 10; }
// the word behind the bins where a rank that did not fit its bin stores (a whole unit of room: s_bin[TOTAL + UNIT])
KH_ARENA_HD constexpr uint32_t arena_trash_addr(int nbk) { return arena_total_bytes(nbk); }
// power-of-two bucket counts (b2 = 1 << p2_bits, 5 <= p2_bits <= 10): a bin is total >> p2_bits bytes, its address a shift
KH_ARENA_HD constexpr uint32_t arena_bin_shift(int nbk, uint32_t p2_bits) { return 17u - p2_bits; }
static_assert(arena_total_bytes(512) == 1u << 17 && arena_total_bytes(1024) == 1u << 17, "arena_bin_shift counts on 128 KiB");
// bytes per bin: the total shared out among the partition's b2 buckets, whole 16-byte words
KH_ARENA_HD constexpr uint32_t arena_bin_bytes(int nbk, uint32_t b2) { return (arena_total_bytes(nbk) / b2) & ~(ARENA_WORD - 1u); }
KH_ARENA_HD constexpr uint32_t arena_bin_bytes_pow2(int nbk, uint32_t p2_bits) { return arena_total_bytes(nbk) >> p2_bits; }
// byte address of (bucket, byte rank) in the bins.  The multiply is a 24-bit one: a bucket is below 1024, a bin below 2^18 bytes.
KH_ARENA_HD uint32_t arena_addr_pow2(uint32_t bucket, uint32_t shift, uint32_t rank) { return (bucket << shift) + rank; }
KH_ARENA_HD uint32_t arena_addr_mul(uint32_t bucket, uint32_t bin_bytes, uint32_t rank) {
    return (bucket & 0xFFFFFFu) * (bin_bytes & 0xFFFFFFu) + rank;
}
// where the flush reads 16-byte word w of whole unit u of a bin
KH_ARENA_HD uint32_t arena_unit_word(uint32_t bin_addr, uint32_t unit_bytes, uint32_t u, uint32_t w) {
    return bin_addr + u * unit_bytes + w * ARENA_WORD;
}

}  // namespace kh
