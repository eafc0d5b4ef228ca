// geom_bits.h -- table / partition geometry arithmetic shared by host and device code (and, like kmer_bits.h, by a plain
// host compiler: tests/geometry_check.cpp holds every function here to 128-bit integer arithmetic for k = 1..32).
// What the names mean, and why the geometry is what it is: kernels.hip.h, "Table geometry".
#pragma once
#include <stdint.h>

#include "kmer_bits.h"

#if defined(__HIPCC__)
#define KH_GEOM_HD __host__ __device__
#define KH_GEOM_FORCEINLINE __forceinline__
#else
#define KH_GEOM_HD
#define KH_GEOM_FORCEINLINE inline
#endif

namespace kh {

typedef unsigned long long u64;

#ifndef KH_REGION_BITS
#define KH_REGION_BITS 12
#endif
constexpr uint32_t REGION_BITS = KH_REGION_BITS;
constexpr uint32_t REGION_SLOTS = 1u << REGION_BITS;
constexpr uint32_t REGION_MASK = REGION_SLOTS - 1;
// A key's probe sequence inside its region starts at an EVEN slot (and goes on slot by slot from there): the region pass
// then sees the two slots a key most likely sits in with ONE 8-byte LDS read (region_count_kernel32: at load 0.5 a key is in
// its home slot two times in three, in its home pair more than four times in five).  Everything that probes uses start_of /
// narrow_start (or this mask), so the layout is one decision.  Measured (S100M, k = 21; 125 M reads at load 0.61), region
// pass: groups of 1 / 2 / 4 slots 24.5 / 21.7 / 22.5 ms and 43.0 / 36.9 / 36.6 ms -- a 16-byte read costs the LDS twice the
// cycles of an 8-byte one, and eight of them in flight do not fit the registers of two workgroups per CU.
#ifndef KH_REGION_GROUP
#define KH_REGION_GROUP 2  // 1, 2 or 4 (A/B builds: make VARIANT=_g4 EXTRA=-DKH_REGION_GROUP=4)
#endif
constexpr uint32_t REGION_GROUP = KH_REGION_GROUP;
constexpr uint32_t REGION_START_MASK = REGION_MASK & ~(REGION_GROUP - 1);

// ---- geometry arithmetic shared by tables (TableGeom) and partition passes (PartGeom) ------------------------------------
struct RegionGeom {  // (p1_bits, b2) of either
    uint32_t p1_bits, b2;
};
KH_GEOM_HD inline u64 kh_regions_of(RegionGeom g) { return (u64)g.b2 << g.p1_bits; }
// the geometry of a table with `nregions` regions: a power of two up to 1024 (p1_bits = log2, b2 = 1), a multiple of 1024 beyond
KH_GEOM_HD inline RegionGeom kh_geom_of_regions(u64 nregions) {
    RegionGeom g;
    if (nregions <= 1024) {
        g.p1_bits = 0;
        while ((2ull << g.p1_bits) <= nregions) ++g.p1_bits;
        g.b2 = 1;
    } else {
        g.p1_bits = 10;
        g.b2 = (uint32_t)(nregions >> 10);
    }
    return g;
}
KH_GEOM_HD inline bool kh_regions_valid(u64 nregions) {
    return nregions >= 1 && (nregions <= 1024 ? (nregions & (nregions - 1)) == 0 : (nregions & 1023) == 0 && (nregions >> 10) <= (1u << 20));
}
KH_GEOM_HD inline uint32_t kh_floor_log2(uint32_t v) {
    uint32_t b = 0;
    while ((2u << b) <= v && b < 31) ++b;
    return b;
}
// x (the 32 hash bits behind the level-1 digit) of the placement hash
KH_GEOM_HD KH_GEOM_FORCEINLINE uint32_t kh_x_of(u64 H, uint32_t p1_bits) { return (uint32_t)((H << p1_bits) >> 32); }
KH_GEOM_HD KH_GEOM_FORCEINLINE uint32_t kh_p1_of(u64 H, uint32_t p1_bits) { return p1_bits ? (uint32_t)(H >> (64 - p1_bits)) : 0u; }
// bucket of x among b2, and its in-region start
KH_GEOM_HD KH_GEOM_FORCEINLINE uint32_t kh_bucket_of_x(uint32_t x, uint32_t b2) { return (uint32_t)(((u64)x * b2) >> 32); }
KH_GEOM_HD KH_GEOM_FORCEINLINE uint32_t kh_start_of_x(uint32_t x, uint32_t b2) {
    return ((uint32_t)(x * b2) >> (32 - REGION_BITS)) & REGION_START_MASK;
}
// smallest x of bucket b (b <= b2: b = b2 gives 2^32): ceil(b * 2^32 / b2)
KH_GEOM_HD KH_GEOM_FORCEINLINE u64 kh_xlo(uint32_t b, uint32_t b2) { return (((u64)b << 32) + b2 - 1) / b2; }
// ... among the x a k-mer table can hold: with 2k < p1_bits + 32 hash bits the low zs = p1_bits + 32 - 2k bits of every x are
// zero, so the smallest x of the bucket is kh_xlo rounded UP to a multiple of 2^zs -- and x minus THAT keeps its low zs bits
// zero (the exchange units count on it: their count field lives there).  zs = kh_x_zero_bits(k, p1_bits).
KH_GEOM_HD KH_GEOM_FORCEINLINE uint32_t kh_x_zero_bits(uint32_t k, uint32_t p1_bits) {
    const int z = (int)p1_bits + 32 - 2 * (int)k;
    return z <= 0 ? 0u : (z >= 32 ? 31u : (uint32_t)z);
}
KH_GEOM_HD KH_GEOM_FORCEINLINE uint32_t kh_xlo_k(uint32_t b, uint32_t b2, uint32_t zs) {
    const u64 m = (1ull << zs) - 1;
    return (uint32_t)((kh_xlo(b, b2) + m) & ~m);
}
// "The hash bits below the region index" as a 32-bit window -- what the exchange units (shard.hip.h) carry: the top
// w = 32 - floor(log2 b2) bits hold x - xlo(bucket) (< 2^w), the bits below them are the hash bits that follow x.
// For b2 = 2^j: bits [p1_bits + j, p1_bits + j + 32) of H, as in rounds 1-3.
KH_GEOM_HD KH_GEOM_FORCEINLINE uint32_t kh_below_w(uint32_t b2) { return 32u - kh_floor_log2(b2); }
KH_GEOM_HD KH_GEOM_FORCEINLINE uint32_t kh_below_region(u64 H, RegionGeom g, uint32_t k) {
    const uint32_t x = kh_x_of(H, g.p1_bits), b = kh_bucket_of_x(x, g.b2), w = kh_below_w(g.b2);
    const uint32_t xoff = x - kh_xlo_k(b, g.b2, kh_x_zero_bits(k, g.p1_bits));
    const uint32_t z = w < 32 ? (uint32_t)((H << (g.p1_bits + 32)) >> (32 + w)) : 0u;  // the 32 - w hash bits behind x
    return (w < 32 ? xoff << (32 - w) : xoff) | z;
}
// the placement hash back from (region, window)
KH_GEOM_HD KH_GEOM_FORCEINLINE u64 kh_hash_of_below(u64 region, uint32_t low, RegionGeom g, uint32_t k) {
    const uint32_t p1 = (uint32_t)(region / g.b2), b = (uint32_t)(region % g.b2), w = kh_below_w(g.b2);
    const uint32_t x = kh_xlo_k(b, g.b2, kh_x_zero_bits(k, g.p1_bits)) + (w < 32 ? low >> (32 - w) : low);
    const u64 z = w < 32 ? (u64)(low << w) : 0ull;  // left-aligned in 32 bits
    u64 H = ((u64)x << 32) | z;                    // x and what follows it, left-aligned in 64 bits ...
    H >>= g.p1_bits;                               // ... behind the level-1 digit
    if (g.p1_bits) H |= (u64)p1 << (64 - g.p1_bits);
    return H;
}
// significant bits of that window for a k-mer table: 2k minus the bits the region index stands for
KH_GEOM_HD inline int kh_below_bits(uint32_t k, uint32_t shard_shift, RegionGeom g) {
    return 2 * (int)k - (int)shard_shift - (int)g.p1_bits - (int)kh_floor_log2(g.b2);
}

}  // namespace kh
