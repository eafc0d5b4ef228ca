// probe.hip.h -- a read-only probe of one table, in either of its forms: what profile.hip asks per window of new sequences
// and join.hip per live slot of another table, and graph.hip and unitig.hip eight times per k-mer of the same table.
#pragma once
#include "ctx.hip.h"
#include "graph_bits.h"

namespace kh {

constexpr uint32_t PF_SAT = 0xFFFFFFFEu;  // the largest count an entry can say
__device__ __forceinline__ uint32_t pf_sat(u64 count) { return count > PF_SAT ? PF_SAT : (uint32_t)count; }

// The two table forms behind one interface: ref() = where a key's probe sequence starts (and whether this -- possibly shard --
// table can hold the key at all), load() = its first slot, resolve() = the count, probing on from that slot.  free_word() is
// what a free slot reads as: resolve() answers 0 to it, so a window that loads nothing (a key of another shard) needs no branch.
struct PfWide {
    TableGeom tg;
    typedef uint4 Word;
    struct Ref {
        const Slot *reg;
        u64 key;
        uint32_t off;
        bool mine;
    };
    __device__ __forceinline__ Ref ref(u64 key) const {
        const u64 H0 = kh_table_hash(key, tg.k);
        Ref r;
        // (a shard holds only keys of its hash range, and places them by the bits below the owner's: the rule of ntable_lookup_kernel)
        r.mine = !tg.shard_shift || (H0 >> (64 - tg.shard_shift)) == tg.shard_index;
        const u64 H = H0 << tg.shard_shift;
        r.reg = tg.table + region_of(tg, H) * REGION_SLOTS;
        r.off = start_of(tg, H);
        r.key = key;
        return r;
    }
    __device__ static __forceinline__ Word free_word() { return make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u); }
    __device__ static __forceinline__ Word load(const Ref &r) { return *reinterpret_cast<const uint4 *>(&r.reg[r.off]); }
    __device__ static __forceinline__ uint32_t resolve(const Ref &r, Word w) {
        uint32_t off = r.off;
        for (uint32_t probes = 0; probes < REGION_SLOTS; ++probes) {
            const u64 sk = ((u64)w.y << 32) | w.x;
            if (sk == r.key) return pf_sat(((u64)w.w << 32) | w.z);
            if (sk == KH_EMPTY_KEY) return 0u;
            off = (off + 1) & REGION_MASK;
            w = *reinterpret_cast<const uint4 *>(&r.reg[off]);
        }
        return 0u;
    }
    // the same walk with the full count (join.hip: a table against a table)
    __device__ static __forceinline__ u64 resolve64(const Ref &r, Word w) {
        uint32_t off = r.off;
        for (uint32_t probes = 0; probes < REGION_SLOTS; ++probes) {
            const u64 sk = ((u64)w.y << 32) | w.x;
            if (sk == r.key) return ((u64)w.w << 32) | w.z;
            if (sk == KH_EMPTY_KEY) return 0ull;
            off = (off + 1) & REGION_MASK;
            w = *reinterpret_cast<const uint4 *>(&r.reg[off]);
        }
        return 0ull;
    }
    // the same walk for WHERE the key is: its slot index in the table (what JsWide::load takes), ~0 when it is absent (unitig.hip)
    __device__ __forceinline__ u64 resolve_slot(const Ref &r, Word w) const {
        uint32_t off = r.off;
        for (uint32_t probes = 0; probes < REGION_SLOTS; ++probes) {
            const u64 sk = ((u64)w.y << 32) | w.x;
            if (sk == r.key) return (u64)(r.reg - tg.table) + off;
            if (sk == KH_EMPTY_KEY) return ~0ull;
            off = (off + 1) & REGION_MASK;
            w = *reinterpret_cast<const uint4 *>(&r.reg[off]);
        }
        return ~0ull;
    }
};

struct PfNarrow {
    const u64 *ntab;
    PartGeom g;
    typedef u64 Word;
    struct Ref {
        const u64 *reg;
        uint32_t pay;
        uint32_t off;
        bool mine;
    };
    __device__ __forceinline__ Ref ref(u64 key) const {
        const u64 H0 = kh_table_hash(key, g.k);
        Ref r;
        r.mine = !g.shard_shift || (H0 >> (64 - g.shard_shift)) == g.shard_index;
        const u64 H = H0 << g.shard_shift;
        r.pay = Pay<uint32_t>::make(key, H, g);
        r.reg = ntab + ((u64)kh_p1_of(H, g.p1_bits) * g.b2 + kh_bucket_of_x(r.pay, g.b2)) * REGION_SLOTS;
        r.off = narrow_start(g, r.pay);
        return r;
    }
    __device__ static __forceinline__ Word free_word() { return 0ull; }
    __device__ static __forceinline__ Word load(const Ref &r) { return r.reg[r.off]; }
    __device__ static __forceinline__ uint32_t resolve(const Ref &r, Word w) {
        uint32_t off = r.off;
        for (uint32_t probes = 0; probes < REGION_SLOTS; ++probes) {
            if ((w >> 32) == 0) return 0u;
            if ((uint32_t)w == r.pay) return pf_sat(w >> 32);
            off = (off + 1) & REGION_MASK;
            w = r.reg[off];
        }
        return 0u;
    }
    __device__ static __forceinline__ u64 resolve64(const Ref &r, Word w) {
        uint32_t off = r.off;
        for (uint32_t probes = 0; probes < REGION_SLOTS; ++probes) {
            if ((w >> 32) == 0) return 0ull;
            if ((uint32_t)w == r.pay) return w >> 32;
            off = (off + 1) & REGION_MASK;
            w = r.reg[off];
        }
        return 0ull;
    }
    __device__ __forceinline__ u64 resolve_slot(const Ref &r, Word w) const {  // (the slot index JsNarrow::load takes)
        uint32_t off = r.off;
        for (uint32_t probes = 0; probes < REGION_SLOTS; ++probes) {
            if ((w >> 32) == 0) return ~0ull;
            if ((uint32_t)w == r.pay) return (u64)(r.reg - ntab) + off;
            off = (off + 1) & REGION_MASK;
            w = r.reg[off];
        }
        return ~0ull;
    }
};

// The de Bruijn mask of key x (include/kmerhip.h, kh_graph_*): eight canonical neighbour keys from ONE reverse complement, eight
// ref() (eight Feistel hashes), the eight first-slot loads all in flight before the first is looked at -- as profile_kernel and
// join_kernel keep eight loads of eight windows / slots in flight --, then the eight walks.  A neighbour is in the node set iff
// its count is >= min_count (>= 1).  (graph.hip per key; unitig.hip per node, once.)
template <typename PRB>
__device__ __forceinline__ uint32_t graph_mask_of(const PRB &prb, u64 x, uint32_t k, u64 min_count) {
    uint64_t nb[8];
    kh_graph_neighbours(x, k, nb);
    typename PRB::Ref ref[8];
    typename PRB::Word first[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ref[j] = prb.ref(nb[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) first[j] = PRB::load(ref[j]);
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (PRB::resolve64(ref[j], first[j]) >= min_count) mask |= 1u << j;
    return mask;
}

// ---- source views: slot i of a scanned table -> (key, count), false for a free slot (join.hip, graph.hip) -------------------
struct JsWide {
    const Slot *table;
    __device__ __forceinline__ bool load(u64 i, u64 &key, u64 &count) const {
        const uint4 v = *reinterpret_cast<const uint4 *>(&table[i]);
        key = ((u64)v.y << 32) | v.x;
        count = ((u64)v.w << 32) | v.z;
        return key != KH_EMPTY_KEY;
    }
};
struct JsNarrow {
    const u64 *ntab;
    PartGeom g;
    __device__ __forceinline__ bool load(u64 i, u64 &key, u64 &count) const {
        const u64 sl = ntab[i];
        count = sl >> 32;
        const bool live = count != 0;
        key = live ? narrow_key(g, i, (uint32_t)sl) : 0ull;  // (the inverse hash only for live slots: ntable_compact_kernel)
        return live;
    }
};

}  // namespace kh

// ---- host side: the one place that says which form a context's table is in ------------------------------------------------------
namespace khi {

// f(view): the probe of c's table / its slots as a source, in the form the table is in -- f is instantiated with both views
template <typename F>
void with_probe(const kh_ctx *c, F f) {
    if (c->narrow) f(kh::PfNarrow{(const u64 *)c->ntab, c->narrow_g});
    else f(kh::PfWide{table_geom(c, c->table, c->cap)});
}
template <typename F>
void with_source(const kh_ctx *c, F f) {
    if (c->narrow) f(kh::JsNarrow{(const u64 *)c->ntab, c->narrow_g});
    else f(kh::JsWide{(const Slot *)c->table});
}

}  // namespace khi
