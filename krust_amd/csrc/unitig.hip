// unitig.hip -- kh_unitigs_*: the unitigs (maximal non-branching paths) of the de Bruijn graph of a count table, built on the
// device (what BCALM / Cuttlefish build after KMC).  No reference counterpart.  The definitions are in include/kmerhip.h, the
// argument that a chain never meets its own mirror image in DESIGN.md 4.11.
//
// Nodes are the table's pairs in ascending key order (compact_pairs + the radix sort of sort.hip): node id = rank, so "smaller key"
// is "smaller id" and unitigs come out in id order of their first nodes without a second sort.  An oriented node is the state
// 2 * id + sign (unitig_bits.h).
//   unitig_index_kernel<PRB>   per node: its slot in the table -> slot2id[slot] = id (resolve_slot, probe.hip.h), and its mask
//                              (graph_mask_of) -> masks[id]
//   unitig_link_kernel<PRB>    per node, both signs: the single successor where the out-degree is 1, its id by ONE probe, the four
//                              conditions of a compactable link -> next[state] or KH_UNI_NONE
//   unitig_rank_init_kernel,   chain ranking by pointer doubling over the 2n states: (state reached, hops so far, smallest node id
//   unitig_rank_round_kernel   seen), one launch per round, double-buffered, a "something changed" word read back per round; the
//                              host bounds the rounds by ceil(log2(2n)) + 1
//   unitig_cut_kernel          states that have not reached an end by then lie on cycles and know their cycle's smallest id m: the
//                              link into (m, +) and its mirror out of (m, -) go, m is marked circular, and the ranking runs again
//   unitig_reading_kernel      per node, from the two ranks of (x, +) and (x, -): its unitig's first node, its own sign in the
//                              reported reading, its position; first nodes are flagged
//   device_scan                flags -> unitig index; then L + k - 1 per unitig -> START
//   unitig_row_kernel          per first node: KMERS, FLAGS, the length
//   unitig_place_kernel        per node: its id and sign into unitig order (4-byte stores); START
//   unitig_sum_kernel          COUNT_SUM: a segmented sum over that order -- one atomic per (wave, unitig), never one per node
//   unitig_bases_kernel        per 16 bytes of the base array: the letters, one aligned 16-byte store (bytes only in the array's tail)
// kh_unitigs_begin_linked only, behind all of the above and while its scratch is live (the links between unitigs, include/kmerhip.h):
//   unitig_end_degree_kernel   per end state (two per unitig: the last node of the reading, rev() of the first): its out-degree from the
//                              node's mask, no probes
//   device_scan                degrees -> offsets; their sum is the number of links
//   unitig_link_out_kernel<PRB> per end state: its up to four successors, four first-slot loads in flight, slot -> node id -> unitig,
//                              position and sign in the reading -> link words, sorted in registers, stored at the lane's offset (no atomics)
// kh_clip_tips_into only, behind the links and while the same scratch is live (one round of tip clipping, include/kmerhip.h):
//   clip_candidate_kernel      per unitig: its row, the offsets of its two end states and the links of the attached end -> one byte
//   clip_decide_kernel         per candidate: its links, the links out of each entered state reversed (the rivals), their bytes and
//                              rows -> one clipped byte; six of the eight words by wave reductions
//   clip_keep_kernel           per node in unitig order: a node of a surviving unitig is upserted into the OTHER context's table
// kh_pop_bubbles_into only, in the same place (one round of bubble popping, include/kmerhip.h); the keep kernel is clip's:
//   pop_exits_kernel           per unitig: its row, the offsets of its two end states and its two links -> one exit word
//   pop_decide_kernel          per candidate: the links out of its + exit reversed (the unitigs that enter the same place), their exit
//                              words, the rows of the parallel ones (kh_pop_beats) -> one popped byte; seven of the nine words
// kh_drop_components_into only, in the same place (one round of dropping small components, include/kmerhip.h); the keep kernel is clip's:
//   components_label           components.hip: hook and compress rounds over the links, then the sums per root
//   comp_drop_kernel           components.hip: per unitig, its component's k-mers against the bound -> one dropped byte; seven of the nine words
// No kernel waits for another workgroup, and no device loop is without a bound.  Rates were not measured (profiles/README.md r13).
#include "ctx.hip.h"
#include "probe.hip.h"
#include "unitig_bits.h"

namespace kh {

struct UniRank {  // 2n entries each
    uint32_t *tgt;   // the state reached so far (itself for an end: a state with no link out)
    uint32_t *hops;  // links followed to get there
    uint32_t *mn;    // smallest node id among the states from this one up to, not including, tgt
};
constexpr uint32_t UNI_SIGN = 0x80000000u;

// kernel-resource-usage (gfx950, hipcc -O3), PfNarrow / PfWide: 65 / 96 VGPRs (eight probes in flight, as graph_kernel), 68 / 63 SGPRs, no LDS,
// no scratch, no spills, 7 / 5 waves per SIMD.
template <typename PRB>
__global__ __launch_bounds__(BLOCK) void unitig_index_kernel(const u64 *__restrict__ keys, uint32_t n, uint32_t k, u64 min_count, PRB prb, u64 cap,
                                                             uint32_t *__restrict__ slot2id, uint8_t *__restrict__ masks) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u64 x = keys[i];
        const typename PRB::Ref ref = prb.ref(x);
        const typename PRB::Word w = PRB::load(ref);
        const uint32_t mask = graph_mask_of(prb, x, k, min_count);
        const u64 slot = prb.resolve_slot(ref, w);
        if (slot < cap) slot2id[slot] = (uint32_t)i;  // (always: x came out of this table)
        masks[i] = (uint8_t)mask;
    }
}

// kernel-resource-usage (gfx950, hipcc -O3), PfNarrow / PfWide: 29 / 39 VGPRs, 66 / 61 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
template <typename PRB>
__global__ __launch_bounds__(BLOCK) void unitig_link_kernel(const u64 *__restrict__ keys, uint32_t n, uint32_t k, PRB prb, u64 cap,
                                                            const uint32_t *__restrict__ slot2id, const uint8_t *__restrict__ masks,
                                                            uint32_t *__restrict__ next) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u64 x = keys[i];
        const uint32_t mask = masks[i];
        const bool pal = kh_unitig_palindrome(x, k);
        u64 y[2];
        uint32_t ys[2];
        bool want[2];
#pragma unroll
        for (uint32_t sg = 0; sg < 2; ++sg) {
            const uint32_t bits = kh_unitig_out_bits(mask, sg);
            y[sg] = x;  // (a key that is there: the probe below needs no branch)
            ys[sg] = 0;
            want[sg] = !pal && __builtin_popcount(bits) == 1;
            if (want[sg]) {
                uint64_t yy;
                uint32_t s;
                bool yp;
                kh_unitig_successor(x, k, sg, kh_unitig_letter_of_bit((uint32_t)__builtin_ctz(bits), sg), &yy, &s, &yp);
                want[sg] = !kh_unitig_self_link(x, yy) && !yp;
                if (want[sg]) {
                    y[sg] = yy;
                    ys[sg] = s;
                }
            }
        }
        typename PRB::Ref ref[2];
        typename PRB::Word first[2];
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) ref[sg] = prb.ref(y[sg]);
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) first[sg] = PRB::load(ref[sg]);  // (both first-slot loads in flight)
        uint32_t nx[2];
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
            nx[sg] = KH_UNI_NONE;
            const u64 slot = prb.resolve_slot(ref[sg], first[sg]);
            if (want[sg] && slot < cap) {
                const uint32_t yid = slot2id[slot];
                if (yid < n && __builtin_popcount(kh_unitig_out_bits(masks[yid], ys[sg] ^ 1u)) == 1) nx[sg] = 2u * yid + ys[sg];
            }
        }
        *reinterpret_cast<uint2 *>(&next[2 * i]) = make_uint2(nx[0], nx[1]);
    }
}

// kernel-resource-usage (gfx950, hipcc -O3): 12 VGPRs, 22 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_rank_init_kernel(const uint32_t *__restrict__ next, u64 states, UniRank r) {
    for (u64 s = (u64)blockIdx.x * BLOCK + threadIdx.x; s < states; s += (u64)gridDim.x * BLOCK) {
        const uint32_t nx = next[s];
        r.tgt[s] = nx == KH_UNI_NONE ? (uint32_t)s : nx;
        r.hops[s] = nx == KH_UNI_NONE ? 0u : 1u;
        r.mn[s] = (uint32_t)(s >> 1);
    }
}

// One round of pointer doubling: a state whose target is not an end takes over the target's jump.  (An end is told by next[], not
// by tgt[t] == t: on a cycle whose length divides the hops so far a state's target is the state itself.)
// kernel-resource-usage (gfx950, hipcc -O3): 13 VGPRs, 50 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_rank_round_kernel(const uint32_t *__restrict__ next, u64 states, UniRank a, UniRank b,
                                                                  uint32_t *__restrict__ changed) {
    bool any = false;
    for (u64 s = (u64)blockIdx.x * BLOCK + threadIdx.x; s < states; s += (u64)gridDim.x * BLOCK) {
        uint32_t t = a.tgt[s], h = a.hops[s], m = a.mn[s];
        if (t < states && next[t] != KH_UNI_NONE) {
            h += a.hops[t];  // (wraps on a cycle only, where it is not used)
            const uint32_t mt = a.mn[t];
            m = mt < m ? mt : m;
            t = a.tgt[t];
            any = true;
        }
        b.tgt[s] = t;
        b.hops[s] = h;
        b.mn[s] = m;
    }
    if (kh_any(any) && lane_id() == 0) *changed = 1u;  // (every writer writes the same word)
}

// After the last round: (m, +) with an unfinished target and m the smallest id of its cycle.  The cycle through (m, +) loses the
// link into (m, +) -- its predecessor is rev(next((m, -))) --, the mirrored cycle the link out of (m, -).  Only this lane writes to
// either cycle, and it has read before it writes.
// kernel-resource-usage (gfx950, hipcc -O3): 14 VGPRs, 30 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_cut_kernel(uint32_t *__restrict__ next, uint32_t n, UniRank r, uint8_t *__restrict__ circ) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const uint32_t t = r.tgt[2 * i];
        if (r.mn[2 * i] != (uint32_t)i || t >= 2ull * n || next[t] == KH_UNI_NONE) continue;
        const uint32_t back = next[2 * i + 1];  // (never NONE: the mirrored cycle passes through (m, -))
        if (back == KH_UNI_NONE || back >= 2ull * n) continue;
        next[back ^ 1u] = KH_UNI_NONE;
        next[2 * i + 1] = KH_UNI_NONE;
        circ[i] = 1;
    }
}

// With E+ = (b, .) the end reached from (x, +) after d+ links and E- = (a, .) the end reached from (x, -) after d-: the chain read
// with x as + starts at rev(E-), has x at position d- and ends in E+; the two end nodes are a and b, and L = d+ + d- + 1.
// kernel-resource-usage (gfx950, hipcc -O3): 16 VGPRs, 50 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_reading_kernel(const uint32_t *__restrict__ next, uint32_t n, UniRank r, uint32_t *__restrict__ head,
                                                               uint32_t *__restrict__ posg, uint32_t *__restrict__ first, uint32_t *__restrict__ err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const uint32_t ep = r.tgt[2 * i], dp = r.hops[2 * i], em = r.tgt[2 * i + 1], dm = r.hops[2 * i + 1];
        uint32_t h = (uint32_t)i, p = 0;
        if (ep >= 2ull * n || em >= 2ull * n || next[ep] != KH_UNI_NONE || next[em] != KH_UNI_NONE) {
            *err = 1u;  // (a chain that did not end: never, behind the cut)
        } else {
            const uint32_t a = em >> 1, b = ep >> 1;
            if (a < b) {
                h = a;
                p = dm;
            } else if (b < a) {
                h = b;
                p = dp | UNI_SIGN;
            } else if (dp | dm) {
                *err = 1u;  // (both ends in one node: L = 1)
            }
        }
        head[i] = h;
        posg[i] = p;
        first[i] = h == (uint32_t)i ? 1u : 0u;
    }
}

// kernel-resource-usage (gfx950, hipcc -O3): 18 VGPRs, 34 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_row_kernel(uint32_t n, uint32_t k, UniRank r, const uint32_t *__restrict__ first,
                                                           const u64 *__restrict__ uidx, const uint8_t *__restrict__ circ, u64 nu,
                                                           uint32_t *__restrict__ ulen, u64 *__restrict__ rows) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        if (!first[i]) continue;
        const u64 u = uidx[i];
        if (u >= nu) continue;  // (never)
        const uint32_t L = r.hops[2 * i] + r.hops[2 * i + 1] + 1u;
        ulen[u] = L + k - 1u;
        rows[KH_UNI_WORDS * u + KH_UNI_KMERS] = L;
        rows[KH_UNI_WORDS * u + KH_UNI_COUNT_SUM] = 0;
        rows[KH_UNI_WORDS * u + KH_UNI_FLAGS] = circ[i] ? KH_UNI_CIRCULAR : 0;
    }
}

// Node q of the order array is the q-th k-mer of the base array's unitigs: unitig u's nodes start at ustart[u] - u (k - 1).
// kernel-resource-usage (gfx950, hipcc -O3): 18 VGPRs, 41 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_place_kernel(uint32_t n, uint32_t k, const uint32_t *__restrict__ head, const uint32_t *__restrict__ posg,
                                                             const u64 *__restrict__ uidx, const u64 *__restrict__ ustart, u64 nu,
                                                             uint32_t *__restrict__ order, uint32_t *__restrict__ ordu, u64 *__restrict__ rows,
                                                             uint32_t *__restrict__ err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const uint32_t h = head[i], pg = posg[i];
        const u64 u = h < n ? uidx[h] : nu;
        if (u >= nu) {
            *err = 1u;
            continue;
        }
        const u64 st = ustart[u];
        const u64 q = st - u * (k - 1u) + (pg & ~UNI_SIGN);
        if (q >= n) {
            *err = 1u;
            continue;
        }
        order[q] = (uint32_t)i | (pg & UNI_SIGN);
        ordu[q] = (uint32_t)u;
        if (h == (uint32_t)i) rows[KH_UNI_WORDS * u + KH_UNI_START] = st;
    }
}

// COUNT_SUM: lanes of a wave that hold nodes of one unitig are neighbours; a segmented scan over the wave (six shuffle steps),
// then the last lane of every run adds the run's sum to its row -- one atomic per (wave, unitig).
// kernel-resource-usage (gfx950, hipcc -O3): 21 VGPRs, 46 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_sum_kernel(uint32_t n, const uint32_t *__restrict__ order, const uint32_t *__restrict__ ordu,
                                                           const u64 *__restrict__ counts, u64 nu, u64 *__restrict__ rows) {
    const uint32_t lane = lane_id();
    for (u64 base = (u64)blockIdx.x * BLOCK; base < n; base += (u64)gridDim.x * BLOCK) {  // (uniform: every lane shuffles)
        const u64 q = base + threadIdx.x;
        uint32_t u = 0xFFFFFFFFu;
        u64 v = 0;
        if (q < n) {
            u = ordu[q];
            const uint32_t id = order[q] & ~UNI_SIGN;
            v = id < n ? counts[id] : 0;
        }
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const u64 vu = __shfl_up(v, d, 64);
            const uint32_t uu = (uint32_t)__shfl_up((int)u, d, 64);
            if (lane >= d && uu == u) v += vu;
        }
        const uint32_t un = (uint32_t)__shfl_down((int)u, 1, 64);
        if (q < n && u < nu && (lane == 63 || un != u))
            (void)__hip_atomic_fetch_add(&rows[KH_UNI_WORDS * (u64)u + KH_UNI_COUNT_SUM], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Bytes [16 g, 16 g + 16) of the base array.  The unitig of the first byte by bisection of ustart (nu + 1 entries), the following
// ones by stepping on.  Byte o of unitig u: o < k - 1 is letter o of its first node, else the LAST letter of node o - (k - 1).
// kernel-resource-usage (gfx950, hipcc -O3): 28 VGPRs, 59 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_bases_kernel(const u64 *__restrict__ keys, uint32_t n, uint32_t k, const uint32_t *__restrict__ order,
                                                             const u64 *__restrict__ ustart, u64 nu, u64 nbases, uint8_t *__restrict__ bases) {
    const u64 ngroups = (nbases + 15) / 16;
    for (u64 g = (u64)blockIdx.x * BLOCK + threadIdx.x; g < ngroups; g += (u64)gridDim.x * BLOCK) {
        const u64 b0 = 16 * g;
        u64 lo = 0, hi = nu;
        for (int it = 0; it < 64 && hi - lo > 1; ++it) {
            const u64 mid = lo + (hi - lo) / 2;
            if (ustart[mid] <= b0) lo = mid;
            else hi = mid;
        }
        u64 u = lo, ust = ustart[u], unext = ustart[u + 1];
        u64 lastq = ~0ull, w = 0;
        uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (uint32_t j = 0; j < 16; ++j) {
            const u64 b = b0 + j;
            if (b >= nbases) break;
            for (int a = 0; a < 17 && b >= unext && u + 1 < nu; ++a) {  // (a unitig has at least one byte)
                ++u;
                ust = unext;
                unext = ustart[u + 1];
            }
            const u64 o = b - ust, ns = ust - u * (k - 1u);
            u64 q = o < k - 1u ? ns : ns + o - (k - 1u);
            const uint32_t li = o < k - 1u ? (uint32_t)o : k - 1u;
            if (q >= n) q = n - 1;  // (never: a guard, not a path)
            if (q != lastq) {
                const uint32_t rec = order[q];
                const uint32_t id = rec & ~UNI_SIGN;
                w = kh_unitig_spell(keys[id < n ? id : 0], k, rec >> 31);
                lastq = q;
            }
            word[j >> 2] |= (uint32_t)kh_unitig_letter(w, k, li) << (8u * (j & 3u));
        }
        if (b0 + 16 <= nbases) {
            *reinterpret_cast<uint4 *>(bases + b0) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {  // the cut group at the end of the array
            for (uint32_t j = 0; j < 16 && b0 + j < nbases; ++j) bases[b0 + j] = (uint8_t)(word[j >> 2] >> (8u * (j & 3u)));
        }
    }
}

// ---- links between unitigs (kh_unitigs_begin_linked) ------------------------------------------------------------------------
// End state t = 2 u + e of unitig u: e = 0 the last oriented node of its reading, e = 1 rev() of its first.  Its node and sign
// from the order array; false where the row or the order array is inconsistent (never).
__device__ __forceinline__ bool unitig_end_state(u64 t, uint32_t n, uint32_t k, const u64 *__restrict__ rows, const uint32_t *__restrict__ order,
                                                 uint32_t *id, uint32_t *sign) {
    const u64 u = t >> 1;
    const uint32_t e = (uint32_t)t & 1u;
    const u64 st = rows[KH_UNI_WORDS * u + KH_UNI_START], L = rows[KH_UNI_WORDS * u + KH_UNI_KMERS];
    const u64 q = st - u * (k - 1u) + (e ? 0 : L - 1);
    *id = 0;
    *sign = e;
    if (q >= n) return false;
    const uint32_t rec = order[q];
    *id = rec & ~UNI_SIGN;
    *sign = (rec >> 31) ^ e;
    return *id < n;
}

// kernel-resource-usage (gfx950, hipcc -O3): 18 VGPRs, 33 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void unitig_end_degree_kernel(uint32_t n, uint32_t k, u64 nu, const u64 *__restrict__ rows,
                                                                  const uint32_t *__restrict__ order, const uint8_t *__restrict__ masks,
                                                                  uint32_t *__restrict__ deg, uint32_t *__restrict__ err) {
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t < 2 * nu; t += (u64)gridDim.x * BLOCK) {
        uint32_t id, sign, d = 0;
        if (unitig_end_state(t, n, k, rows, order, &id, &sign)) d = (uint32_t)__builtin_popcount(kh_unitig_out_bits(masks[id], sign));
        else *err = 1u;
        deg[t] = d;
    }
}

__device__ __forceinline__ void link_cswap(u64 &a, u64 &b) {
    const u64 lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// Per end state: its up to four successors, all first-slot loads in flight before any probe is walked (as graph_mask_of), each
// successor's slot -> node id -> unitig, position and sign in the reading -> the link word; the words sorted in registers (absent
// ones are ~0 and go last) and stored at the lane's offset.
// kernel-resource-usage (gfx950, hipcc -O3), PfNarrow / PfWide: 64 / 73 VGPRs (four probes in flight), 96 / 91 SGPRs, no LDS, no scratch, no spills,
// 8 / 6 waves per SIMD.
template <typename PRB>
__global__ __launch_bounds__(BLOCK) void unitig_link_out_kernel(const u64 *__restrict__ keys, uint32_t n, uint32_t k, PRB prb, u64 cap, u64 nu,
                                                                const u64 *__restrict__ rows, const uint32_t *__restrict__ order,
                                                                const uint32_t *__restrict__ slot2id, const uint8_t *__restrict__ masks,
                                                                const uint32_t *__restrict__ head, const uint32_t *__restrict__ posg,
                                                                const u64 *__restrict__ uidx, const u64 *__restrict__ off, u64 n_links,
                                                                u64 *__restrict__ links, uint32_t *__restrict__ err) {
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t < 2 * nu; t += (u64)gridDim.x * BLOCK) {
        uint32_t id, sign;
        const bool ok = unitig_end_state(t, n, k, rows, order, &id, &sign);
        const u64 x = keys[id];
        const uint32_t bits = ok ? kh_unitig_out_bits(masks[id], sign) : 0u;
        u64 y[4];
        uint32_t ys[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            uint64_t yy;
            bool yp;
            kh_unitig_successor(x, k, sign, kh_unitig_letter_of_bit(j, sign), &yy, &ys[j], &yp);
            y[j] = ((bits >> j) & 1u) ? yy : x;  // (a key that is there: the probe below needs no branch)
        }
        typename PRB::Ref ref[4];
        typename PRB::Word first[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ref[j] = prb.ref(y[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) first[j] = PRB::load(ref[j]);  // (all four first-slot loads in flight)
        u64 w0 = ~0ull, w1 = ~0ull, w2 = ~0ull, w3 = ~0ull;
        bool bad = !ok;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const u64 slot = prb.resolve_slot(ref[j], first[j]);
            u64 w = ~0ull;
            if ((bits >> j) & 1u) {
                const uint32_t yid = slot < cap ? slot2id[slot] : n;
                const uint32_t h = yid < n ? head[yid] : n;
                const u64 ju = h < n ? uidx[h] : nu;
                uint32_t es = KH_UNI_ENTER_NONE;
                if (ju < nu) {
                    const uint32_t pg = posg[yid];
                    es = kh_unitig_enter_sign(pg & ~UNI_SIGN, (uint32_t)rows[KH_UNI_WORDS * ju + KH_UNI_KMERS], pg >> 31, ys[j]);
                }
                if (es == KH_UNI_ENTER_NONE) bad = true;
                else w = kh_unitig_link_word((uint32_t)(t >> 1), (uint32_t)t & 1u, (uint32_t)ju, es);
            }
            if (j == 0) w0 = w;
            else if (j == 1) w1 = w;
            else if (j == 2) w2 = w;
            else w3 = w;
        }
        if (bad) *err = 1u;
        link_cswap(w0, w1);
        link_cswap(w2, w3);
        link_cswap(w0, w2);
        link_cswap(w1, w3);
        link_cswap(w1, w2);
        const u64 o = off[t], d = off[t + 1] - o;  // (d = popcount(bits), by unitig_end_degree_kernel)
        if (o + d > n_links || d > 4) {
            *err = 1u;
            continue;
        }
        if (d > 0) links[o] = w0;
        if (d > 1) links[o + 1] = w1;
        if (d > 2) links[o + 2] = w2;
        if (d > 3) links[o + 3] = w3;
    }
}

// ---- tip clipping (kh_clip_tips_into) -----------------------------------------------------------------------------------------
// The links of end state t = 2 i + s are links[loff[t] .. loff[t + 1]): the array is sorted by from-state.
// Per unitig: 0 = no candidate, 1 = candidate attached at its + end, 2 = at its - end (the rule: include/kmerhip.h).  No probes.
// kernel-resource-usage (gfx950, hipcc -O3): 22 VGPRs, 48 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void clip_candidate_kernel(u64 nu, u64 nl, u64 max_kmers, const u64 *__restrict__ rows, const u64 *__restrict__ loff,
                                                               const u64 *__restrict__ links, uint8_t *__restrict__ cand, uint32_t *__restrict__ err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nu; i += (u64)gridDim.x * BLOCK) {
        const u64 kmers = rows[KH_UNI_WORDS * i + KH_UNI_KMERS], flags = rows[KH_UNI_WORDS * i + KH_UNI_FLAGS];
        const u64 o0 = loff[2 * i], o1 = loff[2 * i + 1], o2 = loff[2 * i + 2];
        const u64 dp = o1 - o0, dm = o2 - o1;
        uint32_t c = 0;
        if (o0 > o1 || o1 > o2 || o2 > nl || dp > 4 || dm > 4) {
            *err = 1u;
        } else if (!(flags & KH_UNI_CIRCULAR) && kmers <= max_kmers && (dp == 0) != (dm == 0)) {
            const uint32_t s = dp ? 0u : 1u;
            const u64 a0 = s ? o1 : o0, d = s ? dm : dp;
            bool self = false;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (j < d && KH_UNI_LINK_TO(links[a0 + j]) == (uint32_t)i) self = true;
            c = self ? 0u : 1u + s;
        }
        cand[i] = (uint8_t)c;
    }
}

// Per candidate: its up to four links, for each the up to four links out of the state it enters, reversed -- the rivals --, their
// candidate bytes and rows (kh_clip_beats) -> one clipped byte.  The four second-level offset pairs are loaded before any is
// used.  The first six words of kh_clip_tips_into: per-lane sums, one reduction per wave and word, one atomic by its lane 0.
// kernel-resource-usage (gfx950, hipcc -O3): 51 VGPRs, 90 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void clip_decide_kernel(u64 nu, u64 nl, const u64 *__restrict__ rows, const u64 *__restrict__ loff,
                                                            const u64 *__restrict__ links, const uint8_t *__restrict__ cand,
                                                            uint8_t *__restrict__ clipped, uint32_t *__restrict__ err, u64 *__restrict__ words) {
    u64 s_uni = 0, s_links = 0, s_cand = 0, s_clip = 0, s_kmers = 0, s_count = 0;
    bool bad = false;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nu; i += (u64)gridDim.x * BLOCK) {
        const uint32_t ci = cand[i];
        s_uni += 1;
        s_links += loff[2 * i + 2] - loff[2 * i];
        uint32_t cl = 0;
        if (ci) {
            const u64 ti = 2 * i + (ci - 1u);
            const u64 a0 = loff[ti];
            u64 d = loff[ti + 1] - a0;
            if (d < 1 || d > 4 || a0 + d > nl) {  // (never: clip_candidate_kernel saw the same offsets)
                bad = true;
                d = 0;
            }
            const u64 ki = rows[KH_UNI_WORDS * i + KH_UNI_KMERS], si = rows[KH_UNI_WORDS * i + KH_UNI_COUNT_SUM];
            u64 tt[4], lo[4], hi[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                tt[j] = ti;  // (a state that is there: the loads below need no branch)
                if (j < d) {
                    const u64 t = (links[a0 + j] & 0xFFFFFFFFull) ^ 1ull;  // (j, 1 - t): the entered state, reversed
                    if (t < 2 * nu) tt[j] = t;
                    else bad = true;
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) lo[j] = loff[tt[j]];  // (all four offset pairs in flight)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) hi[j] = loff[tt[j] + 1];
            bool all = d > 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                if (j >= d) continue;
                u64 e = hi[j] - lo[j];
                if (lo[j] > hi[j] || e > 4 || hi[j] > nl) {
                    bad = true;
                    e = 0;
                }
                bool found = false, beaten = false;
#pragma unroll
                for (uint32_t m = 0; m < 4; ++m) {
                    if (m >= e) continue;
                    const uint32_t b = KH_UNI_LINK_TO(links[lo[j] + m]);
                    if (b == (uint32_t)i) {
                        found = true;
                    } else if (b < nu) {
                        const bool cb = cand[b] != 0;
                        if (!cb || kh_clip_beats(rows[KH_UNI_WORDS * (u64)b + KH_UNI_KMERS], rows[KH_UNI_WORDS * (u64)b + KH_UNI_COUNT_SUM], b, true, ki, si,
                                                 (uint32_t)i))
                            beaten = true;
                    } else {
                        bad = true;
                    }
                }
                if (!found) bad = true;  // i is not among its own rivals
                all = all && beaten;
            }
            cl = all ? 1u : 0u;
            s_cand += 1;
            if (cl) {
                s_clip += 1;
                s_kmers += ki;
                s_count += si;
            }
        }
        clipped[i] = (uint8_t)cl;
    }
    if (kh_any(bad) && lane_id() == 0) *err = 1u;
    s_uni = wave_sum(s_uni);
    s_links = wave_sum(s_links);
    s_cand = wave_sum(s_cand);
    s_clip = wave_sum(s_clip);
    s_kmers = wave_sum(s_kmers);
    s_count = wave_sum(s_count);
    if (lane_id() == 0) {
        if (s_uni) atomicAdd(&words[KH_CLIP_UNITIGS], s_uni);
        if (s_links) atomicAdd(&words[KH_CLIP_LINKS], s_links);
        if (s_cand) atomicAdd(&words[KH_CLIP_CANDIDATES], s_cand);
        if (s_clip) atomicAdd(&words[KH_CLIP_CLIPPED], s_clip);
        if (s_kmers) atomicAdd(&words[KH_CLIP_CLIPPED_KMERS], s_kmers);
        if (s_count) atomicAdd(&words[KH_CLIP_CLIPPED_COUNT], s_count);
    }
}

// Nodes [q0, q1) of the unitig order: a node of a surviving unitig hands (keys[id], counts[id]) to the target table, count += c
// as table_merge_pairs_kernel, whose counters it keeps; the two kept words as above.
// kernel-resource-usage (gfx950, hipcc -O3): 33 VGPRs, 73 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void clip_keep_kernel(TableGeom tg, u64 q0, u64 q1, uint32_t n, u64 nu, const uint32_t *__restrict__ order,
                                                          const uint32_t *__restrict__ ordu, const uint8_t *__restrict__ clipped,
                                                          const u64 *__restrict__ keys, const u64 *__restrict__ counts, Counters *ctr,
                                                          u64 *__restrict__ words) {
    uint32_t nd = 0, nf = 0;
    u64 ad = 0, np = 0;
    for (u64 q = q0 + (u64)blockIdx.x * BLOCK + threadIdx.x; q < q1; q += (u64)gridDim.x * BLOCK) {
        const uint32_t u = ordu[q], id = order[q] & ~UNI_SIGN;
        if (u >= nu || id >= n || clipped[u]) continue;
        const u64 key = keys[id], c = counts[id];
        if (key != KH_EMPTY_KEY && c != 0) {
            upsert(tg, key, c, nd, nf);
            ad += c;
            np += 1;
        }
    }
    const u64 d = wave_sum((u64)nd), f = wave_sum((u64)nf);
    ad = wave_sum(ad);
    np = wave_sum(np);
    if (lane_id() == 0) {
        if (d) atomicAdd(&ctr->distinct, d);
        if (f) atomicAdd(&ctr->failed, f);
        if (ad) atomicAdd(&ctr->kmers, ad);
        if (np) atomicAdd(&words[KH_CLIP_KEPT_KMERS], np);
        if (ad) atomicAdd(&words[KH_CLIP_KEPT_COUNT], ad);
    }
}

// ---- bubble popping (kh_pop_bubbles_into) -------------------------------------------------------------------------------------
static_assert(KH_POP_KEPT_KMERS == KH_CLIP_KEPT_KMERS && KH_POP_KEPT_COUNT == KH_CLIP_KEPT_COUNT && KH_POP_WORDS >= KH_CLIP_WORDS,
              "clip_keep_kernel writes the kept words of both rules");
static_assert(KH_DROP_KEPT_KMERS == KH_CLIP_KEPT_KMERS && KH_DROP_KEPT_COUNT == KH_CLIP_KEPT_COUNT && KH_DROP_UNITIGS == KH_CLIP_UNITIGS &&
                  KH_DROP_LINKS == KH_CLIP_LINKS && KH_DROP_WORDS <= KH_POP_WORDS,
              "clip_keep_kernel writes the kept words of the drop rule too, clip_step() checks its unitigs and links, ClipJob holds its words");
#define KH_POP_NO_EXITS (~0ull)  // no candidate (a to-state is below 2^32 - 2: no pair of them gives this word)

// Per unitig: the unordered pair of the states its two ends enter, min << 32 | max, where it is a candidate (the rule:
// include/kmerhip.h), else KH_POP_NO_EXITS.  No probes.
// kernel-resource-usage (gfx950, hipcc -O3): 22 VGPRs, 44 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void pop_exits_kernel(u64 nu, u64 nl, u64 max_kmers, const u64 *__restrict__ rows, const u64 *__restrict__ loff,
                                                          const u64 *__restrict__ links, u64 *__restrict__ exits, uint32_t *__restrict__ err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nu; i += (u64)gridDim.x * BLOCK) {
        const u64 kmers = rows[KH_UNI_WORDS * i + KH_UNI_KMERS], flags = rows[KH_UNI_WORDS * i + KH_UNI_FLAGS];
        const u64 o0 = loff[2 * i], o1 = loff[2 * i + 1], o2 = loff[2 * i + 2];
        u64 e = KH_POP_NO_EXITS;
        if (o0 > o1 || o1 > o2 || o2 > nl || o1 - o0 > 4 || o2 - o1 > 4) {
            *err = 1u;
        } else if (!(flags & KH_UNI_CIRCULAR) && kmers <= max_kmers && o1 - o0 == 1 && o2 - o1 == 1) {
            const u64 tp = links[o0] & 0xFFFFFFFFull, tm = links[o1] & 0xFFFFFFFFull;
            if ((tp >> 1) != i && (tm >> 1) != i) e = tp < tm ? (tp << 32) | tm : (tm << 32) | tp;
        }
        exits[i] = e;
    }
}

// Per candidate: the state its + link enters, reversed; the up to four links out of that state lead to the unitigs that enter the
// same place, i among them; those with i's exit word are its parallels, and kh_pop_beats on their rows gives the popped byte.  The
// four link words, and then the four exit words, are loaded before any is used; rows only of the parallels.  Seven words of
// kh_pop_bubbles_into: per-lane sums, one reduction per wave and word, one atomic by its lane 0.
// kernel-resource-usage (gfx950, hipcc -O3): 88 VGPRs (four link words, four exit words and the unrolled 128-bit products), 88 SGPRs,
// no LDS, no scratch, no spills, 5 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void pop_decide_kernel(u64 nu, u64 nl, const u64 *__restrict__ rows, const u64 *__restrict__ loff,
                                                           const u64 *__restrict__ links, const u64 *__restrict__ exits,
                                                           uint8_t *__restrict__ popped, uint32_t *__restrict__ err, u64 *__restrict__ words) {
    u64 s_uni = 0, s_links = 0, s_cand = 0, s_pop = 0, s_kmers = 0, s_count = 0, s_bub = 0;
    bool bad = false;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nu; i += (u64)gridDim.x * BLOCK) {
        const u64 ei = exits[i];
        const u64 a0 = loff[2 * i];
        s_uni += 1;
        s_links += loff[2 * i + 2] - a0;
        uint32_t po = 0;
        if (ei != KH_POP_NO_EXITS && a0 >= nl) bad = true;  // (never: pop_exits_kernel saw the same offsets)
        if (ei != KH_POP_NO_EXITS && a0 < nl) {
            u64 t = (links[a0] & 0xFFFFFFFFull) ^ 1ull;  // the state its + end enters, reversed
            if (t >= 2 * nu) {
                bad = true;
                t = 2 * i;  // (a state that is there)
            }
            const u64 lo = loff[t], hi = loff[t + 1];
            u64 e = hi - lo;
            if (lo > hi || e > 4 || hi > nl) {
                bad = true;
                e = 0;
            }
            const u64 ki = rows[KH_UNI_WORDS * i + KH_UNI_KMERS], si = rows[KH_UNI_WORDS * i + KH_UNI_COUNT_SUM];
            u64 w[4], ex[4];
            uint32_t b[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) w[j] = links[j < e ? lo + j : a0];  // (all four link words in flight; a0: a word that is there)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) b[j] = KH_UNI_LINK_TO(w[j]);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) ex[j] = exits[b[j] < nu ? (u64)b[j] : i];  // (all four exit words in flight)
            bool found = false, par = false, beaten = false;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                if (j >= e) continue;
                if (b[j] == (uint32_t)i) {
                    found = true;
                } else if (b[j] >= nu) {
                    bad = true;
                } else if (ex[j] == ei) {
                    par = true;
                    if (kh_pop_beats(rows[KH_UNI_WORDS * (u64)b[j] + KH_UNI_KMERS], rows[KH_UNI_WORDS * (u64)b[j] + KH_UNI_COUNT_SUM], b[j], ki, si, (uint32_t)i))
                        beaten = true;
                }
            }
            if (!found) bad = true;  // i is not among the unitigs that enter its own exit
            po = beaten ? 1u : 0u;
            s_cand += 1;
            if (po) {
                s_pop += 1;
                s_kmers += ki;
                s_count += si;
            } else if (par) {
                s_bub += 1;
            }
        }
        popped[i] = (uint8_t)po;
    }
    if (kh_any(bad) && lane_id() == 0) *err = 1u;
    s_uni = wave_sum(s_uni);
    s_links = wave_sum(s_links);
    s_cand = wave_sum(s_cand);
    s_pop = wave_sum(s_pop);
    s_kmers = wave_sum(s_kmers);
    s_count = wave_sum(s_count);
    s_bub = wave_sum(s_bub);
    if (lane_id() == 0) {
        if (s_uni) atomicAdd(&words[KH_POP_UNITIGS], s_uni);
        if (s_links) atomicAdd(&words[KH_POP_LINKS], s_links);
        if (s_cand) atomicAdd(&words[KH_POP_CANDIDATES], s_cand);
        if (s_pop) atomicAdd(&words[KH_POP_POPPED], s_pop);
        if (s_kmers) atomicAdd(&words[KH_POP_POPPED_KMERS], s_kmers);
        if (s_count) atomicAdd(&words[KH_POP_POPPED_COUNT], s_count);
        if (s_bub) atomicAdd(&words[KH_POP_BUBBLES], s_bub);
    }
}

}  // namespace kh

namespace khi {

void unitigs_release(kh_ctx *c) {
    unitigs_text_release(c);  // (a text stream belongs to these unitigs)
    if (c->un.rows) (void)dev_free(c->un.rows);  // (synchronises the device)
    if (c->un.bases) (void)dev_free(c->un.bases);
    if (c->un.links) (void)dev_free(c->un.links);
    if (c->un.where) (void)dev_free(c->un.where);  // (the place map of kh_unitigs_locate*, locate.hip)
    if (c->un.link_first) (void)dev_free(c->un.link_first);  // (the link index of kh_unitigs_link_support*, support.hip)
    if (c->un.comp_rows) (void)dev_free(c->un.comp_rows);  // (the labels of kh_unitigs_components*, components.hip: rows and ids in one)
    c->un = kh_ctx::Unitigs();
}

namespace {

// The chain ranking over `states` states: init into *cur, then rounds that ping-pong between *cur and *oth until nothing changes
// or the bound is reached.  *open = the last round still changed something: states on cycles.
int unitig_rank(kh_ctx *c, const uint32_t *next, u64 states, kh::UniRank *cur, kh::UniRank *oth, uint32_t *d_flag, bool *open) {
    hipLaunchKernelGGL(kh::unitig_rank_init_kernel, dim3(uni_grid(states)), dim3(kh::BLOCK), 0, c->stream, next, states, *cur);
    HIP_TRY(c, hipGetLastError());
    uint32_t rounds = 1;  // ceil(log2(states)) + 1
    while ((1ull << (rounds - 1)) < states) ++rounds;
    *open = true;
    for (uint32_t r = 0; r < rounds; ++r) {
        HIP_TRY(c, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(kh::unitig_rank_round_kernel, dim3(uni_grid(states)), dim3(kh::BLOCK), 0, c->stream, next, states, *cur, *oth, d_flag);
        HIP_TRY(c, hipGetLastError());
        uint32_t changed = 0;
        HIP_TRY(c, hipMemcpyAsync(&changed, d_flag, sizeof(changed), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::swap(*cur, *oth);
        if (!changed) {
            *open = false;
            break;
        }
    }
    return KH_OK;
}

// The three rules that remove unitigs behind the links: which decision kernels run in front of the keep loop.
enum ClipMode { CLIP_TIPS, CLIP_BUBBLES, CLIP_COMPONENTS };
inline u64 clip_words(ClipMode m) { return m == CLIP_TIPS ? KH_CLIP_WORDS : m == CLIP_BUBBLES ? KH_POP_WORDS : KH_DROP_WORDS; }

// kh_clip_tips_into / kh_pop_bubbles_into / kh_drop_components_into: the rule, the target and the rule's bound in, the eight / nine words out.
struct ClipJob {
    ClipMode mode;
    kh_ctx *dst;
    u64 max_kmers;            // (kh_drop_components_into: its min_kmers)
    u64 words[KH_POP_WORDS];  // (KH_CLIP_WORDS of them for the tips)
    bool on_dst;              // a failure came from dst's side: its text is there already
};

// One round of tip clipping, bubble popping or component dropping behind the links of c, while unitigs_build's scratch is live: the
// rule's decision kernels on c's stream -- they leave one "removed" byte per unitig --, then the surviving nodes into job->dst on ITS stream, in
// ranges it has room for (as combine_scan of join.hip).  Every failure before the first insert leaves dst as it was.
int clip_step(kh_ctx *c, ClipJob *job, CallScratch &sc, u64 n, u64 nu, u64 nl, const u64 *keys, const u64 *counts, const uint32_t *order,
              const uint32_t *ordu, const u64 *loff, uint32_t *d_err) {
    kh_ctx *const dst = job->dst;
    const bool pop = job->mode == CLIP_BUBBLES, drop = job->mode == CLIP_COMPONENTS;
    const u64 nwords = clip_words(job->mode);
    // the tips' candidate bytes / the bubbles' exit words / the components' labels
    void *const cand = sc.take(drop ? nu * sizeof(uint32_t) : pop ? nu * sizeof(u64) : nu);
    u64 *const sums = drop ? (u64 *)sc.take(nu * KH_CSUM_WORDS * sizeof(u64)) : nullptr;  // (per root: components.hip)
    uint8_t *const clipped = (uint8_t *)sc.take(nu);
    u64 *const words = (u64 *)sc.take(nwords * sizeof(u64));
    if (!cand || !clipped || !words || (drop && !sums))
        return soft_oom(c, drop  ? "device memory for the component dropping's scratch"
                           : pop ? "device memory for the bubble popping's scratch"
                                 : "device memory for the tip clipping's scratch");
    HIP_TRY(c, hipMemsetAsync(words, 0, nwords * sizeof(u64), c->stream));
    if (drop) {
        u64 rounds = 0;
        int rc = components_label(c, (uint32_t *)cand, sums, d_err - 1, &rounds);  // (d_err - 1: unitigs_build's "something changed" word, idle by now)
        if (rc == KH_OK) rc = components_drop_launch(c, (const uint32_t *)cand, sums, loff, job->max_kmers, clipped, words);
        if (rc != KH_OK) return rc;
    } else if (pop) {
        hipLaunchKernelGGL(kh::pop_exits_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, nu, nl, job->max_kmers, (const u64 *)c->un.rows, loff,
                           (const u64 *)c->un.links, (u64 *)cand, d_err);
        hipLaunchKernelGGL(kh::pop_decide_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, nu, nl, (const u64 *)c->un.rows, loff,
                           (const u64 *)c->un.links, (const u64 *)cand, clipped, d_err, words);
    } else {
        hipLaunchKernelGGL(kh::clip_candidate_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, nu, nl, job->max_kmers, (const u64 *)c->un.rows, loff,
                           (const u64 *)c->un.links, (uint8_t *)cand, d_err);
        hipLaunchKernelGGL(kh::clip_decide_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, nu, nl, (const u64 *)c->un.rows, loff,
                           (const u64 *)c->un.links, (const uint8_t *)cand, clipped, d_err, words);
    }
    HIP_TRY(c, hipGetLastError());
    uint32_t bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, d_err, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(job->words, words, nwords * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the clipped bytes are complete: dst's stream may read them)
    if (bad || job->words[KH_CLIP_UNITIGS] != nu || job->words[KH_CLIP_LINKS] != nl)
        return fail(c, KH_ERR_STATE, drop  ? "kh_drop_components_into: the unitigs or the links do not add up (internal error)"
                                     : pop ? "kh_pop_bubbles_into: a candidate is not among the unitigs that enter its own exit, or the links do not add up (internal error)"
                                           : "kh_clip_tips_into: a candidate is not among its own rivals, or the links do not add up (internal error)");
    int rc = KH_OK;
    job->on_dst = true;
    const u64 step = SUB_TILES * kh::TILE;
    for (u64 q0 = 0; q0 < n && rc == KH_OK;) {
        const u64 m = std::min(step, n - q0);
        bool smaller = false;
        if ((rc = ensure_room(dst, m, false, &smaller)) != KH_OK) break;
        hipLaunchKernelGGL(kh::clip_keep_kernel, dim3(uni_grid(m)), dim3(kh::BLOCK), 0, dst->stream, table_geom(dst, dst->table, dst->cap), q0, q0 + m,
                           (uint32_t)n, nu, order, ordu, (const uint8_t *)clipped, keys, counts, dst->d_ctr, words);
        if (hipGetLastError() != hipSuccess) rc = fail(dst, KH_ERR_HIP, "clip_keep_kernel");
        dst->table_empty = false;
        dst->rheads_valid = false;
        dst->pending_bound += m;
        q0 += m;
    }
    if (rc == KH_OK && hipMemcpyAsync(job->words + KH_CLIP_KEPT_KMERS, words + KH_CLIP_KEPT_KMERS, 2 * sizeof(u64), hipMemcpyDeviceToHost, dst->stream) != hipSuccess)
        rc = fail(dst, KH_ERR_HIP, drop ? "kh_drop_components_into: the kept words" : pop ? "kh_pop_bubbles_into: the kept words" : "kh_clip_tips_into: the kept words");
    if (rc == KH_OK) rc = sync_counters(dst);  // (complete when it returns; an upsert without a free slot shows here)
    else (void)hipStreamSynchronize(dst->stream);  // (before the scratch goes back)
    return rc;
}

// linked: kh_unitigs_begin_linked -- the link array behind the same kernels; nothing of it is launched or allocated without.
// clip: kh_clip_tips_into / kh_pop_bubbles_into / kh_drop_components_into -- linked, without the base array, and clip_step() behind the links.
int unitigs_build(kh_ctx *c, u64 n, u64 mc, CallScratch &sc, bool linked, ClipJob *clip = nullptr) {
    const uint32_t n32 = (uint32_t)n, k = c->k;
    const u64 states = 2 * n;
    u64 *const keys = (u64 *)sc.take(n * sizeof(u64));
    u64 *const counts = (u64 *)sc.take(n * sizeof(u64));
    if (!keys || !counts) return soft_oom(c, "device memory for the unitigs' nodes");
    int rc = sorted_into(c, keys, counts, n, mc, sc);
    if (rc != KH_OK) return rc;
    uint32_t *const slot2id = (uint32_t *)sc.take(c->cap * sizeof(uint32_t));
    uint8_t *const masks = (uint8_t *)sc.take(n);
    uint8_t *const circ = (uint8_t *)sc.take(n);
    uint32_t *const next = (uint32_t *)sc.take(states * sizeof(uint32_t));
    uint32_t *const rank = (uint32_t *)sc.take(6 * states * sizeof(uint32_t));
    u64 *const uidx = (u64 *)sc.take((n + 1) * sizeof(u64));
    uint32_t *const d_flag = (uint32_t *)sc.take(2 * sizeof(uint32_t));  // "something changed", "something is inconsistent"
    u64 *const scan = (u64 *)sc.take(device_scan_scratch(2 * n));  // for the scans below, of n, nu <= n and 2 nu entries (not the context's scratch: nothing of this call stays allocated)
    if (!slot2id || !masks || !circ || !next || !rank || !uidx || !d_flag || !scan) return soft_oom(c, "device memory for the unitigs' scratch");
    kh::UniRank cur{rank, rank + states, rank + 2 * states}, oth{rank + 3 * states, rank + 4 * states, rank + 5 * states};
    HIP_TRY(c, hipMemsetAsync(slot2id, 0xFF, c->cap * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(circ, 0, n, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_flag, 0, 2 * sizeof(uint32_t), c->stream));
    with_probe(c, [&](auto prb) {
        typedef decltype(prb) PRB;
        hipLaunchKernelGGL((kh::unitig_index_kernel<PRB>), dim3(uni_grid(n)), dim3(kh::BLOCK), 0, c->stream, (const u64 *)keys, n32, k, mc, prb,
                           c->cap, slot2id, masks);
        hipLaunchKernelGGL((kh::unitig_link_kernel<PRB>), dim3(uni_grid(n)), dim3(kh::BLOCK), 0, c->stream, (const u64 *)keys, n32, k, prb,
                           c->cap, (const uint32_t *)slot2id, (const uint8_t *)masks, next);
    });
    HIP_TRY(c, hipGetLastError());

    bool open = false;
    if ((rc = unitig_rank(c, next, states, &cur, &oth, d_flag, &open)) != KH_OK) return rc;
    if (open) {  // cycles: cut each at its smallest node and rank again
        hipLaunchKernelGGL(kh::unitig_cut_kernel, dim3(uni_grid(n)), dim3(kh::BLOCK), 0, c->stream, next, n32, cur, circ);
        HIP_TRY(c, hipGetLastError());
        if ((rc = unitig_rank(c, next, states, &cur, &oth, d_flag, &open)) != KH_OK) return rc;
        if (open) return fail(c, KH_ERR_STATE, "kh_unitigs_begin: a chain is still closed behind the cut (internal error)");
    }

    // the other rank buffer is free from here on: five arrays of n words live in it
    uint32_t *const head = oth.tgt, *const order = oth.tgt + n, *const posg = oth.hops, *const ordu = oth.hops + n, *const first = oth.mn;
    hipLaunchKernelGGL(kh::unitig_reading_kernel, dim3(uni_grid(n)), dim3(kh::BLOCK), 0, c->stream, (const uint32_t *)next, n32, cur, head, posg, first,
                       d_flag + 1);
    HIP_TRY(c, hipGetLastError());
    if ((rc = device_scan(c, first, n, uidx, true, scan)) != KH_OK) return rc;
    u64 nu = 0;
    HIP_TRY(c, hipMemcpyAsync(&nu, uidx + n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (nu == 0 || nu > n) return fail(c, KH_ERR_STATE, "kh_unitigs_begin: the first nodes do not add up (internal error)");

    uint32_t *const ulen = (uint32_t *)sc.take(nu * sizeof(uint32_t));
    u64 *const ustart = (u64 *)sc.take((nu + 1) * sizeof(u64));
    if (!ulen || !ustart) return soft_oom(c, "device memory for the unitigs' offsets");
    if (dev_malloc((void **)&c->un.rows, nu * KH_UNI_WORDS * sizeof(u64)) != hipSuccess) {
        (void)hipGetLastError();
        c->un.rows = nullptr;
        return soft_oom(c, "hipMalloc(unitig rows)");
    }
    hipLaunchKernelGGL(kh::unitig_row_kernel, dim3(uni_grid(n)), dim3(kh::BLOCK), 0, c->stream, n32, k, cur, (const uint32_t *)first, (const u64 *)uidx,
                       (const uint8_t *)circ, nu, ulen, c->un.rows);
    HIP_TRY(c, hipGetLastError());
    if ((rc = device_scan(c, ulen, nu, ustart, true, scan)) != KH_OK) return rc;
    u64 nb = 0;
    HIP_TRY(c, hipMemcpyAsync(&nb, ustart + nu, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (nb != n + nu * (k - 1)) return fail(c, KH_ERR_STATE, "kh_unitigs_begin: the unitigs' lengths do not add up (internal error)");
    if (!clip && dev_malloc((void **)&c->un.bases, nb) != hipSuccess) {
        (void)hipGetLastError();
        c->un.bases = nullptr;
        return soft_oom(c, "hipMalloc(unitig bases)");
    }
    hipLaunchKernelGGL(kh::unitig_place_kernel, dim3(uni_grid(n)), dim3(kh::BLOCK), 0, c->stream, n32, k, (const uint32_t *)head, (const uint32_t *)posg,
                       (const u64 *)uidx, (const u64 *)ustart, nu, order, ordu, c->un.rows, d_flag + 1);
    hipLaunchKernelGGL(kh::unitig_sum_kernel, dim3(uni_grid(n)), dim3(kh::BLOCK), 0, c->stream, n32, (const uint32_t *)order, (const uint32_t *)ordu,
                       (const u64 *)counts, nu, c->un.rows);
    if (!clip)
        hipLaunchKernelGGL(kh::unitig_bases_kernel, dim3(uni_grid((nb + 15) / 16)), dim3(kh::BLOCK), 0, c->stream, (const u64 *)keys, n32, k,
                           (const uint32_t *)order, (const u64 *)ustart, nu, nb, c->un.bases);
    HIP_TRY(c, hipGetLastError());
    // the links: every end state's out-degree -> offsets; their sum comes back with the consistency word
    uint32_t *deg = nullptr;
    u64 *loff = nullptr, nl = 0;
    if (linked) {
        deg = (uint32_t *)sc.take(2 * nu * sizeof(uint32_t));
        loff = (u64 *)sc.take((2 * nu + 1) * sizeof(u64));
        if (!deg || !loff) return soft_oom(c, "device memory for the unitigs' link offsets");
        hipLaunchKernelGGL(kh::unitig_end_degree_kernel, dim3(uni_grid(2 * nu)), dim3(kh::BLOCK), 0, c->stream, n32, k, nu, (const u64 *)c->un.rows,
                           (const uint32_t *)order, (const uint8_t *)masks, deg, d_flag + 1);
        HIP_TRY(c, hipGetLastError());
        if ((rc = device_scan(c, deg, 2 * nu, loff, true, scan)) != KH_OK) return rc;
        HIP_TRY(c, hipMemcpyAsync(&nl, loff + 2 * nu, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    }
    uint32_t bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, d_flag + 1, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (bad) return fail(c, KH_ERR_STATE, "kh_unitigs_begin: the chains are inconsistent (internal error)");
    if (nl > 8 * nu) return fail(c, KH_ERR_STATE, "kh_unitigs_begin_linked: the end states' degrees do not add up (internal error)");
    if (nl) {
        if (dev_malloc((void **)&c->un.links, nl * sizeof(u64)) != hipSuccess) {
            (void)hipGetLastError();
            c->un.links = nullptr;
            return soft_oom(c, "hipMalloc(unitig links)");
        }
        with_probe(c, [&](auto prb) {
            hipLaunchKernelGGL((kh::unitig_link_out_kernel<decltype(prb)>), dim3(uni_grid(2 * nu)), dim3(kh::BLOCK), 0, c->stream, (const u64 *)keys, n32, k,
                               prb, c->cap, nu, (const u64 *)c->un.rows, (const uint32_t *)order, (const uint32_t *)slot2id, (const uint8_t *)masks,
                               (const uint32_t *)head, (const uint32_t *)posg, (const u64 *)uidx, (const u64 *)loff, nl, c->un.links, d_flag + 1);
        });
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&bad, d_flag + 1, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, KH_ERR_STATE, "kh_unitigs_begin_linked: a link enters a unitig at neither end (internal error)");
    }
    c->un.n_unitigs = nu;
    c->un.n_bases = nb;
    c->un.n_links = nl;
    if (clip) return clip_step(c, clip, sc, n, nu, nl, keys, counts, order, ordu, loff, d_flag + 1);
    return KH_OK;
}

// What the two copies check before they write anything.
int unitigs_copy_enter(kh_ctx *c, const char *who, const void *rows, u64 row_cap, const void *bases, u64 base_cap) {
    if (!c) return KH_ERR_BAD_ARG;
    int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (!c->un.live)
        return fail(c, KH_ERR_STATE, (std::string(who) + ": no unitigs: kh_unitigs_begin first (anything that changes the table makes them stale)").c_str());
    if ((row_cap && !rows) || (base_cap && !bases)) return fail(c, KH_ERR_BAD_ARG, (std::string(who) + ": NULL array").c_str());
    if ((rows || row_cap) && row_cap < c->un.n_unitigs) return fail(c, KH_ERR_RANGE, (std::string(who) + ": row array too small").c_str());
    if ((bases || base_cap) && base_cap < c->un.n_bases) return fail(c, KH_ERR_RANGE, (std::string(who) + ": base array too small").c_str());
    return KH_OK;
}

}  // namespace
}  // namespace khi
using namespace khi;

namespace khi {
namespace {

int unitigs_begin(kh_ctx *c, const char *who, uint64_t min_count, uint64_t *n_unitigs, uint64_t *n_bases, uint64_t *n_links, bool linked) {
    if (!c) return KH_ERR_BAD_ARG;
    if (!n_unitigs || !n_bases || (linked && !n_links)) return fail(c, KH_ERR_BAD_ARG, (std::string(who) + ": NULL output").c_str());
    *n_unitigs = *n_bases = 0;
    if (linked) *n_links = 0;
    if (c->shard_shift)
        return fail(c, KH_ERR_STATE, (std::string(who) + ": the table is a shard; its k-mers' neighbours live on other owners").c_str());
    int rc = enter(c, ENTER_READ_TAKE);
    if (rc != KH_OK) return rc;
    unitigs_release(c);
    const u64 mc = min_count ? min_count : 1;
    uint64_t n = 0;
    if ((rc = kh_result_size(c, mc, &n)) != KH_OK) return rc;
    if (n > 0x7FFFFFFFull) return fail(c, KH_ERR_RANGE, (std::string(who) + ": more than 2^31 - 1 nodes: node ids are 32-bit").c_str());
    if (n) {
        {
            CallScratch sc(c);
            rc = unitigs_build(c, n, mc, sc, linked);
            if (rc != KH_OK) (void)hipStreamSynchronize(c->stream);  // (before the scratch goes back)
        }
        if (rc != KH_OK) {
            unitigs_release(c);
            return rc;
        }
    }
    c->un.live = true;
    c->un.linked = linked;
    *n_unitigs = c->un.n_unitigs;
    *n_bases = c->un.n_bases;
    if (linked) *n_links = c->un.n_links;
    return KH_OK;
}

// What the two link copies check before they write anything.
int links_copy_enter(kh_ctx *c, const char *who, const void *links, u64 cap) {
    if (!c) return KH_ERR_BAD_ARG;
    int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (!c->un.live)
        return fail(c, KH_ERR_STATE,
                    (std::string(who) + ": no unitigs: kh_unitigs_begin_linked first (anything that changes the table makes them stale)").c_str());
    if (!c->un.linked) return fail(c, KH_ERR_STATE, (std::string(who) + ": no links were built: kh_unitigs_begin_linked, not kh_unitigs_begin").c_str());
    if (cap && !links) return fail(c, KH_ERR_BAD_ARG, (std::string(who) + ": NULL array").c_str());
    if ((links || cap) && cap < c->un.n_links) return fail(c, KH_ERR_RANGE, (std::string(who) + ": link array too small").c_str());
    return KH_OK;
}

}  // namespace
}  // namespace khi

extern "C" int kh_unitigs_begin(kh_ctx *c, uint64_t min_count, uint64_t *n_unitigs, uint64_t *n_bases) {
    return unitigs_begin(c, "kh_unitigs_begin", min_count, n_unitigs, n_bases, nullptr, false);
}

extern "C" int kh_unitigs_begin_linked(kh_ctx *c, uint64_t min_count, uint64_t *n_unitigs, uint64_t *n_bases, uint64_t *n_links) {
    return unitigs_begin(c, "kh_unitigs_begin_linked", min_count, n_unitigs, n_bases, n_links, true);
}

namespace khi {
namespace {

// kh_clip_tips_into, kh_pop_bubbles_into and kh_drop_components_into: src's unitigs and links are built as kh_unitigs_begin_linked builds them (without the
// bases), decided by the rule of `mode` and handed on while the scratch is live, and released again: nothing of them outlives the call.
int clip_into(const char *who, ClipMode mode, kh_ctx *dst, kh_ctx *src, uint64_t min_count, uint64_t max_kmers, uint64_t *out) {
    if (!dst) return KH_ERR_BAD_ARG;
    const std::string w(who);
    if (!src || !out) return fail(dst, KH_ERR_BAD_ARG, (w + ": NULL argument").c_str());
    if (dst == src) return fail(dst, KH_ERR_BAD_ARG, (w + ": dst must not be src").c_str());
    int rc = join_check(dst, who, src, nullptr, dst);
    if (rc != KH_OK) return rc;
    if (src->shard_shift) return fail(dst, KH_ERR_STATE, (w + ": the table is a shard; its k-mers' neighbours live on other owners").c_str());
    auto from_src = [&](int r) {  // (the error text is on dst)
        if (r != KH_OK) dst->last_error = src->last_error;
        return r;
    };
    if ((rc = enter(src, ENTER_READ_TAKE)) != KH_OK) return from_src(rc);
    unitigs_release(src);
    if ((rc = enter(dst)) != KH_OK) return rc;
    const u64 mc = min_count ? min_count : 1;
    uint64_t n = 0;
    if ((rc = kh_result_size(src, mc, &n)) != KH_OK) return from_src(rc);
    if (n > 0x7FFFFFFFull) return fail(dst, KH_ERR_RANGE, (w + ": more than 2^31 - 1 nodes: node ids are 32-bit").c_str());
    ClipJob job{mode, dst, max_kmers, {0, 0, 0, 0, 0, 0, 0, 0, 0}, false};
    if (n) {
        {
            CallScratch sc(src);
            rc = unitigs_build(src, n, mc, sc, true, &job);
            if (rc != KH_OK) {
                (void)hipStreamSynchronize(src->stream);  // (before the scratch goes back)
                (void)hipStreamSynchronize(dst->stream);
            }
        }
        unitigs_release(src);
        if (rc != KH_OK) return job.on_dst ? rc : from_src(rc);
    }
    memcpy(out, job.words, clip_words(mode) * sizeof(u64));
    return KH_OK;
}

}  // namespace
}  // namespace khi

extern "C" int kh_clip_tips_into(kh_ctx *dst, kh_ctx *src, uint64_t min_count, uint64_t max_kmers, uint64_t *out) {
    return clip_into("kh_clip_tips_into", CLIP_TIPS, dst, src, min_count, max_kmers, out);
}

extern "C" int kh_pop_bubbles_into(kh_ctx *dst, kh_ctx *src, uint64_t min_count, uint64_t max_kmers, uint64_t *out) {
    return clip_into("kh_pop_bubbles_into", CLIP_BUBBLES, dst, src, min_count, max_kmers, out);
}

extern "C" int kh_drop_components_into(kh_ctx *dst, kh_ctx *src, uint64_t min_count, uint64_t min_kmers, uint64_t *out) {
    return clip_into("kh_drop_components_into", CLIP_COMPONENTS, dst, src, min_count, min_kmers, out);
}

extern "C" int kh_unitigs_links_copy_device(kh_ctx *c, uint64_t *d_links, uint64_t cap) {
    int rc = links_copy_enter(c, "kh_unitigs_links_copy_device", d_links, cap);
    if (rc != KH_OK) return rc;
    if (d_links && c->un.n_links) HIP_TRY(c, hipMemcpyAsync(d_links, c->un.links, c->un.n_links * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return KH_OK;
}

extern "C" int kh_unitigs_links_copy(kh_ctx *c, uint64_t *links, uint64_t cap) {
    int rc = links_copy_enter(c, "kh_unitigs_links_copy", links, cap);
    if (rc != KH_OK) return rc;
    if (links && c->un.n_links) rc = d2h_staged(c, links, c->un.links, c->un.n_links * sizeof(u64));
    return rc;
}

extern "C" int kh_unitigs_copy_device(kh_ctx *c, uint64_t *d_rows, uint64_t row_cap, uint8_t *d_bases, uint64_t base_cap) {
    int rc = unitigs_copy_enter(c, "kh_unitigs_copy_device", d_rows, row_cap, d_bases, base_cap);
    if (rc != KH_OK) return rc;
    if (d_rows && c->un.n_unitigs)
        HIP_TRY(c, hipMemcpyAsync(d_rows, c->un.rows, c->un.n_unitigs * KH_UNI_WORDS * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
    if (d_bases && c->un.n_bases) HIP_TRY(c, hipMemcpyAsync(d_bases, c->un.bases, c->un.n_bases, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return KH_OK;
}

extern "C" int kh_unitigs_copy(kh_ctx *c, uint64_t *rows, uint64_t row_cap, uint8_t *bases, uint64_t base_cap) {
    int rc = unitigs_copy_enter(c, "kh_unitigs_copy", rows, row_cap, bases, base_cap);
    if (rc != KH_OK) return rc;
    if (rows && c->un.n_unitigs) rc = d2h_staged(c, rows, c->un.rows, c->un.n_unitigs * KH_UNI_WORDS * sizeof(u64));
    if (rc == KH_OK && bases && c->un.n_bases) rc = d2h_staged(c, bases, c->un.bases, c->un.n_bases);
    return rc;
}

extern "C" int kh_unitigs_end(kh_ctx *c) {
    if (!c) return KH_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    unitigs_release(c);
    return KH_OK;
}
