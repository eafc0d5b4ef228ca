// locate.hip -- kh_unitigs_locate / kh_unitigs_locate_device: where on the live unitigs the canonical k-mer of every window start
// of new sequences lies (include/kmerhip.h, "LOCATED on the live unitigs").  No reference counterpart.  Two halves that the tree
// already had: the read side of profile_kernel (tile staging, Roller, eight first-slot loads in flight, results realigned through
// LDS) and resolve_slot of probe.hip.h; between them a slot-indexed place map, built once per begin from the rows and bases.
//   locate_index_kernel<PRB>       every k-mer of the unitigs' bases -> where[its slot] = (2 u + o) << 32 | j
//   locate_kernel<QUAL, TAB>       profile_kernel with one more dependent load per valid window: where[slot], 8 bytes out per start
//   kh_unitigs_locate_device       one launch over the caller's device buffers (the first call after a begin builds the map)
//   kh_unitigs_locate              the same in chunks through the pinned staging of kh_profile
#include "ctx.hip.h"
#include "locate_bits.h"
#include "probe.hip.h"

namespace kh {

constexpr int LI_RUN = 16;  // consecutive k-mers per lane of locate_index_kernel: two rounds of eight probes in flight

// The place map from the rows and bases alone.  K-mer ordinal t (over all unitigs, in row order) is node j = t - B_u of the unitig u
// with B_u <= t < B_u+1, B_u = START_u - u (k - 1) the k-mers in front of u: a binary search over the rows per lane and run, then
// the lane rolls along the bases -- START_u + j + k - 1 is the last base of node j, and stepping over a unitig's end packs k bases
// anew.  o = 1 when the reading spells the reverse complement of the node's canonical string.  Every slot has one writer (every
// node lies in one unitig once): plain stores.  A k-mer that does not resolve sets *err; the resolved ones are counted per wave
// and added to *hit, which the host holds against the number of nodes.
// kernel-resource-usage (gfx950, hipcc -O3): see DESIGN.md 4.16.
template <typename PRB>
__global__ __launch_bounds__(BLOCK) void locate_index_kernel(const u64 *__restrict__ rows, const uint8_t *__restrict__ bases, u64 nu, u64 nk,
                                                             uint32_t k, PRB prb, u64 cap, u64 *__restrict__ where, u64 *__restrict__ hit,
                                                             u64 *__restrict__ err) {
    const u64 km = kh_kmask(k), k1 = k - 1;
    const u64 nruns = (nk + LI_RUN - 1) / LI_RUN;
    uint32_t found = 0, bad = 0;
    for (u64 run = (u64)blockIdx.x * BLOCK + threadIdx.x; run < nruns; run += (u64)gridDim.x * BLOCK) {
        const u64 t0 = run * LI_RUN;
        u64 lo = 0, hi = nu;  // the last u with B_u <= t0 (B_0 = 0)
        while (hi - lo > 1) {
            const u64 mid = (lo + hi) >> 1;
            if (rows[mid * KH_UNI_WORDS + KH_UNI_START] - mid * k1 <= t0) lo = mid;
            else hi = mid;
        }
        u64 u = lo;
        u64 start = rows[u * KH_UNI_WORDS + KH_UNI_START], L = rows[u * KH_UNI_WORDS + KH_UNI_KMERS];
        u64 j = t0 - (start - u * k1);
        u64 fwd = 0;
        bool fresh = true;  // fwd does not hold the k - 1 bases in front of node j's last
#pragma unroll
        for (int half = 0; half < LI_RUN / 8; ++half) {
            u64 word[8];
            typename PRB::Ref ref[8];
            typename PRB::Word first[8];
            uint32_t ok = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const u64 t = t0 + half * 8 + i;
                u64 key = 0;
                word[i] = KH_LOC_NONE;
                if (t < nk) {
                    if (j == L) {  // (L >= 1: no loop)
                        ++u;
                        start = rows[u * KH_UNI_WORDS + KH_UNI_START];
                        L = rows[u * KH_UNI_WORDS + KH_UNI_KMERS];
                        j = 0;
                        fresh = true;
                    }
                    if (fresh) {
                        fwd = 0;
                        for (uint32_t b = 0; b < k1; ++b) fwd = (fwd << 2) | kh_base_code(bases[start + j + b]);
                        fresh = false;
                    }
                    fwd = ((fwd << 2) | kh_base_code(bases[start + j + k1])) & km;
                    const u64 rc = kh_revcomp(fwd, k);
                    const uint32_t o = fwd > rc ? 1u : 0u;
                    key = o ? rc : fwd;
                    word[i] = kh_loc_word((uint32_t)u, o, (uint32_t)j);
                    ok |= 1u << i;
                    ++j;
                }
                ref[i] = prb.ref(key);
                first[i] = PRB::free_word();
                if (ok & (1u << i)) first[i] = PRB::load(ref[i]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!(ok & (1u << i))) continue;
                const u64 slot = prb.resolve_slot(ref[i], first[i]);
                if (slot < cap) {
                    where[slot] = word[i];
                    ++found;
                } else {
                    bad = 1;
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        found += __shfl_xor(found, d);
        bad |= __shfl_xor(bad, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (found) atomicAdd(reinterpret_cast<unsigned long long *>(hit), (unsigned long long)found);
        if (bad) *err = 1ull;
    }
}

// a tile's 4096 results in LDS, one pad word per 16: lane l writes word j of its 16 to 8-byte unit 17 l + j -- an odd stride, so the
// 32 lanes of a half wave spread over all banks -- and the store phase reads two neighbouring words per lane
constexpr int LC_LDS = TILE + TILE / 16;
__device__ __forceinline__ int lc_lds(int e) { return e + (e >> 4); }

// profile_kernel (profile.hip: the same tiles, the same windows, the same entry of out per lane and base) with the place instead
// of the count: per valid window resolve_slot, then one load of where[slot].  Of the eight windows of a half all first-slot loads
// are in flight before the first is looked at, then all where loads before the first is used.  The results are 8 bytes: a tile's
// 4096 go through 32 KiB of LDS and leave as 16-byte stores at 16-byte-aligned addresses, two words each, with single words only
// in front of the first aligned unit, behind the last, and at the two ends of out.
// The first half is not profile_kernel's text on purpose: the loads here are branch-free and the trip count is 32-bit, because this
// kernel has no scalar registers to spare for the masks of guarded loads.
// kernel-resource-usage (gfx950, hipcc -O3): see DESIGN.md 4.16.
template <bool QUAL, typename TAB>
__global__ __launch_bounds__(BLOCK) void locate_kernel(const uint8_t *__restrict__ abase, const uint8_t *__restrict__ qbase, int qaligned,
                                                       uint32_t vbeg32, u64 vend, u64 ntiles, uint32_t tiles_per_block, uint32_t k, uint32_t thr,
                                                       TAB table, const u64 *__restrict__ where, u64 *__restrict__ out, u64 nout) {
    __shared__ uint32_t s_code[2][BLOCK + 2];
    __shared__ uint16_t s_val[2][BLOCK + 2];
    __shared__ u64 s_out[LC_LDS];

    const int tid = threadIdx.x;
    const TAB tab = table;
    const u64 vbeg = vbeg32;            // (below 16: the bytes in front of the caller's first base in its 16-byte unit)
    const u64 tb = (u64)blockIdx.x * tiles_per_block;
    const uint32_t nt = tb >= ntiles ? 0u : (ntiles - tb < (u64)tiles_per_block ? (uint32_t)(ntiles - tb) : tiles_per_block);

    // (a 32-bit trip count: the scalar registers are what this kernel is short of)
    for (uint32_t it = 0; it < nt; ++it) {
        const u64 t = tb + it;
        const int buf = (int)(it & 1u);
        const WinCtx w = stage_tile<QUAL, BLOCK>(s_code, s_val, buf, it == 0u, tid, abase, qbase, qaligned, t, vbeg, vend, thr);
        Roller roll;
        roll.init(w, k, 0);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            u64 key[8];
            typename TAB::Ref ref[8];
            typename TAB::Word first[8];
            u64 place[8];
            uint32_t ok = 0, strands = 0;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                uint32_t s;
                ok |= (uint32_t)roll.next(half * 8 + jj, key[jj], s) << jj;
                strands |= s << jj;
            }
#pragma unroll
            // No branch around a load: a lane without a window probes key 0 (one line for all of them, and always inside the
            // table), and a k-mer that is not in the table reads where[0] -- the masks of sixteen guarded loads are scalar
            // registers this kernel does not have.
            for (int jj = 0; jj < 8; ++jj) {
                ref[jj] = tab.ref(key[jj] & (0ull - (u64)((ok >> jj) & 1u)));
                first[jj] = TAB::load(ref[jj]);
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const u64 slot = tab.resolve_slot(ref[jj], first[jj]);
                const u64 none = (u64)((int64_t)slot >> 63);  // all ones: not in the table (a slot index is far below 2^63)
                place[jj] = where[slot & ~none] | none;
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const u64 res = kh_loc_result(place[jj], (strands >> jj) & 1u) | ((u64)((ok >> jj) & 1u) - 1ull);  // (all ones: no window)
                s_out[lc_lds(tid * CHUNK + half * 8 + jj)] = res;
            }
        }
        __syncthreads();
        // (the next tile's results are written behind the barrier of its stage_tile: every lane is past these reads by then)
        const int64_t T0 = (int64_t)(t * (u64)TILE) - (int64_t)(k - 1) - (int64_t)vbeg;  // entry of out the tile's first result is
        // the tile's entries [e_lo, e_hi) lie inside out (32-bit and uniform: the tests below are one compare each)
        const int e_lo = T0 < 0 ? (-T0 < (int64_t)TILE ? (int)-T0 : TILE) : 0;
        const int e_hi = (int64_t)nout - T0 < (int64_t)TILE ? ((int64_t)nout - T0 > 0 ? (int)((int64_t)nout - T0) : 0) : TILE;
        u64 *const ot = reinterpret_cast<u64 *>((uintptr_t)out + (uintptr_t)(T0 * (int64_t)sizeof(u64)));  // (only ot[e], e_lo <= e < e_hi, is touched)
        const int sh = (int)(((uintptr_t)ot >> 3) & 1u);  // results in front of the first aligned unit
        if (tid < sh && e_lo == 0 && e_hi > 0) ot[0] = s_out[0];
#pragma unroll
        for (int r = 0; r < TILE / 2 / BLOCK; ++r) {
            const int e0 = sh + 2 * (tid + r * BLOCK);
            if (e0 >= e_lo && e0 + 1 < e_hi) {
                const u64 a = s_out[lc_lds(e0)], b = s_out[lc_lds(e0 + 1)];
                *reinterpret_cast<uint4 *>(ot + e0) = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
            } else {
                if (e0 >= e_lo && e0 < e_hi) ot[e0] = s_out[lc_lds(e0)];
                if (e0 + 1 >= e_lo && e0 + 1 < e_hi) ot[e0 + 1] = s_out[lc_lds(e0 + 1)];
            }
        }
    }
}

}  // namespace kh

namespace khi {

// The place map of the live unitigs, built if this is the first locate call since their begin.  On any failure nothing of it stays.
int locate_index(kh_ctx *c, const char *who) {
    if (c->un.where) return KH_OK;
    const std::string w(who);
    const u64 nu = c->un.n_unitigs, nb = c->un.n_bases, k1 = c->k - 1;
    if (nb < nu * k1 + nu) return fail(c, KH_ERR_STATE, (w + ": the unitigs' lengths do not add up (internal error)").c_str());
    const u64 nk = nb - nu * k1;
    u64 *d_where = nullptr;
    hipError_t e = dev_malloc((void **)&d_where, c->cap * sizeof(u64));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return soft_oom(c, (w + ": device memory for the place map").c_str(), e);  // (a reading call: the context stays usable, the unitigs live)
    }
    int rc = KH_OK;
    u64 words[2] = {0, 0};  // resolved k-mers, "one did not resolve"
    {
        CallScratch sc(c);
        // (never the idle partition buffers: the chunks of a kh_result_text_* stream may live there)
        u64 *const d_words = nu ? (u64 *)sc.fresh(2 * sizeof(u64)) : nullptr;
        auto run = [&]() -> int {
            if (nu && !d_words) return soft_oom(c, (w + ": device memory for the check words of the place map").c_str());
            HIP_TRY(c, hipMemsetAsync(d_where, 0xFF, c->cap * sizeof(u64), c->stream));
            if (nu) {
                HIP_TRY(c, hipMemsetAsync(d_words, 0, 2 * sizeof(u64), c->stream));
                with_probe(c, [&](auto prb) {
                    hipLaunchKernelGGL((kh::locate_index_kernel<decltype(prb)>), dim3(uni_grid((nk + kh::LI_RUN - 1) / kh::LI_RUN)), dim3(kh::BLOCK), 0,
                                       c->stream, (const u64 *)c->un.rows, (const uint8_t *)c->un.bases, nu, nk, c->k, prb, c->cap, d_where, d_words,
                                       d_words + 1);
                });
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
            }
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            return KH_OK;
        };
        rc = run();
        if (rc != KH_OK) (void)hipStreamSynchronize(c->stream);  // (before the scratch and the map go back)
    }
    if (rc == KH_OK && nu && (words[1] || words[0] != nk))
        rc = fail(c, KH_ERR_STATE, (w + ": a k-mer of the unitigs is not in the table (internal error)").c_str());
    if (rc != KH_OK) {
        (void)dev_free(d_where);
        return rc;
    }
    c->un.where = d_where;
    return KH_OK;
}

// Every window start i < nout of the n device-resident bytes -> d_out[i]; asynchronous on the compute stream.  The launch is
// profile_range's: read_plan().
int locate_range(kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, u64 n, u64 nout, u64 *d_out) {
    if (nout == 0) return KH_OK;
    const ReadPlan p = read_plan(c, d_bases, d_qual, n, nout);
    const dim3 grid(p.blocks), block(kh::BLOCK);
    with_probe(c, [&](auto tab) {
        typedef decltype(tab) TAB;
        if (p.qbase)
            hipLaunchKernelGGL((kh::locate_kernel<true, TAB>), grid, block, 0, c->stream, p.abase, p.qbase, p.qaligned, (uint32_t)p.vbeg, p.vend, p.ntiles,
                               p.tpb, c->k, p.thr, tab, (const u64 *)c->un.where, d_out, nout);
        else
            hipLaunchKernelGGL((kh::locate_kernel<false, TAB>), grid, block, 0, c->stream, p.abase, p.qbase, p.qaligned, (uint32_t)p.vbeg, p.vend, p.ntiles,
                               p.tpb, c->k, p.thr, tab, (const u64 *)c->un.where, d_out, nout);
    });
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}

int enter_unitigs(kh_ctx *c, const char *who) {
    const int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (!c->un.live)
        return fail(c, KH_ERR_STATE,
                    (std::string(who) + ": no unitigs: kh_unitigs_begin first (anything that changes the table makes them stale)").c_str());
    return KH_OK;
}

namespace {

// What both calls do before they touch anything: arguments, entry, live unitigs.
int locate_enter(kh_ctx *c, const char *who, const void *bases, uint64_t n, const void *out) {
    if (!c) return KH_ERR_BAD_ARG;
    const std::string w(who);
    if (n && (!bases || !out)) return fail(c, KH_ERR_BAD_ARG, (w + ": NULL argument").c_str());
    if ((uintptr_t)out & 7) return fail(c, KH_ERR_BAD_ARG, (w + ": the output is not 8-byte aligned").c_str());
    return enter_unitigs(c, who);
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_unitigs_locate_device(kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, uint64_t *d_out) {
    int rc = locate_enter(c, "kh_unitigs_locate_device", d_bases, n, d_out);
    if (rc != KH_OK) return rc;
    if (n == 0) return KH_OK;
    if ((rc = locate_index(c, "kh_unitigs_locate_device")) != KH_OK) return rc;
    if ((rc = locate_range(c, d_bases, d_qual, n, n, reinterpret_cast<u64 *>(d_out))) != KH_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (d_out is complete, and the caller's buffers may go)
    return KH_OK;
}

extern "C" int kh_unitigs_locate(kh_ctx *c, const uint8_t *bases, const uint8_t *qual, uint64_t n, uint64_t *out) {
    int rc = locate_enter(c, "kh_unitigs_locate", bases, n, out);
    if (rc != KH_OK) return rc;
    if (n == 0) return KH_OK;
    const u64 chunk = profile_chunk(c, n);
    // (the staging first: whichever allocation fails, nothing of the place map stays behind)
    if ((rc = profile_buffers(c, chunk, sizeof(u64), "kh_unitigs_locate: chunk buffers")) != KH_OK) return rc;
    if ((rc = locate_index(c, "kh_unitigs_locate")) != KH_OK) return rc;
    // kh_profile's pipeline with 8 bytes per window start
    return chunk_pipeline(c, bases, qual, n, chunk, 0, out, sizeof(u64), [&](const ChunkJob &job) {
        return locate_range(c, job.d_bases, job.d_qual, job.len, job.ns, reinterpret_cast<u64 *>(job.d_tail));
    });
}
