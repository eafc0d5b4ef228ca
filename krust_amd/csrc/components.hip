// components.hip -- kh_unitigs_components / kh_unitigs_components_device: the connected components of the live unitigs' link graph
// (include/kmerhip.h, "CONNECTED COMPONENTS"), and the labelling and decide launches of kh_drop_components_into (unitig.hip's
// clip_step()).  No reference counterpart.  The link array holds every link with its mirror: it is an undirected edge list.
//   comp_init_kernel       parent[u] = u
//   comp_hook_kernel       per link word with from unitig < to unitig: the greater of the two ends' labels is lowered to the smaller
//   comp_compress_kernel   per unitig: parent chased to its root, the root stored
//                          -- one launch pair and one flag read-back per round, until a hook round lowers nothing
//   comp_sum_kernel        UNITIGS, KMERS, COUNT_SUM per root: the lanes of a wave that share a label add up first, one lane adds
//   comp_root_kernel       flags the roots; device_scan turns the flags into dense ids
//   comp_write_kernel      comp[u] = rank[parent[u]], a root writes its row; SINGLETONS and LARGEST_KMERS by wave reductions
//   comp_drop_kernel       kh_drop_components_into: removed[u] = (KMERS of u's component < min_kmers), seven of the nine words
// No kernel waits for another workgroup, and no device loop is without a bound.
#include "ctx.hip.h"

namespace kh {

using khi::KH_CSUM_WORDS;

// THE INVARIANT of parent[] through all rounds, which makes stale and concurrent reads harmless: parent[x] <= x always; a value
// is only ever lowered (atomicMin in the hook, a root that lies below in the compress); and every value stored in parent[x] is a
// unitig that really is connected to x.  So following parent from any x descends strictly until it stops at some r with
// parent[r] == r, whatever mixture of old and new values the loads return, and r is in x's component.

// kernel-resource-usage (gfx950, hipcc -O3): 4 VGPRs, 16 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void comp_init_kernel(uint32_t *parent, u64 nu) {
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < nu; u += (u64)gridDim.x * BLOCK) parent[u] = (uint32_t)u;
}

// One lane per link word a -> b with a < b (the mirror word covers b -> a, a self link joins nothing).  ra and rb are roots as the
// last compress left them, or values another lane of this launch has lowered since: either way connected to a and b and <= them.
// Where they differ the greater one's parent is lowered to the smaller: atomicMin, so of several lanes that hook the same unitig
// the smallest wins and the others' links find differing labels again in the next round.  *changed is raised when a value fell.
// A round that raises nothing has seen equal roots at both ends of every link.
// kernel-resource-usage (gfx950, hipcc -O3): 12 VGPRs, 42 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void comp_hook_kernel(const u64 *__restrict__ links, u64 nl, u64 nu, uint32_t *parent, uint32_t *changed) {
    bool any = false;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nl; i += (u64)gridDim.x * BLOCK) {
        const u64 w = links[i];
        const uint32_t a = KH_UNI_LINK_FROM(w), b = KH_UNI_LINK_TO(w);
        if (a >= b || b >= nu) continue;
        const uint32_t ra = parent[a], rb = parent[b];
        if (ra == rb) continue;
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        if (hi < nu && atomicMin(&parent[hi], lo) > lo) any = true;  // (hi < nu: always, by the invariant)
    }
    if (kh_any(any) && lane_id() == 0) *changed = 1u;  // (every writer writes the same word)
}

// One lane per unitig: parent chased to a root, the root stored.  Stores of this launch only replace a value by a root below
// it, and no root's own entry is written, so the chase ends at the same root whichever stores it has seen; it descends strictly,
// so nu steps bound it.
// kernel-resource-usage (gfx950, hipcc -O3): 13 VGPRs, 24 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void comp_compress_kernel(uint32_t *parent, u64 nu) {
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < nu; u += (u64)gridDim.x * BLOCK) {
        const uint32_t p0 = parent[u];
        uint32_t r = p0;
        for (u64 step = 0; step < nu && r < nu; ++step) {
            const uint32_t p = parent[r];
            if (p >= r) break;  // (p == r: a root)
            r = p;
        }
        if (r != p0) parent[u] = r;
    }
}

// sums[KH_CSUM_WORDS * r ..] += (1, KMERS, COUNT_SUM) of every unitig whose label is r.  On real data one component holds nearly
// every unitig: one atomic per unitig on its three words would serialise.  So a wave takes the label of its first lane that is
// still to do, ballots the lanes that share it and retires them: a lane alone with its label adds its own row (the lone path),
// otherwise the wave reduces the members' values and its lane 0 adds the sums (the aggregated path).  At most 64 passes, one per
// distinct label in the wave; the loop is uniform, so every lane takes part in the reductions.  Integer sums: order-free.
// kernel-resource-usage (gfx950, hipcc -O3): 31 VGPRs, 40 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void comp_sum_kernel(const uint32_t *__restrict__ parent, const u64 *__restrict__ rows, u64 nu, u64 *__restrict__ sums) {
    const uint32_t lane = lane_id();
    for (u64 base = (u64)blockIdx.x * BLOCK; base < nu; base += (u64)gridDim.x * BLOCK) {  // (uniform: every lane shuffles)
        const u64 u = base + threadIdx.x;
        const bool in = u < nu;
        uint32_t lab = in ? parent[u] : 0xFFFFFFFFu;
        if (in && lab >= nu) lab = (uint32_t)u;  // (never)
        const u64 km = in ? rows[KH_UNI_WORDS * u + KH_UNI_KMERS] : 0, cs = in ? rows[KH_UNI_WORDS * u + KH_UNI_COUNT_SUM] : 0;
        u64 todo = kh_ballot(in);
        for (int pass = 0; pass < 64 && todo; ++pass) {
            const int first = __builtin_ctzll(todo);
            const uint32_t l0 = (uint32_t)__shfl((int)lab, first, 64);
            const bool mine = in && lab == l0;  // (a retired lane's label was an earlier l0: it matches no later one)
            const u64 m = kh_ballot(mine);
            u64 *const row = sums + KH_CSUM_WORDS * (u64)l0;
            if ((m & (m - 1)) == 0) {  // the lone path
                if (mine) {
                    atomicAdd(&row[0], 1ull);
                    atomicAdd(&row[1], km);
                    if (cs) atomicAdd(&row[2], cs);
                }
            } else {  // the aggregated path
                const u64 skm = wave_sum(mine ? km : 0), scs = wave_sum(mine ? cs : 0);
                if (lane == 0) {
                    atomicAdd(&row[0], (u64)__builtin_popcountll(m));
                    atomicAdd(&row[1], skm);
                    if (scs) atomicAdd(&row[2], scs);
                }
            }
            todo &= ~m;
        }
    }
}

// kernel-resource-usage (gfx950, hipcc -O3): 7 VGPRs, 18 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void comp_root_kernel(const uint32_t *__restrict__ parent, u64 nu, uint32_t *__restrict__ isroot) {
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < nu; u += (u64)gridDim.x * BLOCK) isroot[u] = parent[u] == (uint32_t)u ? 1u : 0u;
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;  // valid in lane 0
}

// rank: the exclusive scan of the root flags, rank[nu] == nc.  comp[u] = rank[parent[u]]; a root writes its row at its rank.
// words: SINGLETONS added, LARGEST_KMERS by atomicMax -- per-lane values, one reduction per wave and word.
// kernel-resource-usage (gfx950, hipcc -O3): 28 VGPRs, 44 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void comp_write_kernel(const uint32_t *__restrict__ parent, const u64 *__restrict__ rank, const u64 *__restrict__ sums,
                                                           u64 nu, u64 nc, uint32_t *__restrict__ comp, u64 *__restrict__ crow, u64 *__restrict__ words,
                                                           uint32_t *__restrict__ err) {
    u64 single = 0, largest = 0;
    bool bad = false;
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < nu; u += (u64)gridDim.x * BLOCK) {
        const uint32_t r = parent[u];
        const u64 id = r < nu ? rank[r] : nc;
        if (id >= nc) {
            bad = true;
            comp[u] = 0;
            continue;
        }
        comp[u] = (uint32_t)id;
        if (r == (uint32_t)u) {
            const u64 cu = sums[KH_CSUM_WORDS * u], km = sums[KH_CSUM_WORDS * u + 1];
            crow[KH_COMP_WORDS * id + KH_COMP_FIRST] = u;
            crow[KH_COMP_WORDS * id + KH_COMP_UNITIGS] = cu;
            crow[KH_COMP_WORDS * id + KH_COMP_KMERS] = km;
            crow[KH_COMP_WORDS * id + KH_COMP_COUNT_SUM] = sums[KH_CSUM_WORDS * u + 2];
            single += cu == 1;
            largest = km > largest ? km : largest;
        }
    }
    if (kh_any(bad) && lane_id() == 0) *err = 1u;
    single = wave_sum(single);
    largest = wave_max(largest);
    if (lane_id() == 0) {
        if (single) atomicAdd(&words[KH_CC_SINGLETONS], single);
        if (largest) atomicMax(&words[KH_CC_LARGEST_KMERS], largest);
    }
}

// kh_drop_components_into: removed[u] = (KMERS of u's component < min_kmers).  UNITIGS and LINKS as the other two rules count them
// (clip_step() holds them against what was built); COMPONENTS, DROPPED, DROPPED_KMERS and DROPPED_COUNT by the roots,
// DROPPED_UNITIGS by every unitig -- per-lane sums, one reduction per wave and word, one atomic by its lane 0.
// kernel-resource-usage (gfx950, hipcc -O3): 46 VGPRs, 34 SGPRs, no LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void comp_drop_kernel(u64 nu, const uint32_t *__restrict__ parent, const u64 *__restrict__ sums,
                                                          const u64 *__restrict__ loff, u64 min_kmers, uint8_t *__restrict__ removed,
                                                          u64 *__restrict__ words) {
    u64 s_uni = 0, s_links = 0, s_comp = 0, s_drop = 0, s_kmers = 0, s_count = 0, s_du = 0;
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < nu; u += (u64)gridDim.x * BLOCK) {
        uint32_t r = parent[u];
        if (r >= nu) r = (uint32_t)u;  // (never)
        const u64 km = sums[KH_CSUM_WORDS * (u64)r + 1];
        const bool rem = km < min_kmers;
        removed[u] = rem ? 1 : 0;
        s_uni += 1;
        s_links += loff[2 * u + 2] - loff[2 * u];
        s_du += rem;
        if (r == (uint32_t)u) {
            s_comp += 1;
            if (rem) {
                s_drop += 1;
                s_kmers += km;
                s_count += sums[KH_CSUM_WORDS * (u64)r + 2];
            }
        }
    }
    s_uni = wave_sum(s_uni);
    s_links = wave_sum(s_links);
    s_comp = wave_sum(s_comp);
    s_drop = wave_sum(s_drop);
    s_kmers = wave_sum(s_kmers);
    s_count = wave_sum(s_count);
    s_du = wave_sum(s_du);
    if (lane_id() == 0) {
        if (s_uni) atomicAdd(&words[KH_DROP_UNITIGS], s_uni);
        if (s_links) atomicAdd(&words[KH_DROP_LINKS], s_links);
        if (s_comp) atomicAdd(&words[KH_DROP_COMPONENTS], s_comp);
        if (s_drop) atomicAdd(&words[KH_DROP_DROPPED], s_drop);
        if (s_kmers) atomicAdd(&words[KH_DROP_DROPPED_KMERS], s_kmers);
        if (s_count) atomicAdd(&words[KH_DROP_DROPPED_COUNT], s_count);
        if (s_du) atomicAdd(&words[KH_DROP_DROPPED_UNITIGS], s_du);
    }
}

}  // namespace kh

namespace khi {

// Rounds repeat until a hook round changes nothing: every changing round lowers a label, so they end; the compress in between is
// what keeps their number near log2 of the unitigs and not at the graph's diameter.  No links: no hook launch, 0 rounds.
int components_label(kh_ctx *c, uint32_t *parent, u64 *sums, uint32_t *d_flag, u64 *rounds, const std::function<void()> &before_sums) {
    const u64 nu = c->un.n_unitigs, nl = c->un.n_links;
    *rounds = 0;
    hipLaunchKernelGGL(kh::comp_init_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, parent, nu);
    HIP_TRY(c, hipGetLastError());
    bool open = nl != 0;
    for (u64 r = 0; open && r <= nu; ++r) {  // (a changing round lowers a label: fewer than nu of them)
        HIP_TRY(c, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(kh::comp_hook_kernel, dim3(uni_grid(nl)), dim3(kh::BLOCK), 0, c->stream, (const u64 *)c->un.links, nl, nu, parent, d_flag);
        hipLaunchKernelGGL(kh::comp_compress_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, parent, nu);
        HIP_TRY(c, hipGetLastError());
        uint32_t changed = 0;
        HIP_TRY(c, hipMemcpyAsync(&changed, d_flag, sizeof(changed), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        *rounds += 1;
        open = changed != 0;
    }
    if (open) return fail(c, KH_ERR_STATE, "kh_unitigs_components: the labels still fall after as many rounds as there are unitigs (internal error)");
    if (before_sums) before_sums();
    HIP_TRY(c, hipMemsetAsync(sums, 0, nu * KH_CSUM_WORDS * sizeof(u64), c->stream));
    hipLaunchKernelGGL(kh::comp_sum_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, (const uint32_t *)parent, (const u64 *)c->un.rows, nu, sums);
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}

int components_drop_launch(kh_ctx *c, const uint32_t *parent, const u64 *sums, const u64 *loff, u64 min_kmers, uint8_t *removed, u64 *words) {
    hipLaunchKernelGGL(kh::comp_drop_kernel, dim3(uni_grid(c->un.n_unitigs)), dim3(kh::BLOCK), 0, c->stream, c->un.n_unitigs, parent, sums, loff, min_kmers,
                       removed, words);
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}

namespace {

inline u64 up16(u64 x) { return (x + 15) & ~15ull; }

// KH_FLAG_TRACE: the device time of the build's three parts -- events on the compute stream, printed once it has run dry
// (tools/unitig_probe.py --components reads the line).  Without the flag nothing is recorded.
struct ComponentTimes {
    bool on;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // in front of the rounds, of the sums, of the ids, behind them
    explicit ComponentTimes(const kh_ctx *c) : on(c->trace) {}
    void mark(kh_ctx *c, int i) {
        if (on && hipEventCreate(&ev[i]) == hipSuccess) (void)hipEventRecord(ev[i], c->stream);
    }
    void report(const char *who, u64 rounds) {  // (the stream is drained)
        if (!on) return;
        float ms[3] = {0, 0, 0}, t = 0;
        for (int s = 0; s < 3; ++s)
            if (ev[s] && ev[s + 1] && hipEventElapsedTime(&t, ev[s], ev[s + 1]) == hipSuccess) ms[s] = t;
        fprintf(stderr, "[kmerhip] %s: rounds %llu, hook and compress %.3f ms, sums %.3f ms, ids and rows %.3f ms\n", who, (unsigned long long)rounds, ms[0],
                ms[1], ms[2]);
    }
    ~ComponentTimes() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// The labels of the live unitigs (Unitigs::comp, comp_rows, cc), built if no call has built them since their begin.  The scratch
// is one allocation of the call's own -- never the idle partition buffers: the chunks of a kh_result_text_* stream may live
// there --, the cache one more, made once the number of components is known.  On any failure nothing of either stays and the
// status is a reading call's.
int components_build(kh_ctx *c, const char *who) {
    if (c->un.comp_built) return KH_OK;
    const u64 nu = c->un.n_unitigs;
    if (nu == 0) {
        c->un.comp_built = true;
        return KH_OK;
    }
    const u64 b_par = up16(nu * sizeof(uint32_t)), b_sums = up16(nu * KH_CSUM_WORDS * sizeof(u64)), b_rank = up16((nu + 1) * sizeof(u64));
    const u64 b_scan = up16(device_scan_scratch(nu)), b_words = up16(KH_CC_WORDS * sizeof(u64));
    CallScratch sc(c);
    uint8_t *const mem = (uint8_t *)sc.fresh(2 * b_par + b_sums + b_rank + b_scan + b_words + 16);
    if (!mem) return soft_oom(c, (std::string(who) + ": device memory for the labelling's scratch").c_str());
    uint32_t *const parent = (uint32_t *)mem, *const isroot = (uint32_t *)(mem + b_par);
    u64 *const sums = (u64 *)(mem + 2 * b_par), *const rank = (u64 *)(mem + 2 * b_par + b_sums);
    u64 *const scan = (u64 *)(mem + 2 * b_par + b_sums + b_rank), *const words = (u64 *)(mem + 2 * b_par + b_sums + b_rank + b_scan);
    uint32_t *const d_flag = (uint32_t *)(words + KH_CC_WORDS);  // ("something changed", "something is inconsistent": the 16 bytes at the end)
    u64 *d_cache = nullptr;
    auto run = [&]() -> int {
        ComponentTimes times(c);
        u64 rounds = 0, nc = 0;
        HIP_TRY(c, hipMemsetAsync(words, 0, b_words + 16, c->stream));
        times.mark(c, 0);
        int rc = components_label(c, parent, sums, d_flag, &rounds, [&]() { times.mark(c, 1); });
        if (rc != KH_OK) return rc;
        times.mark(c, 2);
        hipLaunchKernelGGL(kh::comp_root_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, (const uint32_t *)parent, nu, isroot);
        HIP_TRY(c, hipGetLastError());
        if ((rc = device_scan(c, isroot, nu, rank, true, scan)) != KH_OK) return rc;
        HIP_TRY(c, hipMemcpyAsync(&nc, rank + nu, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (nc == 0 || nc > nu) return fail(c, KH_ERR_STATE, (std::string(who) + ": the roots do not add up (internal error)").c_str());
        const hipError_t e = dev_malloc((void **)&d_cache, nc * KH_COMP_WORDS * sizeof(u64) + nu * sizeof(uint32_t));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            d_cache = nullptr;
            return soft_oom(c, (std::string(who) + ": device memory for the labels").c_str(), e);
        }
        uint32_t *const comp = (uint32_t *)(d_cache + nc * KH_COMP_WORDS);
        hipLaunchKernelGGL(kh::comp_write_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, (const uint32_t *)parent, (const u64 *)rank,
                           (const u64 *)sums, nu, nc, comp, d_cache, words, d_flag + 1);
        HIP_TRY(c, hipGetLastError());
        times.mark(c, 3);
        u64 h[KH_CC_WORDS] = {0, 0, 0, 0};
        uint32_t bad = 0;
        HIP_TRY(c, hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&bad, d_flag + 1, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, KH_ERR_STATE, (std::string(who) + ": a label is no root (internal error)").c_str());
        h[KH_CC_COMPONENTS] = nc;
        h[KH_CC_ROUNDS] = rounds;
        memcpy(c->un.cc, h, sizeof(h));
        c->un.comp_rows = d_cache;
        c->un.comp = comp;
        c->un.n_comp = nc;
        c->un.comp_built = true;
        times.report(who, rounds);
        return KH_OK;
    };
    const int rc = run();
    if (rc != KH_OK) {
        (void)hipStreamSynchronize(c->stream);  // (before the scratch goes back)
        if (d_cache) (void)dev_free(d_cache);
    }
    return rc;
}

// What both calls do before they copy: arguments, entry, live unitigs with links, the labels, out, the caps.  *done: nothing to copy.
// host: the host form -- where it is about to build the labels, the pinned staging of the way back comes first, sized for the most
// it may carry: whichever allocation fails, nothing of the labels stays behind (the staging is the context's, as after a copy).
int components_enter(kh_ctx *c, const char *who, const void *comp, u64 comp_cap, const void *rows, u64 row_cap, uint64_t *out, bool *done, bool host) {
    *done = true;
    if (!c) return KH_ERR_BAD_ARG;
    const std::string w(who);
    if (!out || (comp_cap && !comp) || (row_cap && !rows)) return fail(c, KH_ERR_BAD_ARG, (w + ": NULL argument").c_str());
    if ((uintptr_t)comp & 3) return fail(c, KH_ERR_BAD_ARG, (w + ": comp is not 4-byte aligned").c_str());
    if (((uintptr_t)rows | (uintptr_t)out) & 7) return fail(c, KH_ERR_BAD_ARG, (w + ": rows or out is not 8-byte aligned").c_str());
    int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (!c->un.live)
        return fail(c, KH_ERR_STATE, (w + ": no unitigs: kh_unitigs_begin_linked first (anything that changes the table makes them stale)").c_str());
    if (!c->un.linked) return fail(c, KH_ERR_STATE, (w + ": no links were built: kh_unitigs_begin_linked, not kh_unitigs_begin").c_str());
    if (host && !c->un.comp_built && c->un.n_unitigs) {
        const u64 nu = c->un.n_unitigs;
        u64 need = 0;
        if (comp_cap && !is_pinned_host(comp)) need = nu * sizeof(uint32_t);
        if (row_cap && !is_pinned_host(rows)) need = nu * KH_COMP_WORDS * sizeof(u64);  // (at most one row per unitig)
        if (need && (rc = ensure_stage(c, (need + 1) / 2, true)) != KH_OK) return rc;
    }
    if ((rc = components_build(c, who)) != KH_OK) return rc;
    memcpy(out, c->un.cc, KH_CC_WORDS * sizeof(u64));
    if (comp_cap && comp_cap < c->un.n_unitigs) return fail(c, KH_ERR_RANGE, (w + ": comp array too small").c_str());
    if (row_cap && row_cap < c->un.n_comp) return fail(c, KH_ERR_RANGE, (w + ": row array too small").c_str());
    *done = c->un.n_unitigs == 0;
    return KH_OK;
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_unitigs_components_device(kh_ctx *c, uint32_t *d_comp, uint64_t comp_cap, uint64_t *d_rows, uint64_t row_cap, uint64_t *out) {
    bool done = false;
    const int rc = components_enter(c, "kh_unitigs_components_device", d_comp, comp_cap, d_rows, row_cap, out, &done, false);
    if (rc != KH_OK || done) return rc;
    if (comp_cap) HIP_TRY(c, hipMemcpyAsync(d_comp, c->un.comp, c->un.n_unitigs * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    if (row_cap) HIP_TRY(c, hipMemcpyAsync(d_rows, c->un.comp_rows, c->un.n_comp * KH_COMP_WORDS * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return KH_OK;
}

extern "C" int kh_unitigs_components(kh_ctx *c, uint32_t *comp, uint64_t comp_cap, uint64_t *rows, uint64_t row_cap, uint64_t *out) {
    bool done = false;
    int rc = components_enter(c, "kh_unitigs_components", comp, comp_cap, rows, row_cap, out, &done, true);
    if (rc != KH_OK || done) return rc;
    if (comp_cap) rc = d2h_staged(c, comp, c->un.comp, c->un.n_unitigs * sizeof(uint32_t));
    if (rc == KH_OK && row_cap) rc = d2h_staged(c, rows, c->un.comp_rows, c->un.n_comp * KH_COMP_WORDS * sizeof(u64));
    return rc;
}
