// support.hip -- kh_unitigs_link_support / kh_unitigs_link_support_device: how many reads walk every link of the live unitigs
// (include/kmerhip.h, "READ SUPPORT PER LINK").  No reference counterpart.  The rows of kh_unitigs_paths* never leave the device:
//   link_index_kernel     once per kh_unitigs_begin_linked, by the first call that asks: per end state the index of its first link
//   link_support_kernel   per tile of SUP_TILE rows: which rows are followed by a row of the same record (the record boundaries as an
//                         LDS bitmap), which of those pairs are crossings, the crossing's word looked up among the at most four links
//                         of its first state, one atomic per hit
// The work is per row, never per record or per window: one record that holds every run spreads over the whole grid.
#include "ctx.hip.h"
#include "support_bits.h"

namespace kh {

constexpr int SUP_PER = 4;                  // rows per lane and tile
constexpr int SUP_TILE = BLOCK * SUP_PER;   // 1024 rows per workgroup iteration (tests/test_gpu_link_support.py states it)
constexpr int SUP_RB = SUP_TILE / 32 + 1;   // record boundaries at the tile's rows 0 .. SUP_TILE, one bit each

// The link array is sorted and a state has at most four links out: one lane per link stores its own index where its high half
// differs from the word in front.  index: all ones before the launch; plain stores, every entry has one writer.
__global__ __launch_bounds__(BLOCK) void link_index_kernel(const u64 *__restrict__ links, u64 nl, u64 *__restrict__ index, u64 states) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nl; i += (u64)gridDim.x * BLOCK) {
        const u64 hi = links[i] >> 32;
        if ((i == 0 || (links[i - 1] >> 32) != hi) && hi < states) index[hi] = i;
    }
}

// Per tile: STATE and QSTART of its rows and of the one behind it go to LDS (one 16-byte load per row where runs is 16-byte
// aligned), STATE and QEND stay in the lane; the boundaries run_start[r] that fall on the tile's rows 0 .. SUP_TILE are marked in an
// LDS bitmap as path_flags_kernel marks rec_start (a 256-ary search for the first, then 256 per round: several boundaries on one
// row and empty records set the same bit).  Row i pairs with i + 1 unless i lies in front of run_start[0], i + 1 at or behind
// run_start[nrec] or n_runs, or a boundary lies at i + 1.  A pair with QEND == QSTART is a crossing: one load of index[STATE_i],
// then the up to four link words from there (two 16-byte loads where they are aligned and inside the array), compared with the
// crossing's word; a hit is one 64-bit atomic without a return value.  words: PAIRS, ADJACENT, CREDITED -- per-lane sums, one
// reduction per wave and word, one atomic by its lane 0 (clip_decide_kernel's pattern).
// Offsets outside the contract mark other bits, never one outside the bitmap; a STATE that is no state loads nothing; every link
// index is below nl.
// kernel-resource-usage (gfx950, hipcc -O3): see DESIGN.md 4.18.
__global__ __launch_bounds__(BLOCK) void link_support_kernel(const u64 *__restrict__ run_start, u64 nrec, const uint32_t *__restrict__ runs,
                                                             u64 n_runs, const u64 *__restrict__ links, u64 nl,
                                                             const u64 *__restrict__ index, u64 states, u64 *__restrict__ support,
                                                             u64 *__restrict__ words) {
    __shared__ uint32_t s_state[SUP_TILE + 1];
    __shared__ uint32_t s_qs[SUP_TILE + 1];
    __shared__ uint32_t s_rb[SUP_RB];

    const int tid = threadIdx.x;
    const bool vec = (((uintptr_t)runs) & 15) == 0;
    const u64 R0 = run_start[0];  // the records own the rows [R0, RN)
    const u64 RN = run_start[nrec] < n_runs ? run_start[nrec] : n_runs;
    const u64 nt = (n_runs + SUP_TILE - 1) / SUP_TILE;
    u64 c_pairs = 0, c_adj = 0, c_cred = 0;
    for (u64 t = blockIdx.x; t < nt; t += gridDim.x) {
        const u64 r0 = t * (u64)SUP_TILE;  // the tile's row 0
        uint32_t st[SUP_PER], qe[SUP_PER];
#pragma unroll
        for (int r = 0; r < SUP_PER; ++r) {
            const int e = tid + r * BLOCK;
            const u64 i = r0 + (u64)e;
            uint32_t s = 0xFFFFFFFFu, q0 = 0, q1 = 0;
            if (i < n_runs) {
                const uint32_t *const row = runs + i * KH_RUN_WORDS;
                if (vec) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(row);
                    s = v.x, q0 = v.z, q1 = v.w;
                } else {
                    s = row[KH_RUN_STATE], q0 = row[KH_RUN_QSTART], q1 = row[KH_RUN_QEND];
                }
            }
            st[r] = s;
            qe[r] = q1;
            s_state[e] = s;
            s_qs[e] = q0;
        }
        if (tid == 0) {  // the row behind the tile
            const u64 i = r0 + (u64)SUP_TILE;
            const bool in = i < n_runs;
            s_state[SUP_TILE] = in ? runs[i * KH_RUN_WORDS + KH_RUN_STATE] : 0xFFFFFFFFu;
            s_qs[SUP_TILE] = in ? runs[i * KH_RUN_WORDS + KH_RUN_QSTART] : 0u;
        }
        for (int i = tid; i < SUP_RB; i += BLOCK) s_rb[i] = 0u;
        __syncthreads();

        u64 b0 = wg_first_not(0, nrec + 1, tid, [&](u64 i) { return run_start[i] < r0; });
        for (;;) {  // (uniform: the count below is every lane's)
            const u64 idx = b0 + (u64)tid;
            bool go = false;
            if (idx <= nrec) {
                const u64 v = run_start[idx];
                go = v <= r0 + SUP_TILE;
                if (v >= r0 && go) atomicOr(&s_rb[(uint32_t)(v - r0) >> 5], 1u << ((uint32_t)(v - r0) & 31u));
            }
            if (__syncthreads_count(go) < BLOCK) break;
            b0 += BLOCK;
        }

#pragma unroll
        for (int r = 0; r < SUP_PER; ++r) {
            const int e = tid + r * BLOCK;
            const u64 i = r0 + (u64)e;
            const uint32_t nb = (uint32_t)(e + 1);  // the tile's row of i + 1
            const bool pair = i >= R0 && i + 1 < RN && !((s_rb[nb >> 5] >> (nb & 31u)) & 1u);
            const bool adj = pair && kh_sup_adjacent(qe[r], s_qs[nb]);
            c_pairs += pair;
            c_adj += adj;
            if (adj && (u64)st[r] < states) {
                const u64 w = kh_sup_word(st[r], s_state[nb]);
                const u64 first = index[st[r]];
                if (first < nl) {
                    u64 l[4] = {~0ull, ~0ull, ~0ull, ~0ull};  // (no crossing's word: its high half is a state)
                    if (!(first & 1ull) && first + 4 <= nl) {
                        const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(links + first);
                        const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(links + first + 2);
                        l[0] = a.x, l[1] = a.y, l[2] = b.x, l[3] = b.y;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (first + j < nl) l[j] = links[first + j];
                    }
                    // (the words behind the state's last link have another high half: they match no crossing of this state)
                    const int hit = l[0] == w ? 0 : l[1] == w ? 1 : l[2] == w ? 2 : l[3] == w ? 3 : -1;
                    if (hit >= 0) {
                        atomicAdd(reinterpret_cast<unsigned long long *>(support + first + hit), 1ull);
                        c_cred += 1;
                    }
                }
            }
        }
        __syncthreads();  // (the LDS is free for the next tile)
    }
    c_pairs = wave_sum(c_pairs);
    c_adj = wave_sum(c_adj);
    c_cred = wave_sum(c_cred);
    if (lane_id() == 0) {
        if (c_pairs) atomicAdd(reinterpret_cast<unsigned long long *>(&words[KH_SUP_PAIRS]), c_pairs);
        if (c_adj) atomicAdd(reinterpret_cast<unsigned long long *>(&words[KH_SUP_ADJACENT]), c_adj);
        if (c_cred) atomicAdd(reinterpret_cast<unsigned long long *>(&words[KH_SUP_CREDITED]), c_cred);
    }
}

}  // namespace kh

namespace khi {
namespace {

inline u64 up16(u64 x) { return (x + 15) & ~15ull; }

// KH_FLAG_TRACE: the device time of the index build and of the kernel -- events on the compute stream, printed once it has run dry
// (tools/unitig_probe.py --support reads the line).  Without the flag nothing is recorded.
struct SupportTimes {
    bool on;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // round the index build, round the kernel
    explicit SupportTimes(const kh_ctx *c) : on(c->trace) {}
    void mark(kh_ctx *c, int i) {
        if (on && hipEventCreate(&ev[i]) == hipSuccess) (void)hipEventRecord(ev[i], c->stream);
    }
    void report(const char *who) {  // (the stream is drained)
        if (!on) return;
        float ms[2] = {0, 0}, t = 0;
        for (int s = 0; s < 2; ++s)
            if (ev[2 * s] && ev[2 * s + 1] && hipEventElapsedTime(&t, ev[2 * s], ev[2 * s + 1]) == hipSuccess) ms[s] = t;
        fprintf(stderr, "[kmerhip] %s: index %.3f ms, support %.3f ms\n", who, ms[0], ms[1]);
    }
    ~SupportTimes() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// The link index of the live unitigs (Unitigs::link_first), built if no call has built it since their begin: 2 * n_unitigs entries
// and, behind them, the KH_SUP_WORDS words the kernel adds up -- one allocation, so that a later device-form call makes none.  On
// any failure nothing of it stays and the status is a reading call's.
int support_index(kh_ctx *c, const char *who, SupportTimes &times) {
    if (c->un.link_first) return KH_OK;
    const u64 states = 2 * c->un.n_unitigs, nl = c->un.n_links;
    u64 *d_index = nullptr;
    hipError_t e = dev_malloc((void **)&d_index, (states + KH_SUP_WORDS) * sizeof(u64));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return soft_oom(c, (std::string(who) + ": device memory for the link index").c_str(), e);
    }
    auto run = [&]() -> int {
        times.mark(c, 0);
        if (states) HIP_TRY(c, hipMemsetAsync(d_index, 0xFF, states * sizeof(u64), c->stream));
        if (nl) {
            hipLaunchKernelGGL(kh::link_index_kernel, dim3((unsigned)grid_for(nl)), dim3(kh::BLOCK), 0, c->stream, (const u64 *)c->un.links, nl, d_index,
                               states);
            HIP_TRY(c, hipGetLastError());
        }
        times.mark(c, 1);
        return KH_OK;
    };
    const int rc = run();
    if (rc != KH_OK) {
        (void)hipStreamSynchronize(c->stream);
        (void)dev_free(d_index);
        return rc;
    }
    c->un.link_first = d_index;  // (the launches behind it on the stream find it built)
    return KH_OK;
}

// The launch both forms share: d_support has n_links counters; the three counted words come back into stats, MISSING is derived.
// Drains the compute stream.
int support_run(kh_ctx *c, const u64 *d_run_start, u64 nrec, const uint32_t *d_runs, u64 n_runs, u64 *d_support, u64 *stats, SupportTimes &times) {
    const u64 states = 2 * c->un.n_unitigs, nl = c->un.n_links;
    u64 *const d_words = c->un.link_first + states;
    HIP_TRY(c, hipMemsetAsync(d_words, 0, KH_SUP_WORDS * sizeof(u64), c->stream));
    const u64 nt = (n_runs + kh::SUP_TILE - 1) / kh::SUP_TILE;
    const unsigned grid = (unsigned)(nt < (u64)grid_cap() ? nt : (u64)grid_cap());
    times.mark(c, 2);
    hipLaunchKernelGGL(kh::link_support_kernel, dim3(grid), dim3(kh::BLOCK), 0, c->stream, d_run_start, nrec, d_runs, n_runs, (const u64 *)c->un.links, nl,
                       (const u64 *)c->un.link_first, states, d_support, d_words);
    HIP_TRY(c, hipGetLastError());
    times.mark(c, 3);
    HIP_TRY(c, hipMemcpyAsync(stats, d_words, KH_SUP_WORDS * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stats[KH_SUP_MISSING] = stats[KH_SUP_ADJACENT] - stats[KH_SUP_CREDITED];
    return KH_OK;
}

// What both calls do before they touch anything: arguments, entry, live unitigs with links, the capacity.
int support_enter(kh_ctx *c, const char *who, const void *run_start, u64 nrec, const void *runs, u64 n_runs, const void *support, u64 cap) {
    if (!c) return KH_ERR_BAD_ARG;
    const std::string w(who);
    if ((n_runs && (!run_start || !runs)) || (nrec && !run_start) || (cap && !support)) return fail(c, KH_ERR_BAD_ARG, (w + ": NULL argument").c_str());
    if ((uintptr_t)runs & 3) return fail(c, KH_ERR_BAD_ARG, (w + ": runs is not 4-byte aligned").c_str());
    if (((uintptr_t)run_start | (uintptr_t)support) & 7) return fail(c, KH_ERR_BAD_ARG, (w + ": run_start or support is not 8-byte aligned").c_str());
    if (n_runs > (~0ull) / (KH_RUN_WORDS * sizeof(uint32_t)) || nrec > (~0ull) / sizeof(u64) - 1)
        return fail(c, KH_ERR_BAD_ARG, (w + ": n_runs or nrec is beyond any array").c_str());
    const int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (!c->un.live)
        return fail(c, KH_ERR_STATE, (w + ": no unitigs: kh_unitigs_begin_linked first (anything that changes the table makes them stale)").c_str());
    if (!c->un.linked) return fail(c, KH_ERR_STATE, (w + ": no links were built: kh_unitigs_begin_linked, not kh_unitigs_begin").c_str());
    if (cap < c->un.n_links) return fail(c, KH_ERR_RANGE, (w + ": support array too small").c_str());
    return KH_OK;
}

inline void stats_out(uint64_t *out, const u64 *stats) {
    if (out) memcpy(out, stats, KH_SUP_WORDS * sizeof(u64));
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_unitigs_link_support_device(kh_ctx *c, const uint64_t *d_run_start, uint64_t nrec, const uint32_t *d_runs, uint64_t n_runs,
                                              uint64_t *d_support, uint64_t cap, uint64_t *out) {
    static const char who[] = "kh_unitigs_link_support_device";
    int rc = support_enter(c, who, d_run_start, nrec, d_runs, n_runs, d_support, cap);
    if (rc != KH_OK) return rc;
    u64 stats[KH_SUP_WORDS] = {0, 0, 0, 0};
    if (n_runs >= 2 && nrec) {
        SupportTimes times(c);
        if ((rc = support_index(c, who, times)) != KH_OK) return rc;
        if ((rc = support_run(c, reinterpret_cast<const u64 *>(d_run_start), nrec, d_runs, n_runs, reinterpret_cast<u64 *>(d_support), stats, times)) != KH_OK)
            return rc;  // (the counters are complete, and the caller's buffers may go)
        times.report(who);
    }
    stats_out(out, stats);
    return KH_OK;
}

extern "C" int kh_unitigs_link_support(kh_ctx *c, const uint64_t *run_start, uint64_t nrec, const uint32_t *runs, uint64_t n_runs,
                                       uint64_t *support, uint64_t cap, uint64_t *out) {
    static const char who[] = "kh_unitigs_link_support";
    int rc = support_enter(c, who, run_start, nrec, runs, n_runs, support, cap);
    if (rc != KH_OK) return rc;
    for (u64 r = 0; r < nrec; ++r)
        if (run_start[r] > run_start[r + 1]) return fail(c, KH_ERR_BAD_ARG, "kh_unitigs_link_support: run_start is not ascending");
    if (nrec && run_start[nrec] != n_runs) return fail(c, KH_ERR_BAD_ARG, "kh_unitigs_link_support: run_start[nrec] is not n_runs");
    u64 stats[KH_SUP_WORDS] = {0, 0, 0, 0};
    if (n_runs >= 2 && nrec) {
        const u64 nl = c->un.n_links;
        const u64 b_off = up16((nrec + 1) * sizeof(u64)), b_rows = up16(n_runs * KH_RUN_WORDS * sizeof(uint32_t)), b_sup = up16(nl * sizeof(u64));
        // (the pinned staging of the way back, then the call's arrays, then the index: whichever allocation fails, nothing of the
        // index stays behind; the staging is the context's, as after a copy)
        if (nl && (rc = ensure_stage(c, (b_sup + 1) / 2, true)) != KH_OK) return rc;
        CallScratch sc(c);
        // (never the idle partition buffers: the chunks of a kh_result_text_* stream may live there)
        uint8_t *const mem = (uint8_t *)sc.fresh(b_off + b_rows + b_sup + 16);
        if (!mem) return soft_oom(c, "kh_unitigs_link_support: device memory for the offsets, the rows and the counters");
        SupportTimes times(c);
        if ((rc = support_index(c, who, times)) != KH_OK) return rc;
        u64 *const d_run_start = (u64 *)mem, *const d_support = (u64 *)(mem + b_off + b_rows);
        uint32_t *const d_runs = (uint32_t *)(mem + b_off);
        HIP_TRY(c, hipMemcpyAsync(d_run_start, run_start, (nrec + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_runs, runs, n_runs * KH_RUN_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (nl) HIP_TRY(c, hipMemsetAsync(d_support, 0, nl * sizeof(u64), c->stream));
        if ((rc = support_run(c, d_run_start, nrec, d_runs, n_runs, d_support, stats, times)) != KH_OK) return rc;
        // the counters come back once, through the pinned staging, and are ADDED
        if (nl && stats[KH_SUP_CREDITED]) {
            HIP_TRY(c, hipStreamSynchronize(c->cstream));  // (the staging buffers are free)
            const u64 room = 2 * c->stage_bytes / sizeof(u64);
            for (u64 off = 0; off < nl; off += room) {
                const u64 len = std::min(room, nl - off);
                HIP_TRY(c, hipMemcpyAsync(c->h_stage[0], d_support + off, len * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                const u64 *const h = reinterpret_cast<const u64 *>(c->h_stage[0]);
                for (u64 i = 0; i < len; ++i) support[off + i] += h[i];
            }
            c->stage_used[0] = c->stage_used[1] = false;  // (nothing in flight on the staging buffers)
        }
        times.report(who);
    }
    stats_out(out, stats);
    return KH_OK;
}
