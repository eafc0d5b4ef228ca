// paths.hip -- kh_unitigs_paths / kh_unitigs_paths_device: the words of kh_unitigs_locate* folded on the device into runs, one row
// of KH_RUN_WORDS words per maximal stretch of one record that walks one unitig in one direction (include/kmerhip.h,
// "RUN-COMPRESSED PATHS").  No reference counterpart.  The words never leave the device: per chunk of profile_chunk() window starts
//   locate_range (locate.hip)   the chunk's words, with the word in front of its first entry and the one behind its last
//   path_flags_kernel           per tile of 4096 entries: which entries begin a run (heads) and which end one (tails), as two
//                               bitmaps, and the tile's number of heads
//   device_scan                 the tiles' head counts -> the rank of every tile's first head within the chunk
//   path_emit_kernel            every head stores STATE, OFFSET and QSTART of its row, every tail QEND, the records that start in
//                               the tile their run_start
//   path_cover_kernel           once at the end: one pair of atomics per row into the coverage array
// Heads and tails alternate along the input (head, tail, head, tail, ...: a run is closed before the next opens), so the tail
// of run i is the tail with i + 1 heads at or in front of it: one count per tile ranks both ends.
#include "ctx.hip.h"
#include "paths_bits.h"

namespace kh {

// a tile's 4096 words with the one in front and the one behind, position p = entry + 1, one pad word per 16: a lane's 18 words
// start at 8-byte unit 17 lane -- the odd stride of locate_kernel's s_out
constexpr int PT_LDS = TILE + 2 + (TILE + 2) / 16 + 1;
__device__ __forceinline__ int pt_lds(int p) { return p + (p >> 4); }
constexpr int PT_RB = TILE / 32 + 2;  // record starts at the tile's entries 0 .. 4096, one bit each

// Heads and tails of one chunk.  wq[e] is the word of the chunk's entry e, window start G0 + e of the call, for -1 <= e <= ns (the
// two outer ones KH_LOC_NO_WINDOW where the call has no such window start); wq is 16-byte aligned.  Per tile the words come to LDS
// with 16-byte loads, the record boundaries that fall on the tile's entries 0 .. 4096 are marked in an LDS bitmap (a 256-ary
// search for the first, then 256 boundaries per round), and every lane flags its 16 entries:
//   P(e)    = a record starts at e, or word e does not continue word e - 1
//   head(e) = place(e) and e inside the records and P(e);  tail(e) = place(e) and e inside the records and P(e + 1)
// Out: the two masks of every lane (hm, tm: 16 bits per lane, 256 per tile), the tile's number of heads, and the index of the first
// boundary at or behind the tile's first entry.  Boundaries outside the
// contract mark other bits, never one outside the bitmap.
// kernel-resource-usage (gfx950, hipcc -O3): see DESIGN.md 4.17.
__global__ __launch_bounds__(BLOCK) void path_flags_kernel(const u64 *__restrict__ wq, uint32_t ns, u64 G0, const u64 *__restrict__ rec_start,
                                                           u64 nrec, uint16_t *__restrict__ hm, uint16_t *__restrict__ tm,
                                                           uint32_t *__restrict__ cnt, u64 *__restrict__ first, uint32_t nt) {
    __shared__ u64 s_w[PT_LDS];
    __shared__ uint32_t s_rb[PT_RB];
    __shared__ uint32_t s_wcnt[BLOCK / 64];

    const int tid = threadIdx.x;
    const u64 R0 = rec_start[0], RN = rec_start[nrec];  // the records own the window starts [R0, RN)
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint32_t tE = t * (uint32_t)TILE;  // the chunk's entry that is the tile's entry 0
#pragma unroll
        for (int r = 0; r < TILE / 2 / BLOCK; ++r) {
            const int e = 2 * (tid + r * BLOCK);
            const uint32_t ce = tE + (uint32_t)e;
            u64 a = KH_LOC_NONE, b = KH_LOC_NONE;
            if (ce + 1 <= ns) {
                const uint4 v = *reinterpret_cast<const uint4 *>(wq + ce);
                a = (u64)v.x | ((u64)v.y << 32);
                b = (u64)v.z | ((u64)v.w << 32);
            } else if (ce <= ns) {
                a = wq[ce];
            }
            s_w[pt_lds(e + 1)] = a;
            s_w[pt_lds(e + 2)] = b;
        }
        if (tid == 0) s_w[pt_lds(0)] = *(wq + (int64_t)tE - 1);
        if (tid == 1) s_w[pt_lds(TILE + 1)] = tE + (uint32_t)TILE <= ns ? wq[tE + TILE] : KH_LOC_NONE;
        for (int i = tid; i < PT_RB; i += BLOCK) s_rb[i] = 0u;
        __syncthreads();

        const u64 Gs = G0 + tE;
        u64 b0 = wg_first_not(0, nrec + 1, tid, [&](u64 i) { return rec_start[i] < Gs; });
        if (tid == 0) first[t] = b0;  // (path_emit_kernel goes on from there)
        for (;;) {  // (uniform: the count below is every lane's)
            const u64 idx = b0 + (u64)tid;
            bool go = false;
            if (idx <= nrec) {
                const u64 v = rec_start[idx];
                go = v <= Gs + TILE;
                if (v >= Gs && go) atomicOr(&s_rb[(uint32_t)(v - Gs) >> 5], 1u << ((uint32_t)(v - Gs) & 31u));
            }
            if (__syncthreads_count(go) < BLOCK) break;
            b0 += BLOCK;
        }

        u64 w[CHUNK + 2];
#pragma unroll
        for (int j = 0; j < CHUNK + 2; ++j) w[j] = s_w[pt_lds(CHUNK * tid + j)];
        const int sh = 16 * (tid & 1);
        const uint32_t rb = (uint32_t)(((((u64)s_rb[(tid >> 1) + 1]) << 32) | (u64)s_rb[tid >> 1]) >> sh) & 0x1FFFFu;
        uint32_t P = rb, ok = 0;  // P: bit i is P(lane's entry i), i <= 16
#pragma unroll
        for (int i = 0; i <= CHUNK; ++i) P |= (uint32_t)!kh_path_continues(w[i], w[i + 1]) << i;
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) {
            const uint32_t ce = tE + (uint32_t)(CHUNK * tid + i);
            const u64 G = G0 + ce;
            ok |= (uint32_t)(kh_path_is_place(w[i + 1]) && ce < ns && G >= R0 && G < RN) << i;
        }
        const uint32_t h = ok & P, tl = ok & (P >> 1);
        hm[(u64)t * BLOCK + tid] = (uint16_t)h;
        tm[(u64)t * BLOCK + tid] = (uint16_t)tl;
        uint32_t x = (uint32_t)__popc(h);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
        if ((tid & 63) == 0) s_wcnt[tid >> 6] = x;
        __syncthreads();  // (and s_w, s_rb are free for the next tile)
        if (tid == 0) {
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < BLOCK / 64; ++i) s += s_wcnt[i];
            cnt[t] = s;
        }
    }
}

// The rows of one chunk.  pre[t]: heads of the chunk in front of tile t (pre[nt]: all of them); carry[cur]: heads of the call in
// front of the chunk -- the first workgroup leaves carry[cur ^ 1] for the next chunk, a word nobody reads in this launch.  Per tile
// the lanes' head counts are scanned (shuffles, then the four waves through LDS), which ranks every head; a tail has the rank of
// the head in front of it.  The records that reach into the tile come to LDS 256 boundaries at a time, from the record that holds
// the tile's first entry (path_flags_kernel left the index of the first boundary at or behind it).  Lane i of a round stores
// run_start of record i if that record starts in the tile -- the rank in front of its first entry: right for an empty record and
// for several that start at one entry; the tile that ends at n_all, the call's last, also owns the records that start there --,
// and every lane finds the record of each of its run ends by a binary search over the staged boundaries: once per run end, never
// per window.  A head whose tail is the same lane's writes the whole row (one
// 16-byte store where runs is aligned); otherwise the head stores three words and the tail one.  Nothing at or behind row
// run_cap is written; offsets outside the contract leave run ends out or give them wrong words, never a store outside the arrays.
// kernel-resource-usage (gfx950, hipcc -O3): see DESIGN.md 4.17.
__global__ __launch_bounds__(BLOCK) void path_emit_kernel(const u64 *__restrict__ wq, uint32_t ns, u64 G0, u64 n_all,
                                                          const u64 *__restrict__ rec_start, u64 nrec, const uint16_t *__restrict__ hm,
                                                          const uint16_t *__restrict__ tm, const u64 *__restrict__ first,
                                                          const u64 *__restrict__ pre, u64 *__restrict__ carry,
                                                          int cur, uint32_t nt, u64 *__restrict__ run_start, uint32_t *__restrict__ runs,
                                                          u64 run_cap) {
    __shared__ u64 s_rs[BLOCK + 1];
    __shared__ uint32_t s_hpre[BLOCK + 1];
    __shared__ uint16_t s_hm[BLOCK + 2];
    __shared__ uint32_t s_ws[BLOCK / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool vec = (((uintptr_t)runs) & 15) == 0;
    const u64 base0 = carry[cur];
    if (blockIdx.x == 0 && tid == 0) carry[cur ^ 1] = base0 + pre[nt];

    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint32_t tE = t * (uint32_t)TILE;
        const uint32_t h = hm[(u64)t * BLOCK + tid], tl = tm[(u64)t * BLOCK + tid];
        const uint32_t mine = (uint32_t)__popc(h);
        uint32_t x = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_ws[wave] = x;
        __syncthreads();
        uint32_t excl = x - mine;
        for (int i = 0; i < wave; ++i) excl += s_ws[i];
        s_hpre[tid] = excl;
        s_hm[tid] = (uint16_t)h;
        if (tid == BLOCK - 1) {
            s_hpre[BLOCK] = excl + mine;
            s_hm[BLOCK] = 0;
        }
        __syncthreads();

        const u64 base = base0 + pre[t];
        const u64 Gs = G0 + tE;
        const uint32_t nE = ns - tE < (uint32_t)TILE ? ns - tE : (uint32_t)TILE;
        const uint32_t own = nE + (Gs + nE == n_all ? 1u : 0u);  // the record starts this tile owns: [Gs, Gs + own)
        const u64 b0 = first[t] <= nrec ? first[t] : nrec + 1;  // (what path_flags_kernel found)
        u64 rb = b0 ? b0 - 1 : 0;  // the record that holds Gs, if one does
        uint32_t m = h | tl;       // the lane's run ends that have no record yet
        uint32_t hc = excl;        // heads of the tile in front of the next of them
        while (rb < nrec) {        // (uniform)
            const int cnt = nrec - rb < (u64)BLOCK ? (int)(nrec - rb) : BLOCK;
            if (tid <= cnt) s_rs[tid] = rec_start[rb + tid];
            if (tid == 0 && cnt == BLOCK) s_rs[BLOCK] = rec_start[rb + BLOCK];
            __syncthreads();
            if (tid < cnt) {
                const u64 ra = s_rs[tid];
                if (ra - Gs < (u64)own) {  // (ra < Gs wraps beyond it)
                    const uint32_t e = (uint32_t)(ra - Gs);  // (<= TILE)
                    run_start[rb + tid] = base + s_hpre[e >> 4] + (uint32_t)__popc((uint32_t)s_hm[e >> 4] & ((1u << (e & 15u)) - 1u));
                }
            }
            const u64 lo = s_rs[0], hi = s_rs[cnt];
            bool have = false;  // a head of this lane whose row is not stored yet
            u64 prank = 0;
            uint32_t pstate = 0, poff = 0, pq = 0;
            auto flush = [&]() {
                if (have && prank < run_cap) {
                    uint32_t *const row = runs + prank * KH_RUN_WORDS;
                    row[KH_RUN_STATE] = pstate;
                    row[KH_RUN_OFFSET] = poff;
                    row[KH_RUN_QSTART] = pq;
                }
                have = false;
            };
            while (m) {
                const int i = __ffs(m) - 1;
                const uint32_t ce = tE + (uint32_t)(CHUNK * tid + i);
                const u64 G = G0 + ce;
                if (G >= hi) break;  // (a later round's)
                m &= m - 1u;
                const bool is_h = (h >> i) & 1u, is_t = (tl >> i) & 1u;
                if (G < lo) {  // (outside the contract: in no staged record)
                    hc += is_h;
                    continue;
                }
                int a = 0, b = cnt;  // the last boundary at or in front of G: its record is not empty
                while (b - a > 1) {
                    const int mid = (a + b) >> 1;
                    if (s_rs[mid] <= G) a = mid;
                    else b = mid;
                }
                const uint32_t q = (uint32_t)(G - s_rs[a]);
                if (is_h) {
                    flush();
                    const u64 word = wq[ce];
                    prank = base + hc;
                    ++hc;
                    pstate = kh_run_state(word);
                    poff = kh_run_offset(word);
                    pq = q;
                    have = true;
                }
                if (is_t) {
                    const u64 rank = base + hc - 1;  // (no head in front of it: outside the contract, and beyond every run_cap)
                    if (have) {
                        if (rank < run_cap) {
                            uint32_t *const row = runs + rank * KH_RUN_WORDS;
                            if (vec) {
                                *reinterpret_cast<uint4 *>(row) = make_uint4(pstate, poff, pq, q + 1u);
                            } else {
                                row[KH_RUN_STATE] = pstate;
                                row[KH_RUN_OFFSET] = poff;
                                row[KH_RUN_QSTART] = pq;
                                row[KH_RUN_QEND] = q + 1u;
                            }
                        }
                        have = false;
                    } else if (rank < run_cap) {
                        runs[rank * KH_RUN_WORDS + KH_RUN_QEND] = q + 1u;
                    }
                }
            }
            flush();
            const bool more = hi - Gs < (u64)own && rb + (u64)cnt < nrec;
            __syncthreads();  // (s_rs is free for the next round, s_hpre and s_hm for the next tile)
            if (!more) break;
            rb += (u64)cnt;
        }
        __syncthreads();
    }
}

// One lane per finished row: its windows and itself into the coverage array.  Two 64-bit atomics per run, none per window.
__global__ __launch_bounds__(BLOCK) void path_cover_kernel(const uint32_t *__restrict__ runs, u64 nruns, u64 *__restrict__ cover, u64 nu) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nruns; i += (u64)gridDim.x * BLOCK) {
        const uint32_t *const row = runs + i * KH_RUN_WORDS;
        const u64 u = row[KH_RUN_STATE] >> 1;
        if (u >= nu) continue;  // (never of a row this library wrote)
        atomicAdd(reinterpret_cast<unsigned long long *>(cover + u * KH_COV_WORDS + KH_COV_WINDOWS),
                  (unsigned long long)(row[KH_RUN_QEND] - row[KH_RUN_QSTART]));
        atomicAdd(reinterpret_cast<unsigned long long *>(cover + u * KH_COV_WORDS + KH_COV_RUNS), 1ull);
    }
}

}  // namespace kh

namespace khi {
namespace {

inline u64 up16(u64 x) { return (x + 15) & ~15ull; }

// Device memory of one call beside the words: per tile of a chunk the two bitmaps, the head count and its scan, the scan's own
// scratch, the first boundary of every tile, and the two carry words.
struct PathScratch {
    uint16_t *hm = nullptr, *tm = nullptr;
    uint32_t *cnt = nullptr;
    u64 *first = nullptr, *pre = nullptr, *scan = nullptr, *carry = nullptr;
    static u64 bytes(u64 chunk) {
        const u64 nt = (chunk + kh::TILE - 1) / kh::TILE;
        return 2 * up16(nt * kh::BLOCK * sizeof(uint16_t)) + up16(nt * sizeof(uint32_t)) + up16(nt * sizeof(u64)) + up16((nt + 1) * sizeof(u64)) +
               up16(device_scan_scratch(nt)) + 16;
    }
    uint8_t *carve(uint8_t *p, u64 chunk) {  // returns the first byte behind
        const u64 nt = (chunk + kh::TILE - 1) / kh::TILE;
        hm = (uint16_t *)p, p += up16(nt * kh::BLOCK * sizeof(uint16_t));
        tm = (uint16_t *)p, p += up16(nt * kh::BLOCK * sizeof(uint16_t));
        cnt = (uint32_t *)p, p += up16(nt * sizeof(uint32_t));
        first = (u64 *)p, p += up16(nt * sizeof(u64));
        pre = (u64 *)p, p += up16((nt + 1) * sizeof(u64));
        scan = (u64 *)p, p += up16(device_scan_scratch(nt));
        carry = (u64 *)p, p += 16;
        return p;
    }
};

// KH_FLAG_TRACE: where a call's device time goes -- events on the compute stream round every launch of every chunk, added up per step
// and printed once the stream has run dry (tools/unitig_probe.py --paths reads the line).  Without the flag nothing is recorded.
struct PathTimes {
    bool on;
    std::vector<hipEvent_t> ev;  // per chunk: before locate_range, behind it, behind the flags, the scan, the emit
    hipEvent_t cover[2] = {nullptr, nullptr};
    explicit PathTimes(const kh_ctx *c) : on(c->trace) {}
    static hipEvent_t now(kh_ctx *c) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) == hipSuccess) (void)hipEventRecord(e, c->stream);
        return e;
    }
    void mark(kh_ctx *c) {
        if (on) ev.push_back(now(c));
    }
    void report(const char *who) {  // (the stream is drained)
        if (!on) return;
        float ms[5] = {0, 0, 0, 0, 0}, t = 0;
        for (size_t i = 0; i + 4 < ev.size(); i += 5)
            for (int s = 0; s < 4; ++s)
                if (ev[i + s] && ev[i + s + 1] && hipEventElapsedTime(&t, ev[i + s], ev[i + s + 1]) == hipSuccess) ms[s] += t;
        if (cover[0] && cover[1] && hipEventElapsedTime(&t, cover[0], cover[1]) == hipSuccess) ms[4] = t;
        fprintf(stderr, "[kmerhip] %s: locate %.3f ms, flags %.3f ms, scan %.3f ms, emit %.3f ms, cover %.3f ms\n", who, ms[0], ms[1], ms[2], ms[3], ms[4]);
    }
    ~PathTimes() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : cover)
            if (e) (void)hipEventDestroy(e);
    }
};

// What the calls share once they have entered.  Device pointers: the record offsets, the two outputs, the coverage array or nullptr.
struct PathCall {
    u64 n, nrec, run_cap;
    const u64 *d_rec;
    u64 *d_run_start;
    uint32_t *d_runs;
    PathTimes *times;
};

// Chunk j of the call: ns window starts from a, whose bases (and qualities) lie on the device from window start a - front on.  words:
// 16-byte aligned room for ns + 3 of them.  Asynchronous on the compute stream.
int path_chunk(kh_ctx *c, const PathCall &pc, const PathScratch &ps, u64 j, u64 a, u64 ns, const uint8_t *d_from, const uint8_t *d_qfrom, u64 len,
               u64 *words) {
    const u64 front = a ? 1 : 0, behind = a + ns < pc.n ? 1 : 0;
    u64 *const wq = words + 2;  // entry 0 of the chunk: 16-byte aligned, with the word in front at wq[-1]
    if (!front) HIP_TRY(c, hipMemsetAsync(wq - 1, 0xFF, sizeof(u64), c->stream));
    if (!behind) HIP_TRY(c, hipMemsetAsync(wq + ns, 0xFF, sizeof(u64), c->stream));
    pc.times->mark(c);
    int rc = locate_range(c, d_from, d_qfrom, len, ns + front + behind, wq - front);
    if (rc != KH_OK) return rc;
    pc.times->mark(c);
    const u64 nt = (ns + kh::TILE - 1) / kh::TILE;
    const unsigned grid = (unsigned)(nt < (u64)grid_cap() ? nt : (u64)grid_cap());
    hipLaunchKernelGGL(kh::path_flags_kernel, dim3(grid), dim3(kh::BLOCK), 0, c->stream, (const u64 *)wq, (uint32_t)ns, a, pc.d_rec, pc.nrec, ps.hm,
                       ps.tm, ps.cnt, ps.first, (uint32_t)nt);
    HIP_TRY(c, hipGetLastError());
    pc.times->mark(c);
    if ((rc = device_scan(c, ps.cnt, nt, ps.pre, true, ps.scan)) != KH_OK) return rc;
    pc.times->mark(c);
    hipLaunchKernelGGL(kh::path_emit_kernel, dim3(grid), dim3(kh::BLOCK), 0, c->stream, (const u64 *)wq, (uint32_t)ns, a, pc.n, pc.d_rec, pc.nrec,
                       (const uint16_t *)ps.hm, (const uint16_t *)ps.tm, (const u64 *)ps.first, (const u64 *)ps.pre, ps.carry, (int)(j & 1), (uint32_t)nt, pc.d_run_start,
                       pc.d_runs, pc.run_cap);
    HIP_TRY(c, hipGetLastError());
    pc.times->mark(c);
    return KH_OK;
}

// The call's number of runs, once its last chunk (the nch-th) is launched: drains the compute stream.
int path_total(kh_ctx *c, const PathScratch &ps, u64 nch, u64 *total) {
    HIP_TRY(c, hipMemcpyAsync(total, ps.carry + (nch & 1), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return KH_OK;
}

int path_cover(kh_ctx *c, const uint32_t *d_runs, u64 total, u64 *d_cover, PathTimes &times) {
    if (!total) return KH_OK;
    if (times.on) times.cover[0] = PathTimes::now(c);
    hipLaunchKernelGGL(kh::path_cover_kernel, dim3((unsigned)grid_for(total)), dim3(kh::BLOCK), 0, c->stream, d_runs, total, d_cover,
                       c->un.n_unitigs);
    HIP_TRY(c, hipGetLastError());
    if (times.on) times.cover[1] = PathTimes::now(c);
    return KH_OK;
}

// The host form's results out of device memory, once the compute stream has run dry: through the pinned twin of the first chunk
// buffer, which nothing uses any more.  Not d2h_staged(): that may allocate its staging, and this call allocates nothing behind the
// place map, so that no failure leaves one behind.  add: 64-bit words, added to what dst holds.
int path_d2h(kh_ctx *c, void *dst, const void *d_src, u64 bytes, bool add) {
    const u64 room = (2 * pf_in_stride(c->pf_chunk) + c->pf_out_bytes * c->pf_chunk) & ~7ull;
    for (u64 off = 0; off < bytes; off += room) {
        const u64 len = std::min(room, bytes - off);
        HIP_TRY(c, hipMemcpyAsync(c->pf_h[0], (const uint8_t *)d_src + off, len, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (add) {
            u64 *const d = reinterpret_cast<u64 *>((uint8_t *)dst + off);
            const u64 *const h = reinterpret_cast<const u64 *>(c->pf_h[0]);
            for (u64 i = 0; i < len / sizeof(u64); ++i) d[i] += h[i];
        } else {
            staged_memcpy((uint8_t *)dst + off, c->pf_h[0], len);
        }
    }
    return KH_OK;
}

// What both calls do before they touch anything: arguments, entry, live unitigs.
int paths_enter(kh_ctx *c, const char *who, const void *bases, u64 n, const void *rec_start, u64 nrec, const void *run_start, const void *runs,
                u64 run_cap, const void *cover, const void *n_runs) {
    if (!c) return KH_ERR_BAD_ARG;
    const std::string w(who);
    if (!n_runs || (n && !bases) || (nrec && (!rec_start || !run_start)) || (run_cap && !runs))
        return fail(c, KH_ERR_BAD_ARG, (w + ": NULL argument").c_str());
    if ((uintptr_t)runs & 3) return fail(c, KH_ERR_BAD_ARG, (w + ": runs is not 4-byte aligned").c_str());
    if (((uintptr_t)rec_start | (uintptr_t)run_start | (uintptr_t)cover) & 7)
        return fail(c, KH_ERR_BAD_ARG, (w + ": rec_start, run_start or cover is not 8-byte aligned").c_str());
    if (run_cap > (~0ull) / (KH_RUN_WORDS * sizeof(uint32_t))) return fail(c, KH_ERR_BAD_ARG, (w + ": run_cap is beyond any array").c_str());
    return enter_unitigs(c, who);
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_unitigs_paths_device(kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, const uint64_t *d_rec_start,
                                       uint64_t nrec, uint64_t *d_run_start, uint32_t *d_runs, uint64_t run_cap, uint64_t *d_cover,
                                       uint64_t *n_runs) {
    static const char who[] = "kh_unitigs_paths_device";
    int rc = paths_enter(c, who, d_bases, n, d_rec_start, nrec, d_run_start, d_runs, run_cap, d_cover, n_runs);
    if (rc != KH_OK) return rc;
    *n_runs = 0;
    if (nrec == 0) return KH_OK;
    if (n == 0) {
        HIP_TRY(c, hipMemsetAsync(d_run_start, 0, (nrec + 1) * sizeof(u64), c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return KH_OK;
    }
    const u64 chunk = profile_chunk(c, n), nch = (n + chunk - 1) / chunk;
    CallScratch sc(c);
    // (never the idle partition buffers: the chunks of a kh_result_text_* stream may live there)
    uint8_t *const mem = (uint8_t *)sc.fresh((chunk + 4) * sizeof(u64) + PathScratch::bytes(chunk));
    if (!mem) return soft_oom(c, "kh_unitigs_paths_device: device memory for the chunk's words and flags");
    // (the scratch first: whichever allocation fails, nothing of the place map stays behind)
    if ((rc = locate_index(c, who)) != KH_OK) return rc;
    PathScratch ps;
    ps.carve(mem + (chunk + 4) * sizeof(u64), chunk);
    HIP_TRY(c, hipMemsetAsync(ps.carry, 0, 2 * sizeof(u64), c->stream));
    PathTimes times(c);
    const PathCall pc{n, nrec, run_cap, reinterpret_cast<const u64 *>(d_rec_start), reinterpret_cast<u64 *>(d_run_start), d_runs, &times};
    for (u64 j = 0; j < nch; ++j) {
        const u64 a = j * chunk, ns = std::min<u64>(chunk, n - a), from = a - (a ? 1 : 0);
        if ((rc = path_chunk(c, pc, ps, j, a, ns, d_bases + from, d_qual ? d_qual + from : nullptr, n - from, (u64 *)mem)) != KH_OK) return rc;
    }
    u64 total = 0;
    if ((rc = path_total(c, ps, nch, &total)) != KH_OK) return rc;
    *n_runs = total;
    HIP_TRY(c, hipMemcpyAsync(d_run_start + nrec, &total, sizeof(u64), hipMemcpyHostToDevice, c->stream));
    if (total <= run_cap && d_cover && (rc = path_cover(c, d_runs, total, reinterpret_cast<u64 *>(d_cover), times)) != KH_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the outputs are complete, and the caller's buffers may go)
    times.report(who);
    if (total > run_cap) return fail(c, KH_ERR_RANGE, "kh_unitigs_paths_device: more runs than run_cap (n_runs and run_start are complete)");
    return KH_OK;
}

extern "C" int kh_unitigs_paths(kh_ctx *c, const uint8_t *bases, const uint8_t *qual, uint64_t n, const uint64_t *rec_start, uint64_t nrec,
                                uint64_t *run_start, uint32_t *runs, uint64_t run_cap, uint64_t *cover, uint64_t *n_runs) {
    static const char who[] = "kh_unitigs_paths";
    int rc = paths_enter(c, who, bases, n, rec_start, nrec, run_start, runs, run_cap, cover, n_runs);
    if (rc != KH_OK) return rc;
    // (after enter(), unlike kh_profile_records: a poisoned context reports that before a bad rec_start)
    if ((rc = check_rec_start(c, who, reinterpret_cast<const u64 *>(rec_start), nrec, n)) != KH_OK) return rc;
    *n_runs = 0;
    if (nrec == 0) return KH_OK;
    if (n == 0) {
        memset(run_start, 0, (nrec + 1) * sizeof(u64));
        return KH_OK;
    }
    const u64 chunk = profile_chunk(c, n), nch = (n + chunk - 1) / chunk;
    const u64 nu = c->un.n_unitigs;
    // (the staging and the call's arrays first: whichever allocation fails, nothing of the place map stays behind)
    if ((rc = profile_buffers(c, chunk + 4, sizeof(u64), "kh_unitigs_paths: chunk buffers")) != KH_OK) return rc;  // (+ 4: the words in front and behind)
    CallScratch sc(c);
    const u64 b_off = up16((nrec + 1) * sizeof(u64)), b_rows = up16(run_cap * KH_RUN_WORDS * sizeof(uint32_t)),
              b_cov = cover ? up16(nu * KH_COV_WORDS * sizeof(u64)) : 0;
    uint8_t *const mem = (uint8_t *)sc.fresh(PathScratch::bytes(chunk) + 2 * b_off + b_rows + b_cov + 16);
    if (!mem) return soft_oom(c, "kh_unitigs_paths: device memory for the flags, the offsets, the rows and the coverage");
    if ((rc = locate_index(c, who)) != KH_OK) return rc;
    PathScratch ps;
    uint8_t *p = ps.carve(mem, chunk);
    u64 *const d_rec = (u64 *)p, *const d_run_start = (u64 *)(p + b_off);
    uint32_t *const d_runs = (uint32_t *)(p + 2 * b_off);
    u64 *const d_cover = cover ? (u64 *)(p + 2 * b_off + b_rows) : nullptr;
    HIP_TRY(c, hipMemsetAsync(ps.carry, 0, 2 * sizeof(u64), c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_rec, rec_start, (nrec + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    if (d_cover && nu) HIP_TRY(c, hipMemsetAsync(d_cover, 0, nu * KH_COV_WORDS * sizeof(u64), c->stream));
    PathTimes times(c);
    const PathCall pc{n, nrec, run_cap, d_rec, d_run_start, d_runs, &times};
    // The bases travel as in kh_unitigs_locate, from the window start in front of a chunk's first to the one behind its last (the halo);
    // nothing of a chunk comes back, and its words lie where kh_unitigs_locate's would.
    rc = chunk_pipeline(c, bases, qual, n, chunk, 1, nullptr, 0, [&](const ChunkJob &job) {
        return path_chunk(c, pc, ps, job.j, job.a, job.ns, job.d_bases, job.d_qual, job.len, reinterpret_cast<u64 *>(job.d_tail));
    });
    if (rc != KH_OK) return rc;
    u64 total = 0;
    if ((rc = path_total(c, ps, nch, &total)) != KH_OK) return rc;
    *n_runs = total;
    // the offsets, the rows and the coverage come back once
    if ((rc = path_d2h(c, run_start, d_run_start, nrec * sizeof(u64), false)) != KH_OK) return rc;
    run_start[nrec] = total;
    if (total > run_cap) return fail(c, KH_ERR_RANGE, "kh_unitigs_paths: more runs than run_cap (n_runs and run_start are complete)");
    if ((rc = path_d2h(c, runs, d_runs, total * KH_RUN_WORDS * sizeof(uint32_t), false)) != KH_OK) return rc;
    if (d_cover && nu && total) {
        if ((rc = path_cover(c, d_runs, total, d_cover, times)) != KH_OK) return rc;
        if ((rc = path_d2h(c, cover, d_cover, nu * KH_COV_WORDS * sizeof(u64), true)) != KH_OK) return rc;
    }
    times.report(who);
    return KH_OK;
}
