// profile.hip -- kh_profile / kh_profile_device: the table's count of the canonical k-mer at every window start of new
// sequences (what `jellyfish query -s` answers per read).  No reference counterpart beyond `kmerust query` for ONE k-mer
// (src/main.rs:264-280); the window rules are those of counting (src/run.rs:526-571), by construction: the kernel is built
// from the counting path's tile staging and Roller (kernels.hip.h) and differs from count_direct_kernel only in what it does
// with a key -- a read of its slot where that kernel issues an atomic.
//   profile_kernel<QUAL, TAB>      TAB = PfWide: the 16-byte table; PfNarrow: the 8-byte image (partition.hip.h), as it is
//   kh_profile_device              one launch over the caller's device buffers
//   kh_profile                     the same in chunks through pinned staging: H2D, kernel and D2H of successive chunks overlap
//   profile_records_kernel<QUAL, TAB>   the same first half; the tile's results are reduced per record in LDS instead of stored
//   kh_profile_records_device / kh_profile_records   one row of KH_REC_WORDS words per record: 32 bytes cross the link, not 4 per base
#include "ctx.hip.h"
#include "probe.hip.h"

namespace kh {

constexpr uint32_t PF_NO_WINDOW = KH_PROFILE_NO_WINDOW;
// a tile's 4096 results in LDS, one pad word per 32: lane l writes word j of its 16 to bank (j + l / 2 + 16 (l & 1)) mod 32 and
// the store phase reads words 4 apart -- both without a bank conflict
constexpr int PF_LDS = TILE + TILE / 32;
__device__ __forceinline__ int pf_lds(int e) { return e + (e >> 5); }

// out[i] for every window start i < nout of the data [vbeg, vend) (virtual positions over abase, as in count_direct_kernel):
// the count of the window's canonical k-mer, or PF_NO_WINDOW where counting would see no window.  A lane's 16 results are the
// windows ENDING at its 16 bases -- entries p0 - (k - 1) - vbeg .. + 15 of out -- so a tile's 4096 results are one contiguous
// run of out, k - 1 entries behind the tile: they go through LDS and leave as whole 16-byte units at 16-byte-aligned
// addresses (a wave's store instruction is then 1 KiB of consecutive lines), with single words only in front of the first
// aligned unit, behind the last, and at the two ends of out.  Tiles abut in out as they do in the data: every entry is
// written exactly once.  The tiles run k - 1 positions past the data, where every window is invalid: the trailing entries.
template <bool QUAL, typename TAB>
__global__ __launch_bounds__(BLOCK) void profile_kernel(const uint8_t *__restrict__ abase, const uint8_t *__restrict__ qbase,
                                                        int qaligned, u64 vbeg, u64 vend, u64 ntiles, uint32_t tiles_per_block,
                                                        uint32_t k, uint32_t thr, TAB tab, uint32_t *__restrict__ out, u64 nout) {
    __shared__ uint32_t s_code[2][BLOCK + 2];
    __shared__ uint16_t s_val[2][BLOCK + 2];
    __shared__ uint32_t s_out[PF_LDS];

    const int tid = threadIdx.x;
    const u64 tb = (u64)blockIdx.x * tiles_per_block;
    u64 te = tb + tiles_per_block;
    if (te > ntiles) te = ntiles;

    int buf = 0;
    for (u64 t = tb; t < te; ++t, buf ^= 1) {
        const WinCtx w = stage_tile<QUAL, BLOCK>(s_code, s_val, buf, t == tb, tid, abase, qbase, qaligned, t, vbeg, vend, thr);
        Roller roll;
        roll.init(w, k, 0);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            u64 key[8];
            typename TAB::Ref ref[8];
            typename TAB::Word first[8];
            uint32_t ok = 0;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) ok |= (uint32_t)roll.next(half * 8 + jj, key[jj]) << jj;
            // eight first-slot loads in flight before the first of them is looked at (one random table line per valid window)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                ref[jj] = tab.ref(key[jj]);
                first[jj] = TAB::free_word();
                if ((ok & (1u << jj)) && ref[jj].mine) first[jj] = TAB::load(ref[jj]);
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const uint32_t res = (ok & (1u << jj)) ? TAB::resolve(ref[jj], first[jj]) : PF_NO_WINDOW;
                s_out[pf_lds(tid * CHUNK + half * 8 + jj)] = res;
            }
        }
        __syncthreads();
        // (the next tile's results are written behind the barrier of its stage_tile: every lane is past these reads by then)
        const int64_t T0 = (int64_t)(t * (u64)TILE) - (int64_t)(k - 1) - (int64_t)vbeg;  // entry of out the tile's first result is
        const uint32_t sh = (uint32_t)(-((int64_t)((uintptr_t)out >> 2) + T0)) & 3u;      // results in front of the first aligned unit
        if ((uint32_t)tid < sh) {
            const int64_t gi = T0 + tid;
            if (gi >= 0 && (u64)gi < nout) out[gi] = s_out[tid];
        }
#pragma unroll
        for (int r = 0; r < TILE / 4 / BLOCK; ++r) {
            const int e0 = (int)sh + 4 * (tid + r * BLOCK);
            const int64_t gi = T0 + e0;
            if (e0 + 3 < TILE && gi >= 0 && (u64)gi + 3 < nout) {
                *reinterpret_cast<uint4 *>(out + gi) =
                    make_uint4(s_out[pf_lds(e0)], s_out[pf_lds(e0 + 1)], s_out[pf_lds(e0 + 2)], s_out[pf_lds(e0 + 3)]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = e0 + i;
                    const int64_t g = gi + i;
                    if (e < TILE && g >= 0 && (u64)g < nout) out[g] = s_out[pf_lds(e)];
                }
            }
        }
    }
}

// ---- per-record reduction ---------------------------------------------------------------------------------------------------
// What one (tile, record) part contributes to its record's row.  The three counts share a word, 16 bits each (a part has at most
// TILE = 4096 entries); first = the tile entry of the first window below lo.
struct PrAcc {
    u64 cnt;  // windows | present << 16 | in_range << 32
    u64 sum;
    uint32_t mn, mx, first;
};
__device__ __forceinline__ PrAcc pr_none() { return PrAcc{0ull, 0ull, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu}; }
constexpr int PR_BIG = 1024;  // entries from which a part is reduced by the whole workgroup (at most TILE / PR_BIG of them per tile)
constexpr int PR_WAVES = BLOCK / 64;

__device__ __forceinline__ void pr_add(PrAcc &x, uint32_t v, uint32_t e, uint32_t lo, uint32_t hi) {
    if (v == PF_NO_WINDOW) return;
    x.cnt += 1ull | ((u64)(v > 0u) << 16) | ((u64)(v >= lo && v <= hi) << 32);
    x.sum += v;
    x.mn = min(x.mn, v);
    x.mx = max(x.mx, v);
    if (v < lo) x.first = min(x.first, e);
}
__device__ __forceinline__ void pr_merge(PrAcc &x, const PrAcc &y) {
    x.cnt += y.cnt;
    x.sum += y.sum;
    x.mn = min(x.mn, y.mn);
    x.mx = max(x.mx, y.mx);
    x.first = min(x.first, y.first);
}
__device__ __forceinline__ PrAcc pr_wave_reduce(PrAcc x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        PrAcc y;
        y.cnt = __shfl_xor(x.cnt, d);
        y.sum = __shfl_xor(x.sum, d);
        y.mn = __shfl_xor(x.mn, d);
        y.mx = __shfl_xor(x.mx, d);
        y.first = __shfl_xor(x.first, d);
        pr_merge(x, y);
    }
    return x;
}

// One part into its row.  whole: the part is the whole record (the row is this part's alone: plain stores, 16 bytes at a time where
// the rows are 16-byte aligned); otherwise one set of return-less atomics.  sumw: the word the 64-bit sum starts at while the rows
// are accumulated -- KH_REC_SUM_LO where that is 8-byte aligned, else one behind it with first_low in its place (profile_records_finalize
// puts the words where they belong).  A part without a window changes nothing of a pre-set row.
__device__ __forceinline__ void pr_emit(uint32_t *__restrict__ row, const PrAcc &x, bool whole, uint32_t first_off, int sumw, bool vec) {
    const uint32_t windows = (uint32_t)x.cnt & 0xFFFFu, present = (uint32_t)(x.cnt >> 16) & 0xFFFFu, in_range = (uint32_t)(x.cnt >> 32) & 0xFFFFu;
    if (!windows) return;
    const int flw = sumw == KH_REC_SUM_LO ? KH_REC_FIRST_LOW : KH_REC_SUM_LO;
    if (whole) {
        uint32_t w[KH_REC_WORDS];
        w[KH_REC_WINDOWS] = windows;
        w[KH_REC_PRESENT] = present;
        w[KH_REC_IN_RANGE] = in_range;
        w[KH_REC_MIN] = x.mn;
        w[KH_REC_MAX] = x.mx;
        w[sumw] = (uint32_t)x.sum;
        w[sumw + 1] = (uint32_t)(x.sum >> 32);
        w[flw] = first_off;
        if (vec) {
            reinterpret_cast<uint4 *>(row)[0] = make_uint4(w[0], w[1], w[2], w[3]);
            reinterpret_cast<uint4 *>(row)[1] = make_uint4(w[4], w[5], w[6], w[7]);
        } else {
#pragma unroll
            for (int i = 0; i < KH_REC_WORDS; ++i) row[i] = w[i];
        }
    } else {
        atomicAdd(row + KH_REC_WINDOWS, windows);
        if (present) atomicAdd(row + KH_REC_PRESENT, present);
        if (in_range) atomicAdd(row + KH_REC_IN_RANGE, in_range);
        atomicMin(row + KH_REC_MIN, x.mn);
        atomicMax(row + KH_REC_MAX, x.mx);
        if (x.sum) atomicAdd(reinterpret_cast<unsigned long long *>(row + sumw), (unsigned long long)x.sum);
        if (first_off != 0xFFFFFFFFu) atomicMin(row + flw, first_off);
    }
}

// Rows before the parts arrive: the identities of the reductions.
__global__ __launch_bounds__(BLOCK) void profile_records_preset(uint32_t *__restrict__ rows, u64 nrec, int sumw) {
    const int flw = sumw == KH_REC_SUM_LO ? KH_REC_FIRST_LOW : KH_REC_SUM_LO;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nrec * KH_REC_WORDS; i += (u64)gridDim.x * BLOCK) {
        const int w = (int)(i & (KH_REC_WORDS - 1));
        rows[i] = (w == KH_REC_MIN || w == flw) ? 0xFFFFFFFFu : 0u;
    }
}
// ... and after the last part: min of a record without a window is 0, and the sum and first_low go to their words.
__global__ __launch_bounds__(BLOCK) void profile_records_finalize(uint32_t *__restrict__ rows, u64 nrec, int sumw) {
    for (u64 r = (u64)blockIdx.x * BLOCK + threadIdx.x; r < nrec; r += (u64)gridDim.x * BLOCK) {
        uint32_t *row = rows + r * KH_REC_WORDS;
        if (row[KH_REC_WINDOWS] == 0u) row[KH_REC_MIN] = 0u;
        if (sumw != KH_REC_SUM_LO) {
            const uint32_t fl = row[5], slo = row[6], shi = row[7];
            row[KH_REC_SUM_LO] = slo;
            row[KH_REC_SUM_HI] = shi;
            row[KH_REC_FIRST_LOW] = fl;
        }
    }
}

// profile_kernel up to the tile's 4096 results in LDS; then, instead of the store phase, a segmented reduction: entry e of the
// tile is window start G = out0 + T0 + e of the caller's buffer (out0: where this launch's entry 0 lies -- the chunk offset of the host
// form), record r owns rec_start[r] <= G < rec_start[r + 1].  The workgroup finds the first record that reaches into its first tile
// with a 256-ary search over [r_lo, r_hi) (one load per lane and round), later tiles go on where the last one stopped.  The record
// boundaries of a tile come to LDS 256 at a time; parts of fewer than PR_BIG entries are spread over the four waves (a wave per
// part: lanes stride over the entries, then a shuffle reduction), longer ones are reduced by the whole workgroup.  A record that
// lies inside one tile's run is written with plain stores; one that crosses a tile's edge -- which covers the edge between two
// workgroups, and between two chunks of the host form -- adds each part with one set of atomics.  Never an atomic per window.
// Offsets outside the contract (not ascending) give wrong rows, never an access outside s_out or the nrec rows: a part is
// clipped to the tile's run before it is read.
template <bool QUAL, typename TAB>
__global__ __launch_bounds__(BLOCK) void profile_records_kernel(const uint8_t *__restrict__ abase, const uint8_t *__restrict__ qbase,
                                                                int qaligned, u64 vbeg, u64 vend, u64 ntiles, uint32_t tiles_per_block,
                                                                uint32_t k, uint32_t thr, TAB tab, u64 nout, const u64 *__restrict__ rec_start,
                                                                u64 r_lo, u64 r_hi, u64 out0, uint32_t lo, uint32_t hi,
                                                                uint32_t *__restrict__ rows, int sumw) {
    __shared__ uint32_t s_code[2][BLOCK + 2];
    __shared__ uint16_t s_val[2][BLOCK + 2];
    __shared__ uint32_t s_out[PF_LDS];
    __shared__ u64 s_rs[BLOCK + 1];
    __shared__ PrAcc s_part[PR_WAVES];
    __shared__ uint32_t s_big[TILE / PR_BIG];
    __shared__ uint32_t s_nbig;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool vec = (((uintptr_t)rows) & 15) == 0;
    const u64 tb = (u64)blockIdx.x * tiles_per_block;
    u64 te = tb + tiles_per_block;
    if (te > ntiles) te = ntiles;

    u64 rcur = 0;
    bool searched = false;
    int buf = 0;
    for (u64 t = tb; t < te; ++t, buf ^= 1) {
        const WinCtx w = stage_tile<QUAL, BLOCK>(s_code, s_val, buf, t == tb, tid, abase, qbase, qaligned, t, vbeg, vend, thr);
        Roller roll;
        roll.init(w, k, 0);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            u64 key[8];
            typename TAB::Ref ref[8];
            typename TAB::Word first[8];
            uint32_t ok = 0;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) ok |= (uint32_t)roll.next(half * 8 + jj, key[jj]) << jj;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                ref[jj] = tab.ref(key[jj]);
                first[jj] = TAB::free_word();
                if ((ok & (1u << jj)) && ref[jj].mine) first[jj] = TAB::load(ref[jj]);
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const uint32_t res = (ok & (1u << jj)) ? TAB::resolve(ref[jj], first[jj]) : PF_NO_WINDOW;
                s_out[pf_lds(tid * CHUNK + half * 8 + jj)] = res;
            }
        }
        __syncthreads();
        // (the next tile's results are written behind the barrier of its stage_tile: every lane is past the reads below by then)
        const int64_t T0 = (int64_t)(t * (u64)TILE) - (int64_t)(k - 1) - (int64_t)vbeg;  // entry of this launch the tile's first result is
        const int64_t e_lo = T0 < 0 ? -T0 : 0;
        const int64_t e_hi = (int64_t)nout - T0 < (int64_t)TILE ? (int64_t)nout - T0 : (int64_t)TILE;
        if (e_lo >= e_hi) continue;  // (uniform: a tile in front of entry 0 or behind the last)
        const int64_t G0 = (int64_t)out0 + T0;  // window start of the tile's entry 0
        const u64 Gs = (u64)(G0 + e_lo), Ge = (u64)(G0 + e_hi);

        if (!searched) {  // the first record that ends behind Gs (r_hi: none)
            rcur = wg_first_not(r_lo, r_hi, tid, [&](u64 r) { return rec_start[r + 1] <= Gs; });
            searched = true;
        }

        u64 rb = rcur;
        while (rb < r_hi) {
            const int cnt = r_hi - rb < (u64)BLOCK ? (int)(r_hi - rb) : BLOCK;
            if (tid <= cnt) s_rs[tid] = rec_start[rb + tid];
            if (tid == 0) {
                if (cnt == BLOCK) s_rs[BLOCK] = rec_start[rb + BLOCK];
                s_nbig = 0;
            }
            __syncthreads();
            bool ends_here = false;
            if (tid < cnt) {
                const u64 ra = s_rs[tid], re = s_rs[tid + 1];
                ends_here = re <= Ge;
                const u64 a = ra > Gs ? ra : Gs, b = re < Ge ? re : Ge;
                if (b > a && b - a >= (u64)PR_BIG) {
                    // (ascending offsets give disjoint parts, so at most TILE / PR_BIG long ones; others must not overrun s_big)
                    const uint32_t slot = atomicAdd(&s_nbig, 1u);
                    if (slot < (uint32_t)(TILE / PR_BIG)) s_big[slot] = (uint32_t)tid;
                }
            }
            const int nskip = __syncthreads_count(ends_here);  // records of this batch that end inside the tile's run: a prefix
            const int nparts = nskip < cnt ? nskip + 1 : cnt;
            // short parts: a wave each
            for (int p = wave; p < nparts; p += PR_WAVES) {
                const u64 ra = s_rs[p], re = s_rs[p + 1];
                const u64 a = ra > Gs ? ra : Gs, b = re < Ge ? re : Ge;
                if (b <= a || b - a >= (u64)PR_BIG) continue;
                const int ea = (int)((int64_t)a - G0), eb = (int)((int64_t)b - G0);
                PrAcc x = pr_none();
                for (int e = ea + lane; e < eb; e += 64) pr_add(x, s_out[pf_lds(e)], (uint32_t)e, lo, hi);
                x = pr_wave_reduce(x);
                if (lane == 0) {
                    const uint32_t fo = x.first == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)((u64)(G0 + (int64_t)x.first) - ra);
                    pr_emit(rows + (rb + (u64)p) * KH_REC_WORDS, x, a == ra && b == re, fo, sumw, vec);
                }
            }
            // long parts: the workgroup
            const uint32_t nbig = s_nbig < (uint32_t)(TILE / PR_BIG) ? s_nbig : (uint32_t)(TILE / PR_BIG);
            for (uint32_t q = 0; q < nbig; ++q) {
                const int p = (int)s_big[q];
                const u64 ra = s_rs[p], re = s_rs[p + 1];
                const u64 a = ra > Gs ? ra : Gs, b = re < Ge ? re : Ge;
                const int ea = (int)((int64_t)a - G0), eb = (int)((int64_t)b - G0);
                PrAcc x = pr_none();
                for (int e = ea + tid; e < eb; e += BLOCK) pr_add(x, s_out[pf_lds(e)], (uint32_t)e, lo, hi);
                x = pr_wave_reduce(x);
                if (lane == 0) s_part[wave] = x;
                __syncthreads();
                if (tid == 0) {
#pragma unroll
                    for (int i = 1; i < PR_WAVES; ++i) pr_merge(x, s_part[i]);
                    const uint32_t fo = x.first == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)((u64)(G0 + (int64_t)x.first) - ra);
                    pr_emit(rows + (rb + (u64)p) * KH_REC_WORDS, x, a == ra && b == re, fo, sumw, vec);
                }
                __syncthreads();
            }
            rb += (u64)nskip;
            __syncthreads();  // (s_rs, s_big and s_nbig are free for the next batch / tile)
            if (nskip < cnt) break;  // record rb reaches beyond the tile: the next tile starts with it
        }
        rcur = rb;
    }
}

}  // namespace kh

namespace khi {

constexpr u64 PF_CHUNK_MAX = 4ull << 20;   // window starts per chunk of kh_profile: 4 MiB of bases in, 16 MiB of profile out
constexpr u64 PF_CHUNK_MIN = 64ull << 10;

// the chunk buffers and events of the four host forms (profile_buffers grows them by releasing them first)
static void chunk_release(kh_ctx *c) {
    for (int i = 0; i < 2; ++i) {
        if (c->pf_d[i]) (void)dev_free(c->pf_d[i]);
        if (c->pf_h[i]) (void)pin_free(c->pf_h[i]);
        c->pf_d[i] = c->pf_h[i] = nullptr;
        hipEvent_t *ev[] = {&c->pf_in[i], &c->pf_run[i], &c->pf_out[i]};
        for (hipEvent_t *e : ev) {
            if (*e) (void)hipEventDestroy(*e);
            *e = nullptr;
        }
    }
    c->pf_chunk = 0;
    c->pf_out_bytes = 0;
}

void profile_release(kh_ctx *c) {
    chunk_release(c);
    if (c->pr_rows) (void)dev_free(c->pr_rows);
    if (c->pr_rec) (void)dev_free(c->pr_rec);
    c->pr_rows = nullptr;
    c->pr_rec = nullptr;
    c->pr_rows_cap = c->pr_rec_cap = 0;
}

// Window starts per chunk of a host form over n bytes.
u64 profile_chunk(const kh_ctx *c, u64 n) {
    u64 chunk = PF_CHUNK_MIN;
    while (chunk < n && chunk < PF_CHUNK_MAX) chunk *= 2;
#if KH_TESTING
    if (c->knobs.profile_chunk_kb) chunk = c->knobs.profile_chunk_kb << 10;  // (tests: chunk edges inside reads and records)
#endif
    return chunk;
}

// The two chunk buffers on the device ([bases | qualities | out_bytes per window start]) and their pinned twins, for `chunk` window
// starts each.  Buffers that are too small in either measure are released and allocated again for the larger of both.
int profile_buffers(kh_ctx *c, u64 chunk, u64 out_bytes, const char *who) {
    if (!c->cstream) HIP_TRY(c, hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    if (!c->cstream2) HIP_TRY(c, hipStreamCreateWithFlags(&c->cstream2, hipStreamNonBlocking));
    if (c->pf_chunk < chunk || c->pf_out_bytes < out_bytes) {
        chunk = std::max(chunk, c->pf_chunk);
        out_bytes = std::max(out_bytes, c->pf_out_bytes);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        chunk_release(c);
        const u64 bytes = 2 * pf_in_stride(chunk) + out_bytes * chunk;
        for (int i = 0; i < 2; ++i) {
            hipError_t e = dev_malloc((void **)&c->pf_d[i], bytes);
            if (e == hipSuccess) e = pin_malloc((void **)&c->pf_h[i], bytes, hipHostMallocDefault);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                chunk_release(c);
                return soft_oom(c, who, e);  // (a reading call: the context stays usable)
            }
        }
        c->pf_chunk = chunk;
        c->pf_out_bytes = out_bytes;
    }
    for (int i = 0; i < 2; ++i) {
        hipEvent_t *ev[] = {&c->pf_in[i], &c->pf_run[i], &c->pf_out[i]};
        for (hipEvent_t *e : ev)
            if (!*e) HIP_TRY(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    return KH_OK;
}

int chunk_pipeline(kh_ctx *c, const uint8_t *bases, const uint8_t *qual, u64 n, u64 chunk, u64 halo, void *out, u64 out_bytes,
                   const std::function<int(const ChunkJob &)> &launch) {
    const bool with_qual = qual_filter(c, qual);
    // pinned / registered caller memory: the copy engine reads and writes it itself, no bounce through pf_h
    const bool in_direct = is_pinned_host(bases) && (!with_qual || is_pinned_host(qual));
    const bool out_direct = out && is_pinned_host(out);
    const u64 stride = pf_in_stride(c->pf_chunk), k1 = c->k - 1;  // (the buffers' real size, not this call's chunk)
    const u64 nch = (n + chunk - 1) / chunk;
    // Chunk j owns the window starts [j chunk, (j + 1) chunk).  A window is answered by the chunk that holds its start, so no entry
    // of out is written twice.
    auto finish = [&](u64 j) -> int {  // chunk j has arrived in pinned memory: out of the bounce buffer
        const int b = (int)(j & 1);
        HIP_TRY(c, hipEventSynchronize(c->pf_out[b]));
        if (!out_direct) staged_memcpy((uint8_t *)out + out_bytes * j * chunk, c->pf_h[b] + 2 * stride, out_bytes * std::min(chunk, n - j * chunk));
        return KH_OK;
    };
    for (u64 j = 0; j < nch; ++j) {
        // The buffers of chunk j were those of chunk j - 2, which the last round saw complete: with out, finish() saw its results
        // arrive; without, the host waited for its kernel.
        const int b = (int)(j & 1);
        const u64 a = j * chunk, ns = std::min(chunk, n - a), from = a - (halo && a ? 1 : 0);
        const u64 len = std::min(a + ns + halo + k1, n) - from;
        uint8_t *const d = c->pf_d[b], *const h = c->pf_h[b];
        if (!in_direct) {
            staged_memcpy(h, bases + from, len);
            if (with_qual) staged_memcpy(h + stride, qual + from, len);
        }
        HIP_TRY(c, hipMemcpyAsync(d, in_direct ? bases + from : h, len, hipMemcpyHostToDevice, c->cstream));
        if (with_qual) HIP_TRY(c, hipMemcpyAsync(d + stride, in_direct ? qual + from : h + stride, len, hipMemcpyHostToDevice, c->cstream));
        HIP_TRY(c, hipEventRecord(c->pf_in[b], c->cstream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->pf_in[b], 0));
        int rc = launch(ChunkJob{j, a, ns, d, with_qual ? d + stride : nullptr, len, d + 2 * stride});
        if (rc != KH_OK) return rc;
        HIP_TRY(c, hipEventRecord(c->pf_run[b], c->stream));
        if (!out) {
            if (j) HIP_TRY(c, hipEventSynchronize(c->pf_run[b ^ 1]));
            continue;
        }
        // the results of chunk j travel on a stream of their own, beside the kernel of chunk j + 1
        HIP_TRY(c, hipStreamWaitEvent(c->cstream2, c->pf_run[b], 0));
        HIP_TRY(c, hipMemcpyAsync(out_direct ? (uint8_t *)out + out_bytes * a : h + 2 * stride, d + 2 * stride, out_bytes * ns, hipMemcpyDeviceToHost,
                                  c->cstream2));
        HIP_TRY(c, hipEventRecord(c->pf_out[b], c->cstream2));
        if (j && (rc = finish(j - 1)) != KH_OK) return rc;
    }
    return out ? finish(nch - 1) : KH_OK;
}

ReadPlan read_plan(const kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, u64 n, u64 nout) {
    ReadPlan p;
    const u64 lead = (uintptr_t)d_bases & 15;
    p.abase = d_bases - lead;
    p.vbeg = lead, p.vend = lead + n;
    const bool use_qual = qual_filter(c, d_qual, &p.thr);
    p.qbase = use_qual ? d_qual - lead : nullptr;  // same virtual coordinates as the bases
    p.qaligned = use_qual && (((uintptr_t)p.qbase) & 15) == 0;
    p.ntiles = (p.vbeg + (c->k - 1) + nout + kh::TILE - 1) / kh::TILE;
    u64 blocks = p.ntiles < (u64)grid_cap() ? p.ntiles : (u64)grid_cap();
    p.tpb = (uint32_t)((p.ntiles + blocks - 1) / blocks);
    p.blocks = (unsigned)((p.ntiles + p.tpb - 1) / p.tpb);
    return p;
}

int check_rec_start(kh_ctx *c, const char *who, const u64 *rec_start, u64 nrec, u64 n) {
    const std::string w(who);
    for (u64 r = 0; r < nrec; ++r) {
        if (rec_start[r] > rec_start[r + 1]) return fail(c, KH_ERR_BAD_ARG, (w + ": rec_start is not ascending").c_str());
        if (rec_start[r + 1] - rec_start[r] > 0xFFFFFFFFull) return fail(c, KH_ERR_BAD_ARG, (w + ": a record of 2^32 or more window starts").c_str());
    }
    if (nrec && rec_start[nrec] > n) return fail(c, KH_ERR_BAD_ARG, (w + ": rec_start[nrec] is beyond n").c_str());
    return KH_OK;
}

namespace {

// What profile_records_kernel needs beyond profile_kernel's arguments (see there).
struct RecArgs {
    const u64 *d_rec_start;
    u64 r_lo, r_hi, out0;
    uint32_t lo, hi;
    uint32_t *d_rows;
    int sumw;
};
// the word of a row the 64-bit sum is accumulated at: 8-byte aligned (the device's 64-bit atomic needs it)
int pr_sum_word(const uint32_t *d_rows) { return (((uintptr_t)d_rows) & 7) == 4 ? KH_REC_SUM_LO : KH_REC_SUM_LO + 1; }

// Every window start i < nout of the n device-resident bytes -> d_out[i], or, with rec, into the rows of the records that own
// them; asynchronous on the compute stream.
int profile_range(kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, u64 n, u64 nout, uint32_t *d_out, const RecArgs *rec = nullptr) {
    if (nout == 0) return KH_OK;
    const ReadPlan p = read_plan(c, d_bases, d_qual, n, nout);
    const dim3 grid(p.blocks), block(kh::BLOCK);
    with_probe(c, [&](auto tab) {
        typedef decltype(tab) TAB;
        if (rec && p.qbase)
            hipLaunchKernelGGL((kh::profile_records_kernel<true, TAB>), grid, block, 0, c->stream, p.abase, p.qbase, p.qaligned, p.vbeg, p.vend, p.ntiles,
                               p.tpb, c->k, p.thr, tab, nout, rec->d_rec_start, rec->r_lo, rec->r_hi, rec->out0, rec->lo, rec->hi, rec->d_rows, rec->sumw);
        else if (rec)
            hipLaunchKernelGGL((kh::profile_records_kernel<false, TAB>), grid, block, 0, c->stream, p.abase, p.qbase, p.qaligned, p.vbeg, p.vend, p.ntiles,
                               p.tpb, c->k, p.thr, tab, nout, rec->d_rec_start, rec->r_lo, rec->r_hi, rec->out0, rec->lo, rec->hi, rec->d_rows, rec->sumw);
        else if (p.qbase)
            hipLaunchKernelGGL((kh::profile_kernel<true, TAB>), grid, block, 0, c->stream, p.abase, p.qbase, p.qaligned, p.vbeg, p.vend, p.ntiles, p.tpb,
                               c->k, p.thr, tab, d_out, nout);
        else
            hipLaunchKernelGGL((kh::profile_kernel<false, TAB>), grid, block, 0, c->stream, p.abase, p.qbase, p.qaligned, p.vbeg, p.vend, p.ntiles, p.tpb,
                               c->k, p.thr, tab, d_out, nout);
    });
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}

// Rows of nrec records to the identities of the reductions / from there to what the header promises; on the compute stream.
int records_preset(kh_ctx *c, uint32_t *d_rows, u64 nrec, int sumw) {
    hipLaunchKernelGGL(kh::profile_records_preset, dim3((unsigned)grid_for(nrec * KH_REC_WORDS)), dim3(kh::BLOCK), 0, c->stream, d_rows, nrec, sumw);
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}
int records_finalize(kh_ctx *c, uint32_t *d_rows, u64 nrec, int sumw) {
    hipLaunchKernelGGL(kh::profile_records_finalize, dim3((unsigned)grid_for(nrec)), dim3(kh::BLOCK), 0, c->stream, d_rows, nrec, sumw);
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}

// The device copies of the host form's rows and record offsets: they stay for the whole call (and for the next one).
int records_buffers(kh_ctx *c, u64 nrec) {
    if (c->pr_rows_cap >= nrec && c->pr_rec_cap >= nrec + 1) return KH_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->pr_rows) (void)dev_free(c->pr_rows);
    if (c->pr_rec) (void)dev_free(c->pr_rec);
    c->pr_rows = nullptr;
    c->pr_rec = nullptr;
    c->pr_rows_cap = c->pr_rec_cap = 0;
    hipError_t e = dev_malloc((void **)&c->pr_rows, nrec * KH_REC_WORDS * sizeof(uint32_t));
    if (e == hipSuccess) e = dev_malloc((void **)&c->pr_rec, (nrec + 1) * sizeof(u64));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (c->pr_rows) (void)dev_free(c->pr_rows);
        c->pr_rows = nullptr;
        c->pr_rec = nullptr;
        return soft_oom(c, "kh_profile_records: row buffers", e);  // (a reading call: the context stays usable)
    }
    c->pr_rows_cap = nrec;
    c->pr_rec_cap = nrec + 1;
    return KH_OK;
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_profile_device(kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, uint32_t *d_out) {
    if (!c) return KH_ERR_BAD_ARG;
    if (n && (!d_bases || !d_out)) return fail(c, KH_ERR_BAD_ARG, "kh_profile_device: NULL argument");
    if ((uintptr_t)d_out & 3) return fail(c, KH_ERR_BAD_ARG, "kh_profile_device: d_out is not 4-byte aligned");
    int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (n == 0) return KH_OK;
    rc = profile_range(c, d_bases, d_qual, n, n, d_out);
    if (rc != KH_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (d_out is complete, and the caller's buffers may go)
    return KH_OK;
}

extern "C" int kh_profile(kh_ctx *c, const uint8_t *bases, const uint8_t *qual, uint64_t n, uint32_t *out) {
    if (!c) return KH_ERR_BAD_ARG;
    if (n && (!bases || !out)) return fail(c, KH_ERR_BAD_ARG, "kh_profile: NULL argument");
    if ((uintptr_t)out & 3) return fail(c, KH_ERR_BAD_ARG, "kh_profile: out is not 4-byte aligned");
    int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (n == 0) return KH_OK;
    const u64 chunk = profile_chunk(c, n);
    if ((rc = profile_buffers(c, chunk)) != KH_OK) return rc;
    return chunk_pipeline(c, bases, qual, n, chunk, 0, out, sizeof(uint32_t), [&](const ChunkJob &job) {
        return profile_range(c, job.d_bases, job.d_qual, job.len, job.ns, reinterpret_cast<uint32_t *>(job.d_tail));
    });
}

extern "C" int kh_profile_records_device(kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, const uint64_t *d_rec_start,
                                         uint64_t nrec, uint32_t lo, uint32_t hi, uint32_t *d_rows) {
    if (!c) return KH_ERR_BAD_ARG;
    if ((n && !d_bases) || (nrec && (!d_rec_start || !d_rows))) return fail(c, KH_ERR_BAD_ARG, "kh_profile_records_device: NULL argument");
    if ((uintptr_t)d_rows & 3) return fail(c, KH_ERR_BAD_ARG, "kh_profile_records_device: d_rows is not 4-byte aligned");
    if ((uintptr_t)d_rec_start & 7) return fail(c, KH_ERR_BAD_ARG, "kh_profile_records_device: d_rec_start is not 8-byte aligned");
    int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (nrec == 0) return KH_OK;
    const int sumw = pr_sum_word(d_rows);
    if ((rc = records_preset(c, d_rows, nrec, sumw)) != KH_OK) return rc;
    if (n) {
        const RecArgs ra{reinterpret_cast<const u64 *>(d_rec_start), 0, nrec, 0, lo, hi, d_rows, sumw};
        if ((rc = profile_range(c, d_bases, d_qual, n, n, nullptr, &ra)) != KH_OK) return rc;
    }
    if ((rc = records_finalize(c, d_rows, nrec, sumw)) != KH_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (d_rows is complete, and the caller's buffers may go)
    return KH_OK;
}

extern "C" int kh_profile_records(kh_ctx *c, const uint8_t *bases, const uint8_t *qual, uint64_t n, const uint64_t *rec_start, uint64_t nrec,
                                  uint32_t lo, uint32_t hi, uint32_t *rows) {
    if (!c) return KH_ERR_BAD_ARG;
    if ((n && !bases) || (nrec && (!rec_start || !rows))) return fail(c, KH_ERR_BAD_ARG, "kh_profile_records: NULL argument");
    if ((uintptr_t)rows & 3) return fail(c, KH_ERR_BAD_ARG, "kh_profile_records: rows is not 4-byte aligned");
    if ((uintptr_t)rec_start & 7) return fail(c, KH_ERR_BAD_ARG, "kh_profile_records: rec_start is not 8-byte aligned");
    int rc = check_rec_start(c, "kh_profile_records", reinterpret_cast<const u64 *>(rec_start), nrec, n);  // (before enter(): see kh_unitigs_paths)
    if (rc != KH_OK) return rc;
    if ((rc = enter(c, ENTER_READ)) != KH_OK) return rc;
    if (nrec == 0) return KH_OK;
    if ((rc = records_buffers(c, nrec)) != KH_OK) return rc;
    uint32_t *const d_rows = c->pr_rows;
    const int sumw = pr_sum_word(d_rows);
    HIP_TRY(c, hipMemcpyAsync(c->pr_rec, rec_start, (nrec + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    if ((rc = records_preset(c, d_rows, nrec, sumw)) != KH_OK) return rc;
    if (n) {
        const u64 chunk = profile_chunk(c, n);
        if ((rc = profile_buffers(c, chunk)) != KH_OK) return rc;
        // nothing of a chunk comes back: its kernel adds to the rows
        rc = chunk_pipeline(c, bases, qual, n, chunk, 0, nullptr, 0, [&](const ChunkJob &job) {
            // the records that own a window start of this chunk: those that end behind a and start before a + ns (none: no launch)
            const u64 r_lo = (u64)(std::upper_bound(rec_start + 1, rec_start + nrec + 1, job.a) - (rec_start + 1));
            const u64 r_hi = (u64)(std::lower_bound(rec_start, rec_start + nrec, job.a + job.ns) - rec_start);
            if (r_lo >= r_hi) return (int)KH_OK;
            const RecArgs ra{c->pr_rec, r_lo, r_hi, job.a, lo, hi, d_rows, sumw};
            return profile_range(c, job.d_bases, job.d_qual, job.len, job.ns, nullptr, &ra);
        });
        if (rc != KH_OK) return rc;
    }
    if ((rc = records_finalize(c, d_rows, nrec, sumw)) != KH_OK) return rc;
    return d2h_staged(c, rows, d_rows, nrec * KH_REC_WORDS * sizeof(uint32_t));  // the rows come back once
}
