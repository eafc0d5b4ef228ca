// sort.hip.h -- LSD radix sort of (packed key, count) pairs by key: the pass plan (host and device) and the two kernels of a pass.
//
// Keys are distinct and below 4^k, so only the 2k significant bits are sorted: ceil(2k / 8) passes of one 8-bit digit each, from
// bit 0 upwards; the last pass takes what is left (2k mod 8 bits when that is not 0).  Ascending packed keys are the k-mer
// strings in lexicographic order (A < C < G < T, first base most significant).
//
// One pass is three launches -- no workgroup ever waits for another:
//   sort_hist_kernel     per tile of SORT_TILE pairs: how many keys carry each digit value  -> hist[digit][tile] (u32)
//   device_scan          exclusive scan of that table, digit-major: where every (digit, tile) run starts in the output
//   sort_scatter_kernel  per tile: every pair to  start[digit][tile] + its rank among the tile's earlier pairs of that digit
// The rank comes from wave ballots (which lanes of the wave hold my digit: 8 ballots, one per digit bit) plus one counter per
// (wave, digit) in LDS that only its own wave touches; the waves' counters are then prefixed in wave order.  No atomic decides
// where a pair lands: every pass is stable and the same input gives the same output on every run.
// Traffic of a pass: the histogram reads the keys (8 B x n), the scatter reads and writes the pairs (2 x 16 B x n).
// Measured once on one MI355X (profiles/README.md r11; k = 21: 6 passes): 365.1 M pairs sorted in 55.0 ms beside 3.1 ms for the
// unsorted compaction -- 8.65 ms per pass, 1.35 TB/s of 2 x 16 B x n; 105.1 M pairs: 16.1 ms, 2.49 ms per pass, the same rate.
// kh_result_copy and a sort on 16 host cores: 9.7 s and 2.85 s.
#pragma once
#include <stdint.h>

#include "kmer_bits.h"

namespace kh {

constexpr uint32_t SORT_DIGIT_BITS = 8;

KH_HD uint32_t sort_passes(uint32_t k) { return (2u * k + SORT_DIGIT_BITS - 1u) / SORT_DIGIT_BITS; }
// pass p (0 <= p < sort_passes(k)) sorts by bits [shift, shift + bits) of the key
KH_HD uint32_t sort_pass_shift(uint32_t /*k*/, uint32_t p) { return SORT_DIGIT_BITS * p; }
KH_HD uint32_t sort_pass_bits(uint32_t k, uint32_t p) {
    const uint32_t left = 2u * k - SORT_DIGIT_BITS * p;
    return left < SORT_DIGIT_BITS ? left : SORT_DIGIT_BITS;
}

}  // namespace kh

#if defined(__HIPCC__) && !defined(KH_SORT_HOST_ONLY)
#include "kernels.hip.h"

namespace kh {

constexpr int SORT_PER = 16;                 // pairs per lane
constexpr int SORT_TILE = BLOCK * SORT_PER;  // 4096 pairs per workgroup: wave w takes pairs [w * 1024, (w + 1) * 1024) of the tile,
                                             // lane l of it the pairs j * 64 + l -- so (wave, j, lane) is the pairs' order
constexpr int SORT_BINS = 1 << SORT_DIGIT_BITS;

// Rank of this lane's pair among the pairs of digit d that its wave has seen so far (earlier steps, then lower lanes), and the
// wave's counter moved on.  cnt: the wave's own SORT_BINS counters.  Every lane of the wave calls it (the ballots are wave-wide).
__device__ __forceinline__ uint32_t sort_wave_rank(volatile uint32_t *cnt, uint32_t d, bool valid) {
    u64 peers = kh_ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < SORT_DIGIT_BITS; ++b) {
        const bool bit = (d >> b) & 1u;
        const u64 m = kh_ballot(bit);
        peers &= bit ? m : ~m;
    }
    const uint32_t below = mbcnt(peers);  // valid lanes below this one with the same digit
    uint32_t r = 0;
    if (valid) r = cnt[d] + below;
    __builtin_amdgcn_wave_barrier();  // (every lane has read before the lowest lane of each digit writes)
    if (valid && below == 0) cnt[d] = r + (uint32_t)__builtin_popcountll(peers);
    __builtin_amdgcn_wave_barrier();
    return r;
}

// hist[d * ntiles + t] = keys of tile t whose digit is d.  One workgroup per tile tile0 + blockIdx.x.
// kernel-resource-usage (gfx950, hipcc -O3): 40 VGPRs, 52 SGPRs, 4096 B LDS, no scratch, no spills, 8 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void sort_hist_kernel(const u64 *__restrict__ keys, u64 n, uint32_t shift, uint32_t mask, u64 tile0,
                                                          u64 ntiles, uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_cnt[BLOCK / 64][SORT_BINS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const u64 t = tile0 + blockIdx.x;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) s_cnt[w][tid] = 0;
    __syncthreads();
    const u64 wbase = t * (u64)SORT_TILE + (u64)wave * (SORT_TILE / (BLOCK / 64));
    u64 key[SORT_PER];
#pragma unroll
    for (int j = 0; j < SORT_PER; ++j) {  // (all loads first: the ranking below is a chain of LDS round trips)
        const u64 i = wbase + (u64)j * 64 + lane;
        key[j] = i < n ? keys[i] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < SORT_PER; ++j)
        (void)sort_wave_rank(s_cnt[wave], (uint32_t)(key[j] >> shift) & mask, wbase + (u64)j * 64 + lane < n);
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) sum += s_cnt[w][tid];
    hist[(u64)tid * ntiles + t] = sum;
}

// start[d * ntiles + t]: the exclusive scan of hist.  Pair i of tile t goes to start[d][t] + (pairs of digit d in earlier waves of
// the tile) + its rank in its wave.
// kernel-resource-usage (gfx950, hipcc -O3): 120 VGPRs (16 keys, 16 ranks and the counts' loads in flight), 56 SGPRs, 6144 B LDS, no
// scratch, no spills, 4 waves per SIMD.
KH_GLOBAL __launch_bounds__(BLOCK) void sort_scatter_kernel(const u64 *__restrict__ keys_in, const u64 *__restrict__ counts_in, u64 n,
                                                             uint32_t shift, uint32_t mask, u64 tile0, u64 ntiles,
                                                             const u64 *__restrict__ start, u64 *__restrict__ keys_out,
                                                             u64 *__restrict__ counts_out) {
    __shared__ uint32_t s_cnt[BLOCK / 64][SORT_BINS];
    __shared__ u64 s_start[SORT_BINS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const u64 t = tile0 + blockIdx.x;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) s_cnt[w][tid] = 0;
    __syncthreads();
    const u64 wbase = t * (u64)SORT_TILE + (u64)wave * (SORT_TILE / (BLOCK / 64));
    u64 key[SORT_PER];
    uint32_t rank[SORT_PER];
#pragma unroll
    for (int j = 0; j < SORT_PER; ++j) {
        const u64 i = wbase + (u64)j * 64 + lane;
        key[j] = i < n ? keys_in[i] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < SORT_PER; ++j)
        rank[j] = sort_wave_rank(s_cnt[wave], (uint32_t)(key[j] >> shift) & mask, wbase + (u64)j * 64 + lane < n);
    __syncthreads();
    {  // thread tid owns digit tid: the waves' totals become the waves' bases
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            const uint32_t x = s_cnt[w][tid];
            s_cnt[w][tid] = run;
            run += x;
        }
        s_start[tid] = start[(u64)tid * ntiles + t];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SORT_PER; ++j) {
        const u64 i = wbase + (u64)j * 64 + lane;
        if (i < n) {
            const uint32_t d = (uint32_t)(key[j] >> shift) & mask;
            const u64 o = s_start[d] + s_cnt[wave][d] + rank[j];
            if (o < n) {  // (always, while hist and start describe this input: a guard, not a path)
                keys_out[o] = key[j];
                counts_out[o] = counts_in[i];
            }
        }
    }
}

}  // namespace kh
#endif
