// sort.hip -- kh_result_sorted*: the table's (key, count) pairs in ascending key order, sorted ON THE DEVICE (sort.hip.h).
//
// The pairs are compacted as kh_result_copy_device compacts them, then sorted by ceil(2k / 8) radix passes that ping-pong between
// two pairs of arrays; the compaction goes to the pair from which the last pass lands in the caller's arrays.
// Scratch -- the second pair, the [digit][tile] histogram (u32) and its scan (u64) -- is the call's (ctx.hip.h, CallScratch::take):
// everything goes back at the end of the call, and running out of memory leaves the context usable (KH_ERR_OOM without
// poisoning it).
#include "ctx.hip.h"
#include "sort.hip.h"

namespace khi {

// The n pairs with count >= min_count (n = kh_result_size: the caller has taken it) into out_keys / out_counts (device, n
// entries each), ascending by key.  Asynchronous on the compute stream.
int sorted_into(kh_ctx *c, u64 *out_keys, u64 *out_counts, u64 n, u64 min_count, CallScratch &sc) {
    if (n == 0) return KH_OK;
    const u64 ntiles = (n + kh::SORT_TILE - 1) / kh::SORT_TILE;
    const u64 nhist = ntiles * kh::SORT_BINS;
    u64 *const tk = (u64 *)sc.take(n * sizeof(u64));
    u64 *const tc = (u64 *)sc.take(n * sizeof(u64));
    uint32_t *const hist = (uint32_t *)sc.take(nhist * sizeof(uint32_t));
    u64 *const start = (u64 *)sc.take((nhist + 1) * sizeof(u64));
    u64 *const scan = (u64 *)sc.take(device_scan_scratch(nhist));  // (not the context's: nothing of this call stays allocated)
    if (!tk || !tc || !hist || !start || !scan) return soft_oom(c, "device memory for the sort's scratch");
    const uint32_t passes = kh::sort_passes(c->k);
    u64 *k0 = (passes & 1u) ? tk : out_keys, *c0 = (passes & 1u) ? tc : out_counts;  // an odd number of passes ends in the other pair
    u64 *k1 = (passes & 1u) ? out_keys : tk, *c1 = (passes & 1u) ? out_counts : tc;
    u64 got = 0;
    int rc = compact_pairs(c, k0, c0, n, min_count, &got);
    if (rc != KH_OK) return rc;
    if (got != n) return fail(c, KH_ERR_STATE, "the table changed between the size and the copy of a sorted result");
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t shift = kh::sort_pass_shift(c->k, p), mask = (1u << kh::sort_pass_bits(c->k, p)) - 1u;
        for (u64 s = 0; s < ntiles;) {  // (a grid dimension holds 2^31 - 1 workgroups)
            const u64 m = std::min<u64>(ntiles - s, 1ull << 30);
            hipLaunchKernelGGL(kh::sort_hist_kernel, dim3((unsigned)m), dim3(kh::BLOCK), 0, c->stream, (const u64 *)k0, n, shift, mask, s,
                               ntiles, hist);
            s += m;
        }
        HIP_TRY(c, hipGetLastError());
        if ((rc = device_scan(c, hist, nhist, start, true, scan)) != KH_OK) return rc;
        for (u64 s = 0; s < ntiles;) {
            const u64 m = std::min<u64>(ntiles - s, 1ull << 30);
            hipLaunchKernelGGL(kh::sort_scatter_kernel, dim3((unsigned)m), dim3(kh::BLOCK), 0, c->stream, (const u64 *)k0, (const u64 *)c0,
                               n, shift, mask, s, ntiles, (const u64 *)start, k1, c1);
            s += m;
        }
        HIP_TRY(c, hipGetLastError());
        std::swap(k0, k1);
        std::swap(c0, c1);
    }
    return KH_OK;
}

}  // namespace khi
using namespace khi;

extern "C" int kh_result_sorted_device(kh_ctx *c, uint64_t *d_keys, uint64_t *d_counts, uint64_t cap, uint64_t min_count, uint64_t *n) {
    uint64_t need = 0;
    int rc = result_enter(c, d_keys, d_counts, cap, min_count, n, &need);
    if (rc != KH_OK || need == 0) return rc;
    {
        CallScratch sc(c);
        rc = sorted_into(c, (u64 *)d_keys, (u64 *)d_counts, need, min_count, sc);
        if (rc == KH_OK) HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (rc == KH_OK) *n = need;
    return rc;
}

extern "C" int kh_result_sorted(kh_ctx *c, uint64_t *keys, uint64_t *counts, uint64_t cap, uint64_t min_count, uint64_t *n) {
    uint64_t need = 0;
    int rc = result_enter(c, keys, counts, cap, min_count, n, &need);
    if (rc != KH_OK || need == 0) return rc;
    CallScratch sc(c);
    u64 *const dk = (u64 *)sc.take(need * sizeof(u64));
    u64 *const dc = (u64 *)sc.take(need * sizeof(u64));
    if (!dk || !dc) return soft_oom(c, "device memory for the sorted result");
    rc = sorted_into(c, dk, dc, need, min_count, sc);
    if (rc == KH_OK) rc = d2h_staged(c, keys, dk, need * sizeof(u64));
    if (rc == KH_OK) rc = d2h_staged(c, counts, dc, need * sizeof(u64));
    if (rc == KH_OK) *n = need;
    return rc;
}
