// sort.hip -- kh_result_sorted*: the table's (key, count) pairs in ascending key order, sorted ON THE DEVICE (sort.hip.h).
//
// The pairs are compacted as kh_result_copy_device compacts them, then sorted by ceil(2k / 8) radix passes that ping-pong between
// two pairs of arrays; the compaction goes to the pair from which the last pass lands in the caller's arrays.
// Scratch -- the second pair, the [digit][tile] histogram (u32) and its scan (u64) -- is taken as kh_result_copy takes its two
// arrays: the idle partition buffers when nothing is borrowed, else borrow(), else hipMalloc; everything goes back at the end
// of the call, and running out of memory leaves the context usable (KH_ERR_OOM without poisoning it).
#include "ctx.hip.h"
#include "sort.hip.h"

namespace khi {

SortScratch::SortScratch(kh_ctx *ctx) : c(ctx), loan0(ctx->borrow_off[0]), loan1(ctx->borrow_off[1]) {}

void *SortScratch::take(u64 bytes) {
    const u64 need = (std::max<u64>(bytes, 16) + 4095) & ~4095ull;
    if (!c->borrow_on) {  // the partition buffers are idle: every batch is counted (enter() flushed)
        uint8_t *const base[2] = {c->keysA, c->keysB};
        const u64 cap[2] = {c->key_cap, c->keyb_cap};
        for (int i = 0; i < 2; ++i)
            if (base[i] && used[i] + need <= cap[i]) {
                void *p = base[i] + used[i];
                used[i] += need;
                return p;
            }
    } else if (void *p = borrow(c, need)) {
        return p;
    }
    void *p = nullptr;
    if (dev_malloc(&p, need) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    try {
        owned.push_back(p);
    } catch (...) {
        (void)dev_free(p);
        return nullptr;
    }
    return p;
}

SortScratch::~SortScratch() {
    if (!owned.empty()) (void)hipStreamSynchronize(c->stream);
    for (void *p : owned) (void)dev_free(p);
    c->borrow_off[0] = loan0;  // (a loan taken for this call alone goes back)
    c->borrow_off[1] = loan1;
}

// The n pairs with count >= min_count (n = kh_result_size: the caller has taken it) into out_keys / out_counts (device, n
// entries each), ascending by key.  Asynchronous on the compute stream.
int sorted_into(kh_ctx *c, u64 *out_keys, u64 *out_counts, u64 n, u64 min_count, SortScratch &sc) {
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
    int rc = enter(c, true, true, false, true);
    if (rc != KH_OK) return rc;
    if (!n || (cap && (!d_keys || !d_counts))) return fail(c, KH_ERR_BAD_ARG, "NULL output");
    *n = 0;
    uint64_t need = 0;
    if ((rc = kh_result_size(c, min_count, &need)) != KH_OK) return rc;
    if (need > cap) return fail(c, KH_ERR_RANGE, "output arrays too small");
    if (need == 0) return KH_OK;
    {
        SortScratch sc(c);
        rc = sorted_into(c, (u64 *)d_keys, (u64 *)d_counts, need, min_count, sc);
        if (rc == KH_OK) HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (rc == KH_OK) *n = need;
    return rc;
}

extern "C" int kh_result_sorted(kh_ctx *c, uint64_t *keys, uint64_t *counts, uint64_t cap, uint64_t min_count, uint64_t *n) {
    int rc = enter(c, true, true, false, true);
    if (rc != KH_OK) return rc;
    if (!n || (cap && (!keys || !counts))) return fail(c, KH_ERR_BAD_ARG, "NULL output");
    *n = 0;
    uint64_t need = 0;
    if ((rc = kh_result_size(c, min_count, &need)) != KH_OK) return rc;
    if (need > cap) return fail(c, KH_ERR_RANGE, "output arrays too small");
    if (need == 0) return KH_OK;
    SortScratch sc(c);
    u64 *const dk = (u64 *)sc.take(need * sizeof(u64));
    u64 *const dc = (u64 *)sc.take(need * sizeof(u64));
    if (!dk || !dc) return soft_oom(c, "device memory for the sorted result");
    rc = sorted_into(c, dk, dc, need, min_count, sc);
    if (rc == KH_OK) rc = d2h_staged(c, keys, dk, need * sizeof(u64));
    if (rc == KH_OK) rc = d2h_staged(c, counts, dc, need * sizeof(u64));
    if (rc == KH_OK) *n = need;
    return rc;
}
