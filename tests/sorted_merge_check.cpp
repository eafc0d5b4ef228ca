// sorted_merge_check.cpp -- the host half of `kmerust --sorted` (krust_amd/host/kmerust_host.h: merge_sorted, sort_pairs): the N-way
// merge of the ranks' ascending, disjoint lists, and the kh_result_copy + host sort fallback, which must give the same PackedCounts.
// Pure host code: compiled and run by tests/test_sorted_host.py, no device and no library needed.
#include <cstdio>
#include <random>

#include "../krust_amd/host/kmerust_host.h"

using kmerust::PackedCounts;

static int failures = 0;
static uint64_t count_of(uint64_t key) { return (key * 0x9E3779B97F4A7C15ull >> 40) + 1; }  // a count that belongs to its key

// `keys` (distinct) dealt to n lists by `owner`, every list ascending; merged; compared with the plain sort of all pairs.
static void check(const char *name, std::vector<uint64_t> keys, size_t n, const std::function<size_t(size_t, uint64_t)> &owner) {
    std::sort(keys.begin(), keys.end());
    std::vector<PackedCounts> lists(n);
    for (size_t i = 0; i < keys.size(); ++i) {
        PackedCounts &l = lists[owner(i, keys[i]) % n];
        l.keys.push_back(keys[i]);
        l.counts.push_back(count_of(keys[i]));
    }
    const PackedCounts merged = kmerust::merge_sorted(31, lists);
    bool ok = merged.k == 31 && merged.keys == keys && merged.counts.size() == keys.size();
    for (size_t i = 0; ok && i < keys.size(); ++i) ok = merged.counts[i] == count_of(merged.keys[i]);
    // the fallback: the same pairs in any order (as kh_result_copy gives them), sorted on the host
    PackedCounts any;
    any.k = 31;
    for (size_t i = n; i-- > 0;) {
        any.keys.insert(any.keys.end(), lists[i].keys.rbegin(), lists[i].keys.rend());
        any.counts.insert(any.counts.end(), lists[i].counts.rbegin(), lists[i].counts.rend());
    }
    std::mt19937_64 rng(n * 1000 + keys.size());
    for (size_t i = any.keys.size(); i > 1; --i) {
        const size_t j = rng() % i;
        std::swap(any.keys[i - 1], any.keys[j]);
        std::swap(any.counts[i - 1], any.counts[j]);
    }
    kmerust::sort_pairs(any);
    ok = ok && any.keys == merged.keys && any.counts == merged.counts;
    if (!ok) {
        printf("FAIL %s: n=%zu, %zu keys\n", name, n, keys.size());
        ++failures;
    }
}

int main() {
    std::mt19937_64 rng(20260207);
    const size_t ns[] = {1, 2, 3, 8};
    for (size_t n : ns) {
        std::vector<uint64_t> keys;
        for (int i = 0; i < 5000; ++i) keys.push_back(rng() >> 2);
        for (int i = 0; i < 200; ++i) keys.push_back(rng() | (1ull << 63));  // top bit set (k = 32 keys that start with G or T)
        keys.push_back(0);
        keys.push_back(~0ull - 1);
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        check("round robin", keys, n, [](size_t i, uint64_t) { return i; });
        check("by hash", keys, n, [](size_t, uint64_t k) { return (size_t)(k * 0xD6E8FEB86659FD93ull >> 61); });
        check("all in the last list, the others empty", keys, n, [n](size_t, uint64_t) { return n - 1; });
        check("by range", keys, n, [n](size_t, uint64_t k) { return (size_t)((k >> 32) * n >> 32); });
        check("one element per list", std::vector<uint64_t>(keys.begin(), keys.begin() + n), n, [](size_t i, uint64_t) { return i; });
        check("one element, the other lists empty", {1ull << 63}, n, [](size_t, uint64_t) { return (size_t)0; });
        check("no element at all", {}, n, [](size_t, uint64_t) { return (size_t)0; });
    }
    if (failures) return 1;
    printf("sorted_merge_check ok\n");
    return 0;
}
