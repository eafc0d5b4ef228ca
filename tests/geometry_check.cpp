// CPU check of krust_amd/csrc/geom_bits.h (built and run by tests/test_geometry_small_k.py; no GPU, no HIP): the table /
// partition geometry arithmetic every kernel, exchange unit and the 8-byte table image share, held to plain 128-bit integer
// arithmetic written out HERE, for every k = 1..32 and region counts on both sides of the 10-bit level-1 digit -- among them
// the geometries small k alone reaches: 2k <= p1_bits (no payload bits at all: every x is 0), 2k < p1_bits + 32 (the low
// bits of every x are zero and the exchange units keep their count there) and kh_x_zero_bits at its clamp.
//
// Keys: all 4^k of them for k <= 10, 2^20 distinct random ones (the extremes among them) otherwise.  Per (k, regions) one line
//   GEOM k=<k> regions=<n> keys=<m> OK | FAIL <count>
// on stdout; the first failures of each geometry in words on stderr.  Exit status 1 if anything failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../krust_amd/csrc/geom_bits.h"

typedef unsigned __int128 u128;
typedef uint64_t u64;

static const u64 REGION_COUNTS[] = {1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024,
                                    1024ull * 2, 1024ull * 3, 1024ull * 5, 1024ull * 24, 1024ull * 40, 1024ull * 100,
                                    1024ull * 160, 1024ull * 640, 1024ull * 800, 1024ull * 1024};

static std::mutex out_mutex;
static int total_failures = 0;

static uint32_t floor_log2_ref(u64 v) {
    uint32_t b = 0;
    while ((v >> (b + 1)) != 0) ++b;
    return b;
}

struct Fail {
    int n = 0;
    std::string text;
    void add(int k, u64 regions, u64 key, const char *what, u128 got, u128 want) {
        if (n++ < 5) {
            char buf[256];
            snprintf(buf, sizeof buf, "  k=%d regions=%llu key=%llx: %s: got %llx want %llx\n", k, (unsigned long long)regions,
                     (unsigned long long)key, what, (unsigned long long)got, (unsigned long long)want);
            text += buf;
        }
    }
};

static void check_geometry(int k, u64 regions, const std::vector<std::pair<u64, u64>> &hk /* (H, key), ascending H */) {
    Fail f;
    const kh::RegionGeom g = kh::kh_geom_of_regions(regions);
    // the geometry of a region count: p1_bits + log2 b2 bits of region index, a 10-bit digit beyond 1024 regions
    const uint32_t p1_want = regions <= 1024 ? floor_log2_ref(regions) : 10u;
    const u64 b2_want = regions >> p1_want;
    if (g.p1_bits != p1_want || g.b2 != b2_want || kh::kh_regions_of(g) != regions || !kh::kh_regions_valid(regions))
        f.add(k, regions, 0, "kh_geom_of_regions", ((u128)g.p1_bits << 32) | g.b2, ((u128)p1_want << 32) | b2_want);
    const uint32_t p1b = p1_want;
    const u64 b2 = b2_want;
    const uint32_t lg = floor_log2_ref(b2), w = 32 - lg;
    // zero bits at the low end of every x: x is hash bits [p1b, p1b + 32) of a hash of 2k bits
    const int ztrue = std::min(32, std::max(0, (int)p1b + 32 - 2 * k));
    const uint32_t zs = kh::kh_x_zero_bits((uint32_t)k, g.p1_bits);
    if (zs != (uint32_t)std::min(ztrue, 31)) f.add(k, regions, 0, "kh_x_zero_bits", zs, std::min(ztrue, 31));
    const u128 zmask = ((u128)1 << ztrue) - 1;
    const int hb_want = 2 * k - (int)p1b - (int)lg;
    if (kh::kh_below_bits((uint32_t)k, 0, g) != hb_want) f.add(k, regions, 0, "kh_below_bits", (u128)(int64_t)kh::kh_below_bits((uint32_t)k, 0, g), (u128)(int64_t)hb_want);
    // the window (region, below) covers the top p1b + 32 + (32 - w) bits of H: the whole hash when hb_want <= 32
    const uint32_t covered = p1b + 32 + lg;
    const u64 cover_mask = covered >= 64 ? ~0ull : ~0ull << (64 - covered);

    u64 prev_region = 0, prev_below = 0;
    bool have_prev = false;
    for (const auto &e : hk) {
        const u64 H = e.first, key = e.second;
        // ---- the reference, in 128-bit arithmetic ----
        const u64 p1 = p1b ? H >> (64 - p1b) : 0;
        const u64 x = (u64)((((u128)H << p1b) & (((u128)1 << 64) - 1)) >> 32);
        const u64 bucket = (u64)(((u128)x * b2) >> 32);
        const u64 region = p1 * b2 + bucket;
        u128 xlo = (((u128)bucket << 32) + b2 - 1) / b2;        // smallest x of the bucket ...
        xlo = (xlo + zmask) & ~zmask;                             // ... that a k-mer's hash can take
        const u128 xoff = (u128)x - xlo;                          // (wraps to a huge value if xlo > x)
        const u64 behind = lg ? (u64)((((u128)H << (p1b + 32)) & (((u128)1 << 64) - 1)) >> (64 - lg)) : 0;  // the lg hash bits behind x
        const u64 below = (u64)((xoff << lg) | behind);
        const uint32_t start = (uint32_t)((((u128)x * b2) & 0xFFFFFFFFull) >> (32 - kh::REGION_BITS)) & kh::REGION_START_MASK;

        // ---- the shared functions ----
        const uint32_t gx = kh::kh_x_of(H, g.p1_bits), gp1 = kh::kh_p1_of(H, g.p1_bits), gb = kh::kh_bucket_of_x(gx, g.b2);
        if (gx != x) f.add(k, regions, key, "kh_x_of", gx, x);
        if (gp1 != p1) f.add(k, regions, key, "kh_p1_of", gp1, p1);
        if (gb != bucket) f.add(k, regions, key, "kh_bucket_of_x", gb, bucket);
        const u64 gregion = (u64)gp1 * g.b2 + gb;
        if (gregion >= regions || gregion != region) f.add(k, regions, key, "region", gregion, region);
        if (have_prev && gregion < prev_region) f.add(k, regions, key, "region not monotone in H", gregion, prev_region);
        if (kh::kh_start_of_x(gx, g.b2) != start || start >= kh::REGION_SLOTS) f.add(k, regions, key, "kh_start_of_x", kh::kh_start_of_x(gx, g.b2), start);
        const uint32_t gxlo = kh::kh_xlo_k(gb, g.b2, zs);
        if ((u128)gxlo != xlo) f.add(k, regions, key, "kh_xlo_k", gxlo, xlo);
        if (xoff >> w) f.add(k, regions, key, "x - xlo_k does not fit the window", xoff, (u128)1 << w);
        if (((u128)(uint32_t)(gx - gxlo) & zmask) != 0) f.add(k, regions, key, "low zero bits of x - xlo_k", (uint32_t)(gx - gxlo), 0);
        const uint32_t gbelow = kh::kh_below_region(H, g, (uint32_t)k);
        if (gbelow != below) f.add(k, regions, key, "kh_below_region", gbelow, below);
        const u64 back = kh::kh_hash_of_below(gregion, gbelow, g, (uint32_t)k);
        if (back != (H & cover_mask)) f.add(k, regions, key, "kh_hash_of_below(region, kh_below_region(H))", back, H & cover_mask);
        if (hb_want <= 32 && back != H) f.add(k, regions, key, "round trip loses hash bits although kh_below_bits <= 32", back, H);
        // keys of one region: distinct below words (ascending with H, so neighbours suffice) wherever the window holds the whole hash
        if (hb_want <= 32 && have_prev && gregion == prev_region && gbelow <= prev_below)
            f.add(k, regions, key, "two keys of one region share a below word", gbelow, prev_below);
        prev_region = gregion;
        prev_below = gbelow;
        have_prev = true;
    }
    std::lock_guard<std::mutex> lock(out_mutex);
    if (f.n) {
        printf("GEOM k=%d regions=%llu keys=%zu FAIL %d\n", k, (unsigned long long)regions, hk.size(), f.n);
        fputs(f.text.c_str(), stderr);
        total_failures += f.n;
    } else {
        printf("GEOM k=%d regions=%llu keys=%zu OK\n", k, (unsigned long long)regions, hk.size());
    }
}

static void check_k(int k) {
    const u64 kmask = kh_kmask((uint32_t)k);
    std::vector<std::pair<u64, u64>> hk;
    if (k <= 10) {   // (4^10 = 2^20: the whole key space there too)
        for (u64 key = 0; key <= kmask; ++key) hk.push_back({kh_table_hash(key, (uint32_t)k), key});
    } else {
        u64 s = 0x9E3779B97F4A7C15ull * (u64)(k + 1);
        std::vector<u64> keys = {0, kmask, 1, 1ull << (2 * k - 1), kmask >> 1};
        while (keys.size() < (1u << 20)) {   // 2^20 DISTINCT keys
            while (keys.size() < (1u << 20)) keys.push_back((s = kh_mix64(s + 0x632BE59BD9B4E019ull)) & kmask);
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        }
        for (u64 key : keys) hk.push_back({kh_table_hash(key, (uint32_t)k), key});
    }
    std::sort(hk.begin(), hk.end());
    // the hash is a bijection of the 2k-bit keys, left-aligned: distinct keys, distinct H, nothing below bit 64 - 2k
    Fail f;
    for (size_t i = 0; i < hk.size(); ++i) {
        if (i && hk[i].first == hk[i - 1].first) f.add(k, 0, hk[i].second, "two keys share a hash", hk[i].first, hk[i - 1].first);
        if (k < 32 && (hk[i].first & ((1ull << (64 - 2 * k)) - 1))) f.add(k, 0, hk[i].second, "hash not left-aligned", hk[i].first, 0);
        if (kh_table_unhash(hk[i].first, (uint32_t)k) != hk[i].second) f.add(k, 0, hk[i].second, "kh_table_unhash", kh_table_unhash(hk[i].first, (uint32_t)k), hk[i].second);
    }
    if (f.n) {
        std::lock_guard<std::mutex> lock(out_mutex);
        printf("HASH k=%d FAIL %d\n", k, f.n);
        fputs(f.text.c_str(), stderr);
        total_failures += f.n;
    }
    for (u64 regions : REGION_COUNTS) check_geometry(k, regions, hk);
}

int main(int argc, char **argv) {
    const int nthreads = argc > 1 ? std::max(1, atoi(argv[1])) : 4;
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; ++t)
        pool.emplace_back([t, nthreads] {
            for (int k = 32 - t; k >= 1; k -= nthreads) check_k(k);   // (largest key sets first)
        });
    for (auto &th : pool) th.join();
    if (total_failures) {
        fprintf(stderr, "%d failures\n", total_failures);
        return 1;
    }
    printf("GEOMETRY_OK 32 x %zu\n", sizeof REGION_COUNTS / sizeof REGION_COUNTS[0]);
    return 0;
}
