// unitigs_check.cpp -- the host side of `kmerust unitigs` (krust_amd/host/kmerust_host.h: unitig_header, unitig_summary) on hand-made
// rows.  Pure host code with its own main: compiled and run by tests/test_unitigs_host.py (once more with
// -fsanitize=address,undefined), no device and no library needed.
#include <cstdio>
#include <string>
#include <vector>

#include "../krust_amd/host/kmerust_host.h"

static int failures = 0;
static void expect_u(const char *what, uint64_t got, uint64_t want) {
    if (got != want) {
        printf("FAIL %s: got %llu, want %llu\n", what, (unsigned long long)got, (unsigned long long)want);
        ++failures;
    }
}
static void expect_s(const char *what, const std::string &got, const std::string &want) {
    if (got != want) {
        printf("FAIL %s: got '%s', want '%s'\n", what, got.c_str(), want.c_str());
        ++failures;
    }
}
// rows of unitigs with these k-mer counts L, each with count sum 2 L, START the running sum
static std::vector<uint64_t> rows_of(const std::vector<uint64_t> &L, uint32_t k, uint64_t circular_mask = 0) {
    std::vector<uint64_t> r;
    uint64_t start = 0;
    for (size_t i = 0; i < L.size(); ++i) {
        r.push_back(start);
        r.push_back(L[i]);
        r.push_back(2 * L[i]);
        r.push_back(i < 64 ? (circular_mask >> i) & 1u : 0u);
        start += L[i] + k - 1;
    }
    return r;
}
static kmerust::UnitigSummary sum_of(const std::vector<uint64_t> &L, uint32_t k, uint64_t circ = 0) {
    const std::vector<uint64_t> r = rows_of(L, k, circ);
    return kmerust::unitig_summary(r.data(), L.size(), k);
}

int main() {
    // headers
    {
        const uint64_t a[KH_UNI_WORDS] = {0, 10, 25, 0};
        expect_s("plain header", kmerust::unitig_header(0, a, 21), ">0 LN:i:30 KC:i:25 km:f:2.5");
        const uint64_t b[KH_UNI_WORDS] = {30, 3, 3, KH_UNI_CIRCULAR};
        expect_s("circular header", kmerust::unitig_header(7, b, 31), ">7 LN:i:33 KC:i:3 km:f:1.0 CR:i:1");
        const uint64_t c[KH_UNI_WORDS] = {0, 1, 18446744073709551615ull, 0};  // COUNT_SUM at 2^64 - 1: printed whole, no sign
        expect_s("count sum 2^64 - 1", kmerust::unitig_header(18446744073709551615ull, c, 1),
                 ">18446744073709551615 LN:i:1 KC:i:18446744073709551615 km:f:18446744073709551616.0");
        const uint64_t d[KH_UNI_WORDS] = {0, 3, 18446744073709551614ull, 0};
        // (2^64 as a double, over 3: 0x5555555555555555.55.., and doubles of that size are multiples of 1024: 0x5555555555555400)
        expect_s("count sum near 2^64 over L", kmerust::unitig_header(1, d, 32), ">1 LN:i:34 KC:i:18446744073709551614 km:f:6148914691236516864.0");
        const uint64_t e[KH_UNI_WORDS] = {0, 3, 4, 0};
        expect_s("rounding to one decimal", kmerust::unitig_header(2, e, 5), ">2 LN:i:7 KC:i:4 km:f:1.3");
        const uint64_t f[KH_UNI_WORDS] = {0, 0, 0, 0};  // (no such row comes from the library: no division by zero all the same)
        expect_s("L = 0", kmerust::unitig_header(3, f, 5), ">3 LN:i:4 KC:i:0 km:f:0.0");
    }
    // summary: empty
    {
        const kmerust::UnitigSummary u = kmerust::unitig_summary(nullptr, 0, 21);
        expect_u("empty unitigs", u.unitigs, 0);
        expect_u("empty kmers", u.kmers, 0);
        expect_u("empty bases", u.bases, 0);
        expect_u("empty circular", u.circular, 0);
        expect_u("empty longest", u.longest, 0);
        expect_u("empty n50", u.n50, 0);
    }
    // one unitig
    {
        const kmerust::UnitigSummary u = sum_of({100}, 21, 1);
        expect_u("one unitigs", u.unitigs, 1);
        expect_u("one kmers", u.kmers, 100);
        expect_u("one bases", u.bases, 120);
        expect_u("one circular", u.circular, 1);
        expect_u("one longest", u.longest, 120);
        expect_u("one n50", u.n50, 120);
    }
    // k = 1: bases = kmers; lengths 2, 3, 4, 5, 6 (20 bases): 6 + 5 = 11 >= 10 -> n50 = 5
    {
        const kmerust::UnitigSummary u = sum_of({4, 2, 6, 3, 5}, 1, 0b10100);
        expect_u("k1 bases", u.bases, 20);
        expect_u("k1 kmers", u.kmers, 20);
        expect_u("k1 longest", u.longest, 6);
        expect_u("k1 n50", u.n50, 5);
        expect_u("k1 circular", u.circular, 2);
    }
    // exactly half: lengths 10, 10 -> the first 10 holds half: n50 = 10; lengths 6, 4 (k = 1) -> 6 >= 5: n50 = 6; 5, 5, 5, 5 -> 5
    expect_u("tie two", sum_of({10, 10}, 1).n50, 10);
    expect_u("six four", sum_of({6, 4}, 1).n50, 6);
    expect_u("ties four", sum_of({5, 5, 5, 5}, 1).n50, 5);
    // exactly half is reached by the second: 5, 3, 2 (10 bases): 5 >= 5 -> 5; 4, 3, 3: 4 < 5, 7 >= 5 -> 3
    expect_u("half at first", sum_of({2, 5, 3}, 1).n50, 5);
    expect_u("half at second", sum_of({3, 4, 3}, 1).n50, 3);
    // k enters the lengths: L = 1, 1, 1, 30 at k = 31: bases 31, 31, 31, 60 = 153; 60 < 76.5, 91 >= 76.5 -> 31
    {
        const kmerust::UnitigSummary u = sum_of({1, 30, 1, 1}, 31);
        expect_u("k31 bases", u.bases, 153);
        expect_u("k31 kmers", u.kmers, 33);
        expect_u("k31 longest", u.longest, 60);
        expect_u("k31 n50", u.n50, 31);
    }
    // many singletons and one long
    {
        std::vector<uint64_t> L(1000, 1);
        L[500] = 2000;
        const kmerust::UnitigSummary u = sum_of(L, 21);
        expect_u("many bases", u.bases, 999 * 21 + 2020);
        expect_u("many n50", u.n50, 21);  // 2020 < half of 22999
        expect_u("many longest", u.longest, 2020);
    }
    if (failures) return 1;
    printf("unitigs_check ok\n");
    return 0;
}
