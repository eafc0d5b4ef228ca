// join_check.cpp -- the derived measures of `kmerust compare` (krust_amd/host/kmerust_host.h: compare_measures, format_measure)
// on hand-computed words.  Pure host code: compiled and run by tests/test_join_host.py, no device and no library needed.
#include <cstdio>
#include <cstring>
#include <string>

#include "../krust_amd/host/kmerust_host.h"

static int failures = 0;
static void expect(const char *what, const std::string &got, const char *want) {
    if (got != want) {
        printf("FAIL %s: got %s, want %s\n", what, got.c_str(), want);
        ++failures;
    }
}
static void check(const char *name, const uint64_t *w, const char *j, const char *ca, const char *cb, const char *bc) {
    const kmerust::CompareMeasures m = kmerust::compare_measures(w);
    const std::string n = name;
    expect((n + " jaccard").c_str(), kmerust::format_measure(m.jaccard), j);
    expect((n + " containment_a").c_str(), kmerust::format_measure(m.containment_a), ca);
    expect((n + " containment_b").c_str(), kmerust::format_measure(m.containment_b), cb);
    expect((n + " bray_curtis").c_str(), kmerust::format_measure(m.bray_curtis), bc);
}

int main() {
    uint64_t w[KH_CMP_WORDS];
    memset(w, 0, sizeof(w));  // two empty tables: every divisor is 0
    check("zero", w, "nan", "nan", "nan", "nan");
    // identical tables: 1000 keys, 2500 occurrences
    w[KH_CMP_DISTINCT_A] = w[KH_CMP_DISTINCT_B] = w[KH_CMP_SHARED] = 1000;
    w[KH_CMP_SUM_A] = w[KH_CMP_SUM_B] = w[KH_CMP_SHARED_SUM_A] = w[KH_CMP_SHARED_SUM_B] = w[KH_CMP_SUM_MIN] = 2500;
    check("identical", w, "1.000000", "1.000000", "1.000000", "0.000000");
    // by hand: |A| = 8, |B| = 6, 3 shared -> J = 3 / 11, C_a = 3 / 8, C_b = 1 / 2; sums 20 and 10, sum_min 5 -> BC = 1 - 10 / 30
    w[KH_CMP_DISTINCT_A] = 8, w[KH_CMP_DISTINCT_B] = 6, w[KH_CMP_SHARED] = 3;
    w[KH_CMP_SUM_A] = 20, w[KH_CMP_SUM_B] = 10, w[KH_CMP_SHARED_SUM_A] = 9, w[KH_CMP_SHARED_SUM_B] = 6, w[KH_CMP_SUM_MIN] = 5;
    check("hand", w, "0.272727", "0.375000", "0.500000", "0.666667");
    // a only: b is empty
    memset(w, 0, sizeof(w));
    w[KH_CMP_DISTINCT_A] = 4, w[KH_CMP_SUM_A] = 9;
    check("a only", w, "0.000000", "0.000000", "nan", "1.000000");
    if (failures) return 1;
    printf("join_check ok\n");
    return 0;
}
