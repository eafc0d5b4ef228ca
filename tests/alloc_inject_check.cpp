// The arming logic of KMERHIP_ALLOC_FAIL (krust_amd/csrc/alloc_inject.h) on the host: a stand-alone program with its own main,
// nothing preloaded -- tests/test_alloc_inject.py builds and runs it plain and under ASan + UBSan.
#include "../krust_amd/csrc/alloc_inject.h"

#include <cstdio>
#include <string>
#include <vector>

static int g_bad = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_bad;                                                     \
        }                                                                \
    } while (0)

// the ordinals (0: goes to the runtime) of `steps` allocations made while the variable holds `env`
static std::vector<uint64_t> run(khi::AllocInject &a, const char *env, int steps) {
    std::vector<uint64_t> out;
    for (int i = 0; i < steps; ++i) out.push_back(a.step(env));
    return out;
}

int main() {
    using khi::AllocInject;
    typedef std::vector<uint64_t> V;
    {   // the parser: n and n+ with n >= 1, nothing else
        uint64_t n = 99;
        bool plus = true;
        CHECK(AllocInject::parse("1", &n, &plus) && n == 1 && !plus);
        CHECK(AllocInject::parse("37+", &n, &plus) && n == 37 && plus);
        CHECK(AllocInject::parse("000012", &n, &plus) && n == 12 && !plus);
        CHECK(AllocInject::parse("999999999999999999", &n, &plus) && n == 999999999999999999ull);
        for (const char *bad : {"", "0", "0+", "+", "+3", "-1", "3++", "3 ", " 3", "3+x", "x", "1e3", "0x10", "1234567890123456789", "3-"})
            CHECK(!AllocInject::parse(bad, &n, &plus));
        CHECK(!AllocInject::parse(nullptr, &n, &plus));
    }
    {   // unset and empty: disarmed, nothing is counted
        AllocInject a;
        CHECK(run(a, nullptr, 4) == V({0, 0, 0, 0}));
        CHECK(run(a, "", 4) == V({0, 0, 0, 0}));
        CHECK(a.count == 0);
    }
    {   // n: exactly the n-th, those before and after succeed
        AllocInject a;
        CHECK(run(a, "3", 6) == V({0, 0, 3, 0, 0, 0}));
        AllocInject b;
        CHECK(run(b, "1", 3) == V({1, 0, 0}));
    }
    {   // n+: the n-th and every later one, with their own ordinals
        AllocInject a;
        CHECK(run(a, "2+", 5) == V({0, 2, 3, 4, 5}));
        AllocInject b;
        CHECK(run(b, "1+", 3) == V({1, 2, 3}));
    }
    {   // a changed value re-arms and restarts the count; the same value again does not
        AllocInject a;
        CHECK(run(a, "2", 1) == V({0}));
        CHECK(run(a, "3", 3) == V({0, 0, 3}));    // (not the 2nd of "2": the count started again)
        CHECK(run(a, "3", 3) == V({0, 0, 0}));    // (still "3": it fired once)
        CHECK(run(a, "3+", 3) == V({0, 0, 3}));   // ("3+" is another value)
        CHECK(run(a, nullptr, 2) == V({0, 0}));   // disarmed ...
        CHECK(run(a, "3+", 3) == V({0, 0, 3}));   // ... and armed again with the value it had: a fresh count
        CHECK(run(a, "", 2) == V({0, 0}));
        CHECK(run(a, "1", 2) == V({1, 0}));
    }
    {   // what does not parse disarms, also when it is longer than any n / n+ can be
        AllocInject a;
        CHECK(run(a, "2", 1) == V({0}));
        CHECK(run(a, "two", 3) == V({0, 0, 0}));
        CHECK(run(a, "2", 2) == V({0, 2}));
        const std::string longv(200, '7');
        CHECK(run(a, longv.c_str(), 3) == V({0, 0, 0}));
        CHECK(run(a, "1", 1) == V({1}));
        const std::string prefix = "1" + std::string(40, ' ');  // (shares its first bytes with an armed value: still another value)
        CHECK(run(a, prefix.c_str(), 2) == V({0, 0}));
        CHECK(run(a, "1", 1) == V({1}));
    }
    if (g_bad) {
        fprintf(stderr, "alloc_inject_check: %d check(s) failed\n", g_bad);
        return 1;
    }
    printf("alloc_inject_check ok\n");
    return 0;
}
