// alloc_inject.h -- the arming logic of KMERHIP_ALLOC_FAIL (test build only; ctx.hip.h, Knobs): which allocation fails.
//
//   "n"    the n-th allocation after the variable took this value fails (1-based); those before and after it succeed
//   "n+"   the n-th and every later one fail
//   unset, empty or anything else: disarmed
//
// A changed value re-arms and restarts the count.  Pure C++ without HIP and without a lock (the caller holds one):
// tests/alloc_inject_check.cpp checks it on the host, plain and under the sanitizers.
#pragma once
#include <cstdint>
#include <cstring>

namespace khi {

struct AllocInject {
    char armed[24] = {0};  // the value the count belongs to ("" = disarmed)
    uint64_t n = 0;        // 0: disarmed (also: a value that does not parse)
    bool plus = false;
    uint64_t count = 0;    // allocations seen since that value appeared

    // n / n+ with n >= 1 in decimal, at most 18 digits: true and *n, *plus; everything else false
    static bool parse(const char *s, uint64_t *n, bool *plus) {
        if (!s || !*s) return false;
        uint64_t v = 0;
        int digits = 0;
        for (; *s >= '0' && *s <= '9'; ++s, ++digits) {
            if (digits >= 18) return false;
            v = v * 10 + (uint64_t)(*s - '0');
        }
        if (!digits || v == 0) return false;
        const bool p = *s == '+';
        if (p) ++s;
        if (*s) return false;
        *n = v;
        *plus = p;
        return true;
    }

    // One allocation is about to be made while the variable holds `env` (nullptr: unset).  Returns its ordinal (>= 1) when
    // it has to fail, 0 when it goes to the runtime.
    uint64_t step(const char *env) {
        if (!env) env = "";
        if (strncmp(env, armed, sizeof(armed)) != 0 || strlen(env) >= sizeof(armed)) {  // a new value: re-arm
            const bool fits = strlen(env) < sizeof(armed);
            memset(armed, 0, sizeof(armed));
            if (fits) memcpy(armed, env, strlen(env));
            n = 0;
            plus = false;
            count = 0;
            if (fits && !parse(env, &n, &plus)) n = 0;
            if (!fits) return 0;  // (too long to be n / n+: disarmed, and compared again next time)
        }
        if (!n) return 0;
        ++count;
        if (count == n || (plus && count > n)) return count;
        return 0;
    }
};

}  // namespace khi
