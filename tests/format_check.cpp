// format_check.cpp -- drives the HOST twin of krust_amd/csrc/format.hip.h (the record formatter the device runs on
// LDS) for tests/test_format_records.py.  Reads cases from stdin, one per line:
//     R <format> <k> <key> <count> <first>          one record
//     D <format> <k> <n> <key> <count> ...          a whole document of n records (the first flag, then the tail)
// and answers each with "<record_len sum> <bytes written> <hex of the bytes>".  The buffer is guarded on both sides: a
// writer that leaves its record_len() is reported, not silently tolerated.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../krust_amd/csrc/format.hip.h"

int main() {
    char line[1 << 16];
    const size_t GUARD = 64;
    while (fgets(line, sizeof line, stdin)) {
        char kind = 0;
        unsigned format = 0, k = 0;
        int pos = 0;
        if (sscanf(line, " %c %u %u%n", &kind, &format, &k, &pos) != 3) continue;
        if (!kh::fmt_valid(format) || k < 1 || k > 32) {
            printf("ERR bad case\n");
            continue;
        }
        const char *p = line + pos;
        std::vector<std::pair<uint64_t, uint64_t>> recs;
        unsigned long long n = 1, first = 0;
        int adv = 0;
        if (kind == 'D') {
            if (sscanf(p, "%llu%n", &n, &adv) != 1) return 2;
            p += adv;
        }
        for (unsigned long long i = 0; i < n; ++i) {
            unsigned long long key = 0, cnt = 0;
            if (sscanf(p, "%llu %llu%n", &key, &cnt, &adv) != 2) return 2;
            p += adv;
            recs.push_back({key, cnt});
        }
        if (kind == 'R' && sscanf(p, "%llu", &first) != 1) return 2;
        std::vector<uint8_t> buf(GUARD + recs.size() * kh::record_len_max(format, k) + kh::FMT_TAIL_LEN + GUARD, 0xEE);
        uint8_t *w = buf.data() + GUARD;
        uint64_t want = 0;
        for (size_t i = 0; i < recs.size(); ++i) {
            const uint32_t len = kh::record_len(format, k, recs[i].second);
            if (len > kh::record_len_max(format, k)) return 3;
            want += len;
            w += kh::write_record(w, format, k, recs[i].first, recs[i].second, kind == 'D' ? i == 0 : first != 0);
        }
        if (kind == 'D') {
            want += format == kh::FMT_JSON ? kh::FMT_TAIL_LEN : 0;
            w += kh::write_tail(w, format, recs.size());
        }
        const size_t wrote = (size_t)(w - (buf.data() + GUARD));
        bool guard_ok = true;
        for (size_t i = 0; i < GUARD; ++i) guard_ok = guard_ok && buf[i] == 0xEE && buf[GUARD + wrote + i] == 0xEE;
        if (!guard_ok) {
            printf("ERR wrote outside the record\n");
            continue;
        }
        // every record start inside the text is found by the piece cutter's rule, and nothing else is
        if (kind == 'D' && recs.size() > 1) {
            const uint8_t *t = buf.data() + GUARD;
            const size_t body = wrote - (format == kh::FMT_JSON ? kh::FMT_TAIL_LEN : 0);
            std::vector<size_t> starts;
            size_t o = 0;
            for (size_t i = 0; i < recs.size(); ++i) {
                if (i) starts.push_back(o);
                o += kh::record_len(format, k, recs[i].second);
            }
            size_t si = 0;
            for (size_t e = 1; e < body; ++e) {
                const bool is = kh::fmt_record_starts_at(format, t, e);
                const bool should = si < starts.size() && starts[si] == e;
                if (is != should) {
                    printf("ERR record start rule at %zu\n", e);
                    return 4;
                }
                if (should) ++si;
            }
        }
        printf("%" PRIu64 " %zu ", want, wrote);
        for (size_t i = 0; i < wrote; ++i) printf("%02x", buf[GUARD + i]);
        printf("\n");
    }
    puts("FORMAT_CHECK_DONE");
    return 0;
}
