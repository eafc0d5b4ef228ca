// unitig_text_check.cpp -- the HOST twin of krust_amd/csrc/unitig_text.hip.h (the unitig FASTA / GFA formatter the device runs on its
// LDS image) against the host writers of krust_amd/host/kmerust_host.h, for tests/test_unitig_text_records.py.  A stand-alone
// program with its own main: no device, no library.  It compares
//   ut_record_len + ut_put_generated   with  unitig_header / gfa_segment_tags / gfa_segment_line
//   ut_link_len + ut_put_link          with  gfa_link_line
//   ut_km                              with  snprintf("%.1f")
// on rows at every digit edge, writes every record a second time through windows that cut it at every offset (what a tile edge
// does), and prints "unitig_text_check ok <cases>" -- or the first difference, and exits 1.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../krust_amd/csrc/unitig_text.hip.h"
#include "../krust_amd/host/kmerust_host.h"

using namespace kmerust;

static uint64_t g_cases = 0;
static const size_t GUARD = 64;

[[noreturn]] static void die(const std::string &what) {
    printf("FAIL %s\n", what.c_str());
    exit(1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// what the host writers print for record i, the sequence being `seq`
static std::string host_record(uint32_t format, uint64_t i, const uint64_t *row, uint32_t k, const std::string &seq) {
    if (format == kh::UT_FASTA) return unitig_header(i, row, k) + "\n" + seq + "\n";
    return gfa_segment_line(i, row, k, seq.data(), seq.size()) + "\n";
}

// The record through the device's writers into a window [w0, w0 + span) of the record's bytes; the sequence is copied as the
// kernel copies it.  Returns the window's bytes; the buffer is guarded on both sides and has the sink's dump byte behind it.
static std::string twin_record(uint32_t format, uint64_t i, const uint64_t *row, uint32_t k, const std::string &seq, int64_t w0, uint32_t span) {
    const kh::UtRec r = kh::ut_rec(format, i, row, k);
    std::vector<uint8_t> buf(GUARD + span + GUARD + 1, 0xEE);
    const kh::UtSink sink{buf.data() + GUARD, span, (uint32_t)(span + GUARD)};
    const int64_t rel = -w0, rs = rel + r.pre, rp = rs + r.bases;
    kh::ut_put_generated(sink, format, (uint32_t)i, r, kh::ut_clip(rel), kh::ut_clip(rp));
    for (int64_t b = std::max<int64_t>(0, -rs); b < (int64_t)r.bases && rs + b < (int64_t)span; ++b) buf[GUARD + (size_t)(rs + b)] = (uint8_t)seq[(size_t)b];
    for (size_t g = 0; g < GUARD; ++g)
        if (buf[g] != 0xEE || buf[GUARD + span + g] != 0xEE) die("a writer left its window");
    return std::string((const char *)buf.data() + GUARD, span);
}

static void check_record(uint32_t format, uint64_t i, uint64_t L, uint64_t cs, bool circ, uint32_t k, bool windows) {
    uint64_t row[KH_UNI_WORDS];
    row[KH_UNI_START] = 0;
    row[KH_UNI_KMERS] = L;
    row[KH_UNI_COUNT_SUM] = cs;
    row[KH_UNI_FLAGS] = circ ? KH_UNI_CIRCULAR : 0;
    std::string seq((size_t)(L + k - 1), 'A');
    for (size_t b = 0; b < seq.size(); ++b) seq[b] = "ACGT"[(b * 7 + b / 5) & 3];
    const std::string want = host_record(format, i, row, k, seq);
    char id[160];
    snprintf(id, sizeof id, "format %u i %" PRIu64 " L %" PRIu64 " cs %" PRIu64 " circ %d k %u", format, i, L, cs, (int)circ, k);
    const uint32_t len = kh::ut_record_len(format, i, row, k);
    if (len != want.size()) die(std::string("ut_record_len: ") + id + ": " + std::to_string(len) + " for " + std::to_string(want.size()) + " bytes");
    const kh::UtRec r = kh::ut_rec(format, i, row, k);
    if (kh::ut_seq_offset(format, i, len, r.bases) != r.pre || want.compare(r.pre, seq.size(), seq) != 0) die(std::string("ut_seq_offset: ") + id);
    std::string whole;  // tile after tile, as the kernel builds it (a window is never longer than a tile: ut_clip counts on that)
    for (uint32_t w0 = 0; w0 < len; w0 += kh::UT_TILE) whole += twin_record(format, i, row, k, seq, w0, std::min(kh::UT_TILE, len - w0));
    if (whole != want) {
        size_t at = 0;
        while (at < want.size() && whole[at] == want[at]) ++at;
        die(std::string("the whole record: ") + id + ": first difference at byte " + std::to_string(at));
    }
    ++g_cases;
    if (!windows) return;
    for (uint32_t cut = 1; cut < len && len <= kh::UT_TILE; ++cut) {  // a tile edge at every offset: the part in front of it and the part behind it
        if (twin_record(format, i, row, k, seq, 0, cut) != want.substr(0, cut)) die(std::string("the head up to ") + std::to_string(cut) + ": " + id);
        if (twin_record(format, i, row, k, seq, cut, len - cut) != want.substr(cut)) die(std::string("the tail from ") + std::to_string(cut) + ": " + id);
        ++g_cases;
    }
}

static void check_link(uint32_t from, uint32_t fs, uint32_t to, uint32_t ts, uint32_t k) {
    const uint64_t w = ((uint64_t)(2u * from + fs) << 32) | (uint64_t)(2u * to + ts);
    const std::string want = gfa_link_line(w, k) + "\n";
    const uint32_t len = kh::ut_link_len(w, k);
    char id[120];
    snprintf(id, sizeof id, "link %u%c -> %u%c k %u", from, fs ? '-' : '+', to, ts ? '-' : '+', k);
    if (len != want.size()) die(std::string("ut_link_len: ") + id);
    for (uint32_t cut = 0; cut < len; ++cut) {  // the line behind a tile edge at `cut`, and in front of it
        for (int side = 0; side < 2; ++side) {
            const uint32_t span = side ? cut : len - cut;
            if (!span) continue;
            std::vector<uint8_t> buf(GUARD + span + GUARD + 1, 0xEE);
            const kh::UtSink sink{buf.data() + GUARD, span, (uint32_t)(span + GUARD)};
            const int32_t end = kh::ut_put_link(sink, side ? 0 : -(int32_t)cut, w, k);
            if (end != (side ? (int32_t)len : (int32_t)(len - cut))) die(std::string("ut_put_link's end: ") + id);
            for (size_t g = 0; g < GUARD; ++g)
                if (buf[g] != 0xEE || buf[GUARD + span + g] != 0xEE) die(std::string("ut_put_link left its window: ") + id);
            if (std::string((const char *)buf.data() + GUARD, span) != (side ? want.substr(0, cut) : want.substr(cut))) die(std::string("ut_put_link: ") + id);
        }
    }
    ++g_cases;
}

static void check_km(uint64_t cs, uint64_t L) {
    char want[64];
    snprintf(want, sizeof want, "%.1f", L ? (double)cs / (double)L : 0.0);
    const kh::UtKm m = kh::ut_km(cs, L);
    uint8_t buf[64 + 1];
    memset(buf, 0xEE, sizeof buf);
    const kh::UtSink sink{buf, 64, 64};
    const int32_t end = kh::ut_put_km(sink, 0, m);
    if (end != (int32_t)kh::ut_km_len(m) || (size_t)end != strlen(want) || memcmp(buf, want, (size_t)end) != 0) {
        buf[end > 0 && end < 64 ? end : 0] = 0;
        die("km of " + std::to_string(cs) + " / " + std::to_string(L) + ": " + (const char *)buf + " for " + want);
    }
    ++g_cases;
}

int main() {
    // the digit edges: 10^d - 1 and 10^d
    std::vector<uint64_t> edges32, edges64;
    for (uint64_t p = 10; p < (1ull << 31); p *= 10) {
        edges32.push_back(p - 1);
        edges32.push_back(p);
    }
    edges32.push_back(0);
    edges32.push_back((1ull << 31) - 1);
    for (uint64_t p = 10;; p *= 10) {
        edges64.push_back(p - 1);
        edges64.push_back(p);
        if (p == 10000000000000000000ull) break;
    }
    for (uint64_t v : {0ull, 1ull, (1ull << 32) - 1, 1ull << 32, (1ull << 53) - 1, 1ull << 53, (1ull << 53) + 1, 1ull << 63, ~0ull - 1, ~0ull}) edges64.push_back(v);

    for (uint32_t format : {kh::UT_FASTA, kh::UT_GFA}) {
        // i and cs at every edge, both flags, k = 1, 21, 32; short sequences, cut at every offset
        for (uint32_t k : {1u, 21u, 32u})
            for (int circ = 0; circ < 2; ++circ) {
                for (uint64_t i : edges32) check_record(format, i, 3, 17, circ, k, true);
                for (uint64_t cs : edges64) check_record(format, 5, 1, cs, circ, k, true);
                for (uint64_t cs : edges64) check_record(format, 12345, 7, cs, circ, k, false);
            }
        // L + k - 1 at every edge (whole records only beyond a few thousand bases: the windows are quadratic)
        for (uint32_t k : {1u, 32u})
            for (uint64_t len : edges32) {
                if (len < k || len > 10000000ull) continue;  // (longer sequences are more than this check should allocate: below)
                check_record(format, 99, len - k + 1, 1000003, len & 1, k, len <= 1000);
            }
        // the ties of km in a whole record
        for (uint64_t x = 0; x < 50; ++x) {
            check_record(format, x, 4, 4 * x + 1, false, 21, false);
            check_record(format, x, 4, 4 * x + 3, true, 21, false);
        }
        check_record(format, 0, 0, 0, false, 1, true);  // (L = 0 is no unitig, but the writers are defined for it)
    }
    // bases at the edges above what a sequence is allocated for here: the lengths and tags alone
    for (uint64_t len : {99999999ull, 100000000ull, 999999999ull, 1000000000ull, (1ull << 31) - 1 + 31}) {
        uint64_t row[KH_UNI_WORDS] = {0, len - 31, 77, 0};
        const std::string tags = gfa_segment_tags(row, 32);
        const kh::UtRec r = kh::ut_rec(kh::UT_GFA, 1, row, 32);
        std::vector<uint8_t> buf(tags.size() + 1, 0xEE);
        const kh::UtSink sink{buf.data(), (uint32_t)tags.size(), (uint32_t)tags.size()};
        if (kh::ut_tags_len(r) != tags.size() || kh::ut_put_tags(sink, 0, r, '\t') != (int32_t)tags.size() || memcmp(buf.data(), tags.data(), tags.size()) != 0)
            die("tags at " + std::to_string(len) + " bases");
        ++g_cases;
    }

    // links: both indices at every edge, both signs on both sides, k = 1 (0M), 10, 11, 32
    for (uint32_t k : {1u, 10u, 11u, 32u})
        for (uint32_t fs = 0; fs < 2; ++fs)
            for (uint32_t ts = 0; ts < 2; ++ts) {
                for (uint64_t a : edges32) {
                    check_link((uint32_t)a, fs, 7, ts, k);
                    check_link(7, fs, (uint32_t)a, ts, k);
                    check_link((uint32_t)a, fs, (uint32_t)a, ts, k);
                }
            }

    // km
    for (uint64_t x = 0; x < 3000; ++x) {
        check_km(4 * x + 1, 4);  // .25 and .75: the ties
        check_km(4 * x + 3, 4);
    }
    for (uint64_t x = 0; x < 64; ++x) {
        check_km((1ull << x) + 1, 4);
        check_km((1ull << x) + 3, 4);
        check_km(((1ull << x) | 1ull), 8);  // .125
    }
    for (uint64_t cs = 0; cs < 2000; ++cs)
        for (uint64_t L = 0; L < 200; ++L) check_km(cs, L);  // L = 0, cs < L and everything small
    for (uint64_t cs : edges64)
        for (uint64_t L : {1ull, 2ull, 3ull, 4ull, 7ull, 10ull, 1000ull, (1ull << 31) - 1, 1ull << 52, 1ull << 53, (1ull << 53) + 1, 1ull << 63, ~0ull}) check_km(cs, L);
    for (uint64_t d = 0; d < 2000; ++d) {
        check_km((1ull << 53) + d, 1);  // cs >= 2^53: the conversion rounds
        check_km((1ull << 53) + d, 10);
        check_km(~0ull - d, 1);  // 2^64 - 1 and below: up to 2^64 as a double
        check_km(~0ull - d * 1024, 3);
    }
    for (int n = 0; n < 200000; ++n) {
        const uint64_t a = rnd(), b = rnd();
        check_km(a, b);                           // anything
        check_km(a >> (b & 63), (b >> 33) + 1);   // every magnitude over a 31-bit L
        check_km(a >> 40, (b >> 40) + 1);         // quotients near 1
    }

    printf("unitig_text_check ok %" PRIu64 "\n", g_cases);
    return 0;
}
