// unitig_links_check.cpp -- the host-checkable side of kh_unitigs_links_* and `kmerust gfa`: the link word and the enter-sign decision
// of krust_amd/csrc/unitig_bits.h (what unitig_link_out_kernel runs per successor) against string arithmetic for k = 1..32, the
// KH_UNI_LINK_* macros of include/kmerhip.h, and gfa_segment_line / gfa_link_line / link_summary of krust_amd/host/kmerust_host.h on
// hand-made rows and links.  Pure host code with its own main: compiled and run by tests/test_unitig_links_host.py (once more with
// -fsanitize=address,undefined), no device and no library needed.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../krust_amd/csrc/unitig_bits.h"
#include "../krust_amd/host/kmerust_host.h"

static int failures = 0;
static void expect_u(const std::string &what, uint64_t got, uint64_t want) {
    if (got != want) {
        printf("FAIL %s: got %llu, want %llu\n", what.c_str(), (unsigned long long)got, (unsigned long long)want);
        ++failures;
    }
}
static void expect_s(const std::string &what, const std::string &got, const std::string &want) {
    if (got != want) {
        printf("FAIL %s: got '%s', want '%s'\n", what.c_str(), got.c_str(), want.c_str());
        ++failures;
    }
}

// ---- strings ---------------------------------------------------------------------------------------------------------------------
static std::string rc(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}
static std::string canon(const std::string &s) {
    const std::string r = rc(s);
    return s <= r ? s : r;
}
static uint64_t pack(const std::string &s) {
    uint64_t x = 0;
    for (char c : s) x = (x << 2) | (uint64_t)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3);
    return x;
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static std::string random_string(size_t n) {
    std::string s;
    for (size_t i = 0; i < n; ++i) s.push_back("ACGT"[rnd() & 3u]);
    return s;
}

// The sign the unitig with the reported sequence `seq` is entered with by the string t, from strings alone: 0 = t is its first
// k-mer, 1 = t is the first k-mer of its reverse complement, 2 = neither.  The first is tested first.
static uint32_t enter_by_strings(const std::string &seq, uint32_t k, const std::string &t) {
    if (t == seq.substr(0, k)) return 0;
    if (t == rc(seq.substr(seq.size() - k))) return 1;
    return 2;
}
// The same through unitig_bits.h: a predecessor that spells p = a + t[:-1] is stepped on by t's last letter (kh_unitig_successor on
// its packed canonical key and sign), the node entered is looked for in the reading, and kh_unitig_enter_sign decides.
static uint32_t enter_by_bits(const std::string &seq, uint32_t k, const std::string &t) {
    const std::string p = std::string(1, "ACGT"[rnd() & 3u]) + t.substr(0, k - 1);
    const std::string pc = canon(p);
    uint64_t y;
    uint32_t ysign;
    bool ypal;
    kh_unitig_successor(pack(pc), k, p == pc ? 0u : 1u, (uint32_t)std::string("ACGT").find(t[k - 1]), &y, &ysign, &ypal);
    expect_u("successor key of " + t, y, pack(canon(t)));
    expect_u("successor palindrome of " + t, ypal ? 1 : 0, rc(t) == t ? 1 : 0);
    const uint32_t L = (uint32_t)(seq.size() - k + 1);
    for (uint32_t pos = 0; pos < L; ++pos) {
        const std::string w = seq.substr(pos, k);
        if (pack(canon(w)) == y) return kh_unitig_enter_sign(pos, L, w == canon(w) ? 0u : 1u, ysign);
    }
    return 99;  // (the node is not in this unitig)
}
static void check_enter(const std::string &what, const std::string &seq, uint32_t k, const std::string &t) {
    expect_u(what + " k=" + std::to_string(k) + " seq=" + seq + " t=" + t, enter_by_bits(seq, k, t), enter_by_strings(seq, k, t));
}

int main() {
    // ---- the link word: helper against macros, every sign, indices up to 2^31 - 2 -------------------------------------------------
    {
        const uint32_t ids[] = {0u, 1u, 2u, 77u, 65535u, 65536u, 0x3FFFFFFFu, 0x40000000u, 0x7FFFFFFDu, 0x7FFFFFFEu};
        for (uint32_t a : ids)
            for (uint32_t b : ids)
                for (uint32_t s = 0; s < 4; ++s) {
                    const uint64_t w = kh_unitig_link_word(a, s >> 1, b, s & 1u);
                    expect_u("word value", w, ((2ull * a + (s >> 1)) << 32) | (2ull * b + (s & 1u)));
                    expect_u("from", KH_UNI_LINK_FROM(w), a);
                    expect_u("from sign", KH_UNI_LINK_FROM_SIGN(w), s >> 1);
                    expect_u("to", KH_UNI_LINK_TO(w), b);
                    expect_u("to sign", KH_UNI_LINK_TO_SIGN(w), s & 1u);
                }
        // the order of the words is the order of (from, from sign, to, to sign)
        expect_u("order: + end first", kh_unitig_link_word(5, 0, 9, 1) < kh_unitig_link_word(5, 1, 0, 0) ? 1 : 0, 1);
        expect_u("order: by from", kh_unitig_link_word(5, 1, 9, 1) < kh_unitig_link_word(6, 0, 0, 0) ? 1 : 0, 1);
        expect_u("order: by to", kh_unitig_link_word(5, 0, 3, 1) < kh_unitig_link_word(5, 0, 4, 0) ? 1 : 0, 1);
        expect_u("order: to + first", kh_unitig_link_word(5, 0, 3, 0) < kh_unitig_link_word(5, 0, 3, 1) ? 1 : 0, 1);
    }
    // ---- the enter sign, k = 1..32 ---------------------------------------------------------------------------------------------------
    for (uint32_t k = 1; k <= 32; ++k) {
        for (int round = 0; round < 8; ++round) {
            // L = 1: the node entered both ways
            std::string one = random_string(k);
            if (rc(one) == one) one[0] = one[0] == 'A' ? 'C' : 'A';  // (not a palindrome here)
            one = canon(one);                                          // (L = 1 is reported as (x, +))
            check_enter("L1 as +", one, k, one);
            check_enter("L1 as -", one, k, rc(one));
            expect_u("L1 as - is -", enter_by_strings(one, k, rc(one)), 1);
            // L = 2 and L = 5: the first node, rev() of the last, and for L = 5 what must not happen
            for (uint32_t L : {2u, 5u}) {
                std::string seq;
                for (int tries = 0; tries < 100; ++tries) {  // (all nodes distinct, none a palindrome)
                    seq = random_string(L + k - 1);
                    std::vector<std::string> nodes;
                    bool ok = true;
                    for (uint32_t i = 0; i < L; ++i) {
                        const std::string w = seq.substr(i, k);
                        ok = ok && rc(w) != w;
                        nodes.push_back(canon(w));
                    }
                    std::sort(nodes.begin(), nodes.end());
                    if (ok && std::adjacent_find(nodes.begin(), nodes.end()) == nodes.end()) break;
                    seq.clear();
                }
                if (seq.empty()) continue;  // (k = 1, L = 5: there are two nodes only)
                check_enter("first", seq, k, seq.substr(0, k));
                check_enter("rev(last)", seq, k, rc(seq.substr(seq.size() - k)));
                expect_u("first is +", enter_by_strings(seq, k, seq.substr(0, k)), 0);
                expect_u("rev(last) is -", enter_by_strings(seq, k, rc(seq.substr(seq.size() - k))), 1);
                check_enter("rev(first): neither", seq, k, rc(seq.substr(0, k)));
                check_enter("last: neither", seq, k, seq.substr(seq.size() - k));
                if (L == 5) {
                    check_enter("interior", seq, k, seq.substr(2, k));
                    check_enter("rev(interior)", seq, k, rc(seq.substr(2, k)));
                }
                expect_u("KH_UNI_ENTER_NONE", enter_by_strings(seq, k, seq.substr(seq.size() - k)), KH_UNI_ENTER_NONE);
            }
            // a palindrome (even k): a unitig of its own, entered as + whichever way it is reached
            if (k % 2 == 0) {
                const std::string h = random_string(k / 2), pal = h + rc(h);
                check_enter("palindrome", pal, k, pal);
                expect_u("palindrome is +", enter_by_strings(pal, k, rc(pal)), 0);
                expect_u("palindrome: helper, either sign", kh_unitig_enter_sign(0, 1, 0, 0), 0);
            }
        }
    }
    expect_u("L1 + ", kh_unitig_enter_sign(0, 1, 0, 0), 0);
    expect_u("L1 -", kh_unitig_enter_sign(0, 1, 0, 1), 1);
    expect_u("first written as -", kh_unitig_enter_sign(0, 7, 1, 1), 0);
    expect_u("last written as -, entered as +", kh_unitig_enter_sign(6, 7, 1, 0), 1);
    expect_u("interior", kh_unitig_enter_sign(3, 7, 0, 0), KH_UNI_ENTER_NONE);
    expect_u("last as itself", kh_unitig_enter_sign(6, 7, 0, 0), KH_UNI_ENTER_NONE);

    // ---- GFA lines -----------------------------------------------------------------------------------------------------------------------
    {
        const uint64_t a[KH_UNI_WORDS] = {0, 3, 7, 0};
        expect_s("S line", kmerust::gfa_segment_line(0, a, 5, "ACGTTGA", 7), "S\t0\tACGTTGA\tLN:i:7\tKC:i:7\tkm:f:2.3");
        const uint64_t b[KH_UNI_WORDS] = {30, 3, 3, KH_UNI_CIRCULAR};
        expect_s("circular S line", kmerust::gfa_segment_line(2147483646ull, b, 2, "ACGA", 4), "S\t2147483646\tACGA\tLN:i:4\tKC:i:3\tkm:f:1.0\tCR:i:1");
        // the tags are those of unitig_header(), tab for blank
        std::string h = kmerust::unitig_header(0, b, 31).substr(3);
        std::replace(h.begin(), h.end(), ' ', '\t');
        expect_s("tags as unitig_header", kmerust::gfa_segment_tags(b, 31), h);
        const uint64_t c[KH_UNI_WORDS] = {0, 1, 18446744073709551615ull, 0};
        expect_s("count sum 2^64 - 1", kmerust::gfa_segment_tags(c, 1), "LN:i:1\tKC:i:18446744073709551615\tkm:f:18446744073709551616.0");
        expect_s("L line", kmerust::gfa_link_line(kh_unitig_link_word(3, 0, 4, 1), 21), "L\t3\t+\t4\t-\t20M");
        expect_s("L line, k = 1", kmerust::gfa_link_line(kh_unitig_link_word(0, 1, 0, 1), 1), "L\t0\t-\t0\t-\t0M");
        expect_s("L line near 2^31", kmerust::gfa_link_line(kh_unitig_link_word(0x7FFFFFFEu, 1, 0x7FFFFFFDu, 0), 32), "L\t2147483646\t-\t2147483645\t+\t31M");
        expect_s("L line at 2^31 - 2, both", kmerust::gfa_link_line(kh_unitig_link_word(0x7FFFFFFEu, 0, 0x7FFFFFFEu, 1), 32),
                 "L\t2147483646\t+\t2147483646\t-\t31M");
    }
    // ---- the link summary ------------------------------------------------------------------------------------------------------------
    auto expect_sum = [](const std::string &what, const kmerust::LinkSummary &s, uint64_t unitigs, uint64_t links, uint64_t self_links, uint64_t dead_ends,
                         uint64_t isolated, uint64_t tips) {
        expect_u(what + " unitigs", s.unitigs, unitigs);
        expect_u(what + " links", s.links, links);
        expect_u(what + " self_links", s.self_links, self_links);
        expect_u(what + " dead_ends", s.dead_ends, dead_ends);
        expect_u(what + " isolated", s.isolated, isolated);
        expect_u(what + " tips", s.tips, tips);
    };
    expect_sum("none", kmerust::link_summary(nullptr, 0, nullptr, 0, 21), 0, 0, 0, 0, 0, 0);
    {
        const uint64_t rows[] = {0, 1, 4, 0};  // one isolated unitig: both ends dead; no tip (a tip has exactly one)
        expect_sum("isolated", kmerust::link_summary(rows, 1, nullptr, 0, 21), 1, 0, 0, 2, 1, 0);
    }
    {
        const uint64_t rows[] = {0, 3, 3, KH_UNI_CIRCULAR};
        const uint64_t links[] = {kh_unitig_link_word(0, 0, 0, 0), kh_unitig_link_word(0, 1, 0, 1)};
        expect_sum("circular", kmerust::link_summary(rows, 1, links, 2, 21), 1, 2, 2, 0, 0, 0);
    }
    {
        // k = 5: unitig 0 (L = 10) forks at its + end into 1 (L = 3: a tip) and 2 (L = 20: a dead end, too long for a tip)
        const uint64_t rows[] = {0, 10, 10, 0, 14, 3, 3, 0, 21, 20, 20, 0};
        const uint64_t links[] = {kh_unitig_link_word(0, 0, 1, 0), kh_unitig_link_word(0, 0, 2, 0), kh_unitig_link_word(1, 1, 0, 1),
                                  kh_unitig_link_word(2, 1, 0, 1)};
        expect_sum("tip", kmerust::link_summary(rows, 3, links, 4, 5), 3, 4, 0, 3, 0, 1);
        expect_sum("tip, KMERS = k", kmerust::link_summary(rows, 3, links, 4, 3), 3, 4, 0, 3, 0, 1);
        expect_sum("tip, KMERS > k", kmerust::link_summary(rows, 3, links, 4, 2), 3, 4, 0, 3, 0, 0);
        const uint64_t circ[] = {0, 10, 10, 0, 14, 3, 3, KH_UNI_CIRCULAR, 21, 20, 20, 0};  // (no such graph; the flag alone excludes it)
        expect_sum("a circular one is no tip", kmerust::link_summary(circ, 3, links, 4, 5), 3, 4, 0, 3, 0, 0);
    }
    {
        // a hairpin: 0+ -> 0-, its own mirror; the - end is dead
        const uint64_t rows[] = {0, 30, 30, 0};
        const uint64_t links[] = {kh_unitig_link_word(0, 0, 0, 1)};
        expect_sum("hairpin", kmerust::link_summary(rows, 1, links, 1, 21), 1, 1, 1, 1, 0, 0);
        expect_sum("hairpin, short", kmerust::link_summary(rows, 1, links, 1, 31), 1, 1, 1, 1, 0, 1);
    }
    {
        // indices near 2^31 - 2: links that leave unitigs beyond the rows given count as links and self-links, and touch no end
        const uint64_t rows[] = {0, 1, 1, 0, 21, 1, 1, 0};
        const uint64_t links[] = {kh_unitig_link_word(1, 0, 0x7FFFFFFEu, 1), kh_unitig_link_word(0x7FFFFFFDu, 1, 0x7FFFFFFEu, 0),
                                  kh_unitig_link_word(0x7FFFFFFEu, 1, 0x7FFFFFFEu, 1)};
        expect_sum("near 2^31", kmerust::link_summary(rows, 2, links, 3, 21), 2, 3, 1, 3, 1, 1);
    }
    if (failures) return 1;
    printf("unitig_links_check ok\n");
    return 0;
}
