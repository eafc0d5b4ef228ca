// graph_check.cpp -- the host side of `kmerust graph` (krust_amd/host/kmerust_host.h: graph_summary, format_graph_line) on hand-made
// words.  Pure host code with its own main: compiled and run by tests/test_graph_host.py (once more with -fsanitize=address,undefined),
// no device and no library needed.
#include <cstdio>
#include <cstring>
#include <string>

#include "../krust_amd/host/kmerust_host.h"

static int failures = 0;
static void expect_u(const char *what, uint64_t got, uint64_t want) {
    if (got != want) {
        printf("FAIL %s: got %llu, want %llu\n", what, (unsigned long long)got, (unsigned long long)want);
        ++failures;
    }
}
static void expect_line(const char *what, uint64_t key, uint32_t k, uint64_t count, uint8_t mask, const std::string &want) {
    std::string got = "x";  // (the line is APPENDED)
    kmerust::format_graph_line(got, key, k, count, mask);
    if (got != "x" + want) {
        printf("FAIL %s: got %s want %s\n", what, got.c_str(), want.c_str());
        ++failures;
    }
}
static unsigned bits4(unsigned v) { return (v & 1) + ((v >> 1) & 1) + ((v >> 2) & 1) + ((v >> 3) & 1); }

int main() {
    uint64_t w[KH_GRAPH_WORDS];
    // an empty table
    memset(w, 0, sizeof(w));
    kmerust::GraphSummary g = kmerust::graph_summary(w);
    expect_u("zero nodes", g.nodes, 0);
    expect_u("zero arcs", g.arcs, 0);
    expect_u("zero isolated", g.isolated, 0);
    for (int l = 0; l < 5; ++l)
        for (int r = 0; r < 5; ++r) expect_u("zero deg", g.deg[l][r], 0);
    // one node of each of the 256 masks, each counted 3 times: the cells are products of binomials C(4, l) * C(4, r)
    for (int m = 0; m < 256; ++m) w[m] = 1;
    w[KH_GRAPH_NODES] = 256, w[KH_GRAPH_KMERS] = 768;
    g = kmerust::graph_summary(w);
    static const uint64_t binom[5] = {1, 4, 6, 4, 1};
    uint64_t total = 0;
    for (int l = 0; l < 5; ++l)
        for (int r = 0; r < 5; ++r) {
            expect_u("each deg", g.deg[l][r], binom[l] * binom[r]);
            total += g.deg[l][r];
        }
    expect_u("each total", total, 256);
    expect_u("each nodes", g.nodes, 256);
    expect_u("each kmers", g.kmers, 768);
    expect_u("each arcs", g.arcs, 2 * 256 * 2);         // every side has mean degree 2
    expect_u("each isolated", g.isolated, 1);
    expect_u("each dead_ends", g.dead_ends, 2 * 15);     // one side empty, the other one of 15 non-empty patterns
    expect_u("each simple", g.simple, 16);
    expect_u("each branching", g.branching, 256 - 5 * 5);  // not branching: both sides of degree 0 or 1 -- (1 + 4)^2 masks
    {   // the same by the definition, mask by mask
        uint64_t de = 0, br = 0;
        for (unsigned m = 0; m < 256; ++m) {
            const unsigned l = bits4(m >> 4), r = bits4(m & 15);
            de += (l == 0) != (r == 0);
            br += l >= 2 || r >= 2;
        }
        expect_u("each dead_ends by definition", g.dead_ends, de);
        expect_u("each branching by definition", g.branching, br);
    }
    // words near 2^64: the sums wrap like the words do
    memset(w, 0, sizeof(w));
    const uint64_t big = ~0ull - 4;  // 2^64 - 5
    w[0x11] = big;                   // simple nodes
    w[0x13] = 7;                     // right degree 2
    w[0x00] = 3;
    w[0x10] = 2;                     // left only: a dead end
    w[KH_GRAPH_NODES] = big + 12;    // wraps to 7
    w[KH_GRAPH_KMERS] = ~0ull;
    g = kmerust::graph_summary(w);
    expect_u("big nodes", g.nodes, 7);
    expect_u("big kmers", g.kmers, ~0ull);
    expect_u("big simple", g.simple, big);
    expect_u("big deg_1_1", g.deg[1][1], big);
    expect_u("big deg_1_2", g.deg[1][2], 7);
    expect_u("big branching", g.branching, 7);
    expect_u("big isolated", g.isolated, 3);
    expect_u("big dead_ends", g.dead_ends, 2);
    expect_u("big arcs", g.arcs, big * 2 + 21 + 2);  // modulo 2^64

    // format_graph_line: masks 0x00, 0xFF, 0x12 at k = 1, 21, 32
    expect_line("k1 m00", 2, 1, 5, 0x00, "G\t5\t.\t.\n");
    expect_line("k1 mFF", 0, 1, 1, 0xFF, "A\t1\tACGT\tACGT\n");
    expect_line("k1 m12", 1, 1, 18446744073709551615ull, 0x12, "C\t18446744073709551615\tA\tC\n");
    const uint64_t k21 = 0x1B1B1B1B1B1ull >> 2;  // ACGT ACGT .. : 21 letters
    std::string s21;
    for (int i = 0; i < 21; ++i) s21.push_back("ACGT"[(k21 >> (2 * (20 - i))) & 3]);
    expect_line("k21 m00", k21, 21, 7, 0x00, s21 + "\t7\t.\t.\n");
    expect_line("k21 mFF", k21, 21, 7, 0xFF, s21 + "\t7\tACGT\tACGT\n");
    expect_line("k21 m12", k21, 21, 7, 0x12, s21 + "\t7\tA\tC\n");
    expect_line("k21 A", 0, 21, 1, 0x80, std::string(21, 'A') + "\t1\tT\t.\n");
    const uint64_t k32 = 0x1B1B1B1B1B1B1B1Bull;  // ACGT x 8
    expect_line("k32 m00", k32, 32, 2, 0x00, "ACGTACGTACGTACGTACGTACGTACGTACGT\t2\t.\t.\n");
    expect_line("k32 mFF", k32, 32, 2, 0xFF, "ACGTACGTACGTACGTACGTACGTACGTACGT\t2\tACGT\tACGT\n");
    expect_line("k32 m12", k32, 32, 2, 0x12, "ACGTACGTACGTACGTACGTACGTACGTACGT\t2\tA\tC\n");
    expect_line("k32 top", 0xC000000000000001ull, 32, 9, 0x69, "T" + std::string(30, 'A') + "C\t9\tCG\tAT\n");
    if (failures) return 1;
    printf("graph_check ok\n");
    return 0;
}
