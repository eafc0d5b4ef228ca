// unitig_bits_check.cpp -- the oriented-successor arithmetic of krust_amd/csrc/unitig_bits.h (what unitig.hip runs per node) compiled
// for the host: reads "k key" lines (decimal, canonical keys) from stdin and prints per line
//   pal spell+ spell-   then for sign 0, 1 and letter c = 0..3:   y ysign ypal self bit nb
// pal: kh_unitig_palindrome; spell: the k letters of kh_unitig_spell through kh_unitig_letter; y, ysign, ypal: kh_unitig_successor;
// self: kh_unitig_self_link; bit: the mask bit whose kh_unitig_letter_of_bit is c, counted over the whole mask; nb: the key
// kh_graph_neighbours has at that bit.  tests/test_unitig_links_ref.py compares them with string arithmetic.
#include <cinttypes>
#include <cstdio>
#include <string>

#include "../krust_amd/csrc/graph_bits.h"
#include "../krust_amd/csrc/unitig_bits.h"

int main() {
    unsigned k;
    uint64_t x;
    while (scanf("%u %" SCNu64, &k, &x) == 2) {
        if (k < 1 || k > 32) return 2;
        uint64_t nb[8];
        kh_graph_neighbours(x, k, nb);
        printf("%d", kh_unitig_palindrome(x, k) ? 1 : 0);
        for (uint32_t sign = 0; sign < 2; ++sign) {
            std::string s;
            for (uint32_t i = 0; i < k; ++i) s.push_back((char)kh_unitig_letter(kh_unitig_spell(x, k, sign), k, i));
            printf(" %s", s.c_str());
        }
        for (uint32_t sign = 0; sign < 2; ++sign)
            for (uint32_t c = 0; c < 4; ++c) {
                uint64_t y;
                uint32_t ysign;
                bool ypal;
                kh_unitig_successor(x, k, sign, c, &y, &ysign, &ypal);
                uint32_t bit = 99;
                for (uint32_t j = 0; j < 4; ++j)
                    if (kh_unitig_letter_of_bit(j, sign) == c) bit = j + 4 * sign;
                if (bit > 7 || kh_unitig_out_bits(1u << bit, sign) != (1u << (bit & 3u)) || kh_unitig_out_bits(1u << bit, sign ^ 1u) != 0) return 3;
                printf(" %" PRIu64 " %u %d %d %u %" PRIu64, y, ysign, ypal ? 1 : 0, kh_unitig_self_link(x, y) ? 1 : 0, bit, nb[bit]);
            }
        printf("\n");
    }
    return 0;
}
