// CPU check of the arena level 2's bin geometry (krust_amd/csrc/arena_bits.h), for every geometry the arena path can get:
// 32..1024 buckets per partition as powers of two (shift addresses) and every other count from 33 to 1023 (24-bit multiply-add),
// with the instance (512 / 768 / 1024 buckets), the payload size and the flush unit that batch.hip picks for it.
//   * (bucket, byte rank) -> address is injective into the bins, and is bucket x bin + rank in exact arithmetic;
//   * an address is aligned as its payload needs, lies inside the bins and never is the trash word, which lies behind them;
//   * the 16-byte words of a unit are where the flush reads them, 16-byte aligned, and the whole units of a bin lie inside it.
// Build: g++ -O1 -std=c++17 -o arena_bits_check arena_bits_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../krust_amd/csrc/arena_bits.h"

using namespace kh;

static int fails = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (fails < 20) {                     \
                printf("FAIL %s: ", #cond);       \
                printf(__VA_ARGS__);              \
                printf("\n");                     \
            }                                     \
            ++fails;                              \
        }                                         \
    } while (0)

// one geometry: nbk = the kernel instance, b2 buckets, pb payload bytes in the bins, unit_bytes per flushed unit
static void check_geometry(int nbk, uint32_t b2, bool pow2, uint32_t p2_bits, uint32_t pb, uint32_t unit_bytes) {
    const uint32_t total = arena_total_bytes(nbk), trash = arena_trash_addr(nbk);
    const uint32_t bin = pow2 ? arena_bin_bytes_pow2(nbk, p2_bits) : arena_bin_bytes(nbk, b2);
    const uint32_t sh = pow2 ? arena_bin_shift(nbk, p2_bits) : 0;
    auto addr = [&](uint32_t b, uint32_t r) { return pow2 ? arena_addr_pow2(b, sh, r) : arena_addr_mul(b, bin, r); };
    CHECK(b2 <= (uint32_t)nbk && b2 >= 32, "nbk %d b2 %u", nbk, b2);
    CHECK(bin % ARENA_WORD == 0 && bin >= unit_bytes + ARENA_WORD, "nbk %d b2 %u: bin of %u bytes, units of %u", nbk, b2, bin, unit_bytes);
    CHECK((uint64_t)bin * b2 <= total, "nbk %d b2 %u: bins of %u bytes beyond %u", nbk, b2, bin, total);
    CHECK(b2 < (1u << 24) && bin < (1u << 18), "nbk %d b2 %u bin %u: the 24-bit multiply", nbk, b2, bin);
    if (pow2) {
        CHECK(bin == 1u << sh, "nbk %d p2_bits %u: bin %u, shift %u", nbk, p2_bits, bin, sh);
        CHECK(bin == arena_bin_bytes(nbk, b2), "nbk %d b2 %u: the two bin sizes differ", nbk, b2);
    }
    // the trash word: behind every bin, aligned for either payload, inside the unit of room the kernel declares behind the bins
    CHECK(trash >= bin * b2 && trash % 8 == 0 && trash + pb <= total + unit_bytes, "nbk %d b2 %u: trash word at %u", nbk, b2, trash);
    std::vector<uint8_t> seen(total / 4, 0);
    for (uint32_t b = 0; b < b2; ++b) {
        for (uint32_t r = 0; r < bin; r += pb) {
            const uint32_t a = addr(b, r);
            CHECK((uint64_t)a == (uint64_t)b * bin + r, "nbk %d b2 %u: (%u, %u) -> %u", nbk, b2, b, r, a);
            CHECK(a % pb == 0 && a + pb <= total && a != trash, "nbk %d b2 %u: (%u, %u) -> %u", nbk, b2, b, r, a);
            if (a + pb > total) continue;
            for (uint32_t w = a / 4; w < (a + pb) / 4; ++w) {
                CHECK(!seen[w], "nbk %d b2 %u: (%u, %u) -> %u is taken", nbk, b2, b, r, a);
                seen[w] = 1;
            }
        }
        // the flush: unit u, 16-byte word w of bucket b's bin holds the payloads of byte ranks [u x unit + 16 w, + 16)
        const uint32_t first = addr(b, 0);
        for (uint32_t u = 0; u < bin / unit_bytes; ++u)
            for (uint32_t w = 0; w < unit_bytes / ARENA_WORD; ++w) {
                const uint32_t a = arena_unit_word(first, unit_bytes, u, w);
                CHECK(a % ARENA_WORD == 0 && a + ARENA_WORD <= first + bin, "nbk %d b2 %u: unit word (%u, %u, %u) at %u", nbk, b2, b, u, w, a);
                for (uint32_t i = 0; i < ARENA_WORD; i += pb)
                    CHECK(addr(b, u * unit_bytes + w * ARENA_WORD + i) == a + i, "nbk %d b2 %u: unit word (%u, %u, %u) byte %u", nbk, b2, b, u, w, i);
            }
        // ... and the lane's own word of unit 0 is the bin's address of byte rank 16 x lane (how the kernel forms it)
        for (uint32_t oi = 0; oi < 4; ++oi) CHECK(addr(b, oi * ARENA_WORD) == arena_unit_word(first, unit_bytes, 0, oi), "nbk %d b2 %u", nbk, b2);
    }
}

int main() {
    int n = 0;
    for (uint32_t pb : {4u, 8u}) {
        // powers of two: 32 .. 512 buckets in the 512-bucket instance (whole lines for 4-byte payloads), 1024 in its own
        for (uint32_t p2_bits = 5; p2_bits <= 10; ++p2_bits) {
            const int nbk = p2_bits == 10 ? 1024 : 512;
            check_geometry(nbk, 1u << p2_bits, true, p2_bits, pb, nbk == 1024 || pb == 8 ? 64 : 128), ++n;
        }
        // every other count, in the instance and with the unit batch.hip picks
        for (uint32_t b2 = 33; b2 < 1024; ++b2) {
            if ((b2 & (b2 - 1)) == 0) continue;
            const int nbk = b2 > 768 ? 1024 : b2 > 512 ? 768 : 512;
            const uint32_t unit = nbk == 1024 ? 64 : nbk == 768 ? (pb == 4 && b2 <= 682 ? 128 : 64) : (pb == 4 ? 128 : 64);
            check_geometry(nbk, b2, false, 0, pb, unit), ++n;
        }
    }
    if (fails) {
        printf("ARENA_BITS_FAILED %d\n", fails);
        return 1;
    }
    printf("ARENA_BITS_OK %d geometries\n", n);
    return 0;
}
