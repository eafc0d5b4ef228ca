// clip_host_check.cpp -- the pure host side of `kmerust clip` (krust_amd/host/kmerust_host.h): parse_clip_args on accepted and refused
// command lines, clip_stops -- the round loop's stop rule -- and clip_round_line, the stderr line of a round.  Pure host code with its
// own main: compiled and run by tests/test_clip_host.py (once more with -fsanitize=address,undefined), no device and no library needed.
#include <cstdio>
#include <string>
#include <vector>

#include "../krust_amd/host/kmerust_host.h"

using namespace kmerust;

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

int main() {
    {  // the defaults
        const ClipArgs c = parse_clip_args({"a.kmix"});
        expect_s("defaults error", c.error, "");
        expect_s("defaults index", c.index, "a.kmix");
        expect_u("defaults min_count", c.min_count, 1);
        expect_u("defaults rounds", c.rounds, 1);
        expect_u("defaults have_max_kmers", c.have_max_kmers, 0);
        expect_u("defaults format", (uint64_t)c.format, (uint64_t)OutputFormat::Fasta);
        expect_u("defaults flags", (uint64_t)(c.sorted || c.quiet || !c.save.empty()), 0);
    }
    {  // every option, in every spelling
        const ClipArgs c = parse_clip_args({"-m", "3", "--max-kmers=42", "x.kmix", "--rounds", "0", "-ftsv", "--sorted", "--save", "out.kmix", "-q"});
        expect_s("all error", c.error, "");
        expect_s("all index", c.index, "x.kmix");
        expect_u("all min_count", c.min_count, 3);
        expect_u("all max_kmers", c.max_kmers, 42);
        expect_u("all have_max_kmers", c.have_max_kmers, 1);
        expect_u("all rounds", c.rounds, 0);
        expect_u("all format", (uint64_t)c.format, (uint64_t)OutputFormat::Tsv);
        expect_u("all flags", (uint64_t)(c.sorted && c.quiet), 1);
        expect_s("all save", c.save, "out.kmix");
        const ClipArgs d = parse_clip_args({"--min-count=18446744073709551615", "--format", "histogram", "--max-kmers", "0", "--quiet", "--save=o", "i"});
        expect_s("long error", d.error, "");
        expect_u("long min_count", d.min_count, UINT64_MAX);
        expect_u("long max_kmers", d.max_kmers + (d.have_max_kmers ? 0 : 99), 0);
        expect_u("long format", (uint64_t)d.format, (uint64_t)OutputFormat::Histogram);
        expect_s("long save", d.save + "|" + d.index, "o|i");
        expect_u("json", (uint64_t)parse_clip_args({"i", "-f", "json"}).format, (uint64_t)OutputFormat::Json);
    }
    // refusals: the text behind "error: "
    expect_s("no index", parse_clip_args({}).error, "the following required arguments were not provided:\n  <INDEX>\n\nUsage: kmerust clip <INDEX>");
    expect_s("no index 2", parse_clip_args({"-m", "2"}).error, "the following required arguments were not provided:\n  <INDEX>\n\nUsage: kmerust clip <INDEX>");
    expect_s("two", parse_clip_args({"a", "b"}).error, "unexpected argument 'b' found");
    expect_s("unknown", parse_clip_args({"a", "--bubbles"}).error, "unexpected argument '--bubbles' found");
    expect_s("format", parse_clip_args({"a", "-f", "gfa"}).error, "invalid value 'gfa' for '--format <FORMAT>'\n  [possible values: fasta, tsv, json, histogram]");
    expect_s("format none", parse_clip_args({"a", "-f"}).error, "a value is required for '--format <FORMAT>' but none was supplied");
    expect_s("rounds none", parse_clip_args({"a", "--rounds"}).error, "a value is required for '--rounds <R>' but none was supplied");
    expect_s("digit", parse_clip_args({"a", "-m", "x"}).error, "invalid value 'x' for '--min-count <MIN_COUNT>': invalid digit found in string");
    expect_s("negative", parse_clip_args({"a", "--rounds=-1"}).error, "invalid value '-1' for '--rounds <R>': invalid digit found in string");
    expect_s("empty", parse_clip_args({"a", "--max-kmers="}).error, "invalid value '' for '--max-kmers <L>': invalid digit found in string");
    expect_s("large", parse_clip_args({"a", "--max-kmers", "18446744073709551616"}).error,
             "invalid value '18446744073709551616' for '--max-kmers <L>': number too large to fit in target type");
    // the stop rule
    expect_u("stop: clipped nothing", clip_stops(1, 0, 0), 1);
    expect_u("stop: clipped nothing, limit far", clip_stops(1, 9, 0), 1);
    expect_u("go: no limit", clip_stops(1000000, 0, 1), 0);
    expect_u("go: below the limit", clip_stops(2, 3, 7), 0);
    expect_u("stop: at the limit", clip_stops(3, 3, 7), 1);
    expect_u("stop: default one round", clip_stops(1, 1, UINT64_MAX), 1);
    // the stderr line
    const uint64_t w[KH_CLIP_WORDS] = {3541, 1157, 663, 1701, 2241, 229635, 255396, 3416};
    expect_s("line", clip_round_line(1, w), "1\t3541\t1157\t663\t1701\t229635\n");
    const uint64_t z[KH_CLIP_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    expect_s("line of nothing", clip_round_line(12, z), "12\t0\t0\t0\t0\t0\n");
    const uint64_t big[KH_CLIP_WORDS] = {UINT64_MAX, 1, 2, 3, 4, UINT64_MAX - 1, 6, 7};
    expect_s("line, large", clip_round_line(UINT64_MAX, big), "18446744073709551615\t18446744073709551615\t1\t2\t3\t18446744073709551614\n");
    if (failures) {
        printf("clip_host_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("clip_host_check ok\n");
    return 0;
}
