// cli_args_check.cpp -- the argument parser of `kmerust` (krust_amd/host/cli_args.h) and the commands' tables on top of it
// (parse_*_args in krust_amd/host/kmerust_host.h) on accepted and refused command lines.  Per command, in this order: the defaults,
// every spelling of every option, every refusal with its whole text, the first error in argv order, "-" as a positional, and the number
// parser at its edges and at every option's maximum.  Pure host code with its own main: compiled and run by tests/test_cli_args.py (once
// more with -fsanitize=address,undefined), no device and no library needed.
#include <cstdio>
#include <string>
#include <vector>

#include "../krust_amd/host/kmerust_host.h"

using namespace kmerust;
using A = std::vector<std::string>;

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

static const std::string U64 = "18446744073709551615", OVER = "18446744073709551616", NINES(20, '9');
static std::string digit(const std::string &v, const std::string &what) { return "invalid value '" + v + "' for '" + what + "': invalid digit found in string"; }
static std::string large(const std::string &v, const std::string &what) { return "invalid value '" + v + "' for '" + what + "': number too large to fit in target type"; }
static std::string needs(const std::string &what) { return "a value is required for '" + what + "' but none was supplied"; }
static std::string unexpected(const std::string &a) { return "unexpected argument '" + a + "' found"; }
static std::string possible(const std::string &v, const std::string &what, const std::string &list) {
    return "invalid value '" + v + "' for '" + what + "'\n  [possible values: " + list + "]";
}
static std::string missing(const std::string &names, const std::string &usage) {
    return "the following required arguments were not provided:\n" + names + "\n\nUsage: kmerust " + usage;
}
static A with(A base, const A &more) {
    base.insert(base.end(), more.begin(), more.end());
    return base;
}

// A number option of a command whose parser is `parse` and whose other arguments are `base`: the value `get` reads back at 0, at `max`
// and -- where max is 2^64 - 1 -- nowhere above; the refusals one above max, at 2^64, at 20 nines, and of what is no number.
template <class Parse, class Get>
static void check_number(const std::string &tag, Parse parse, const A &base, const std::string &key, const std::string &what, uint64_t max, Get get) {
    const auto at = [&](const std::string &v) { return parse(with(base, {key, v})); };
    expect_s(tag + " 0", at("0").error, "");
    expect_u(tag + " 0 value", get(at("0")), 0);
    expect_s(tag + " max", at(std::to_string(max)).error, "");
    expect_u(tag + " max value", get(at(std::to_string(max))), max);
    expect_u(tag + " leading zeros", get(at("007")), 7);
    if (max != UINT64_MAX) expect_s(tag + " max + 1", at(std::to_string(max + 1)).error, large(std::to_string(max + 1), what));
    if (max != UINT64_MAX) expect_s(tag + " 2^64 - 1", at(U64).error, large(U64, what));
    expect_s(tag + " 2^64", at(OVER).error, large(OVER, what));
    expect_s(tag + " 20 nines", at(NINES).error, large(NINES, what));
    for (const char *bad : {"", "-1", "+1", "1x", " 1", "000000000000000000001"}) expect_s(tag + " '" + bad + "'", at(bad).error, digit(bad, what));
    expect_s(tag + " no value", parse(with(base, {key})).error, needs(what));
}

static void check_parser() {
    uint64_t v = 99;
    expect_s("parse_u64 0", parse_u64("0", "N", UINT64_MAX, &v), "");
    expect_u("parse_u64 0 value", v, 0);
    expect_s("parse_u64 2^64 - 1", parse_u64(U64, "N", UINT64_MAX, &v), "");
    expect_u("parse_u64 2^64 - 1 value", v, UINT64_MAX);
    v = 5;
    expect_s("parse_u64 2^64", parse_u64(OVER, "N", UINT64_MAX, &v), large(OVER, "N"));
    expect_s("parse_u64 20 nines", parse_u64(NINES, "N", UINT64_MAX, &v), large(NINES, "N"));
    expect_s("parse_u64 max + 1", parse_u64("256", "N", 255, &v), large("256", "N"));
    for (const char *bad : {"", "-1", "+1", "1x"}) expect_s(std::string("parse_u64 '") + bad + "'", parse_u64(bad, "N", UINT64_MAX, &v), digit(bad, "N"));
    expect_u("parse_u64 leaves the target alone", v, 5);
    size_t c = 7;
    expect_s("parse_choice", parse_choice("b", "X", {"a", "b"}, &c), "");
    expect_u("parse_choice value", c, 1);
    expect_s("parse_choice refusal", parse_choice("B", "X", {"a", "b"}, &c), possible("B", "X", "a, b"));
}

static void check_count() {
    const CountArgs d = parse_count_args({"21"});
    expect_s("count defaults error", d.error, "");
    expect_s("count defaults path", d.path + "|" + d.save, "-|");
    expect_u("count defaults k", d.k, 21);
    expect_u("count defaults numbers", d.min_count * 10 + (uint64_t)(d.min_quality + 1) + d.devices.size(), 10);
    expect_u("count defaults formats", (uint64_t)d.format * 10 + (uint64_t)d.input_format, (uint64_t)OutputFormat::Fasta * 10 + (uint64_t)SequenceFormat::Auto);
    expect_u("count defaults flags", d.help || d.version || d.quiet || d.sorted, 0);

    const CountArgs a = parse_count_args({"-f", "tsv", "-i", "fastq", "-m", "3", "-Q", "20", "--save", "o.kmix", "--sorted", "--gpus", "3", "-q", "31", "x.fq"});
    expect_s("count short error", a.error, "");
    expect_s("count short texts", a.path + "|" + a.save, "x.fq|o.kmix");
    expect_u("count short numbers", a.k * 1000000 + a.min_count * 10000 + (uint64_t)a.min_quality * 100 + a.devices.size(), 31032003);
    expect_u("count short devices", (uint64_t)(a.devices[0] * 100 + a.devices[1] * 10 + a.devices[2]), 12);
    expect_u("count short formats", (uint64_t)a.format * 10 + (uint64_t)a.input_format, (uint64_t)OutputFormat::Tsv * 10 + (uint64_t)SequenceFormat::Fastq);
    expect_u("count short flags", a.quiet && a.sorted && !a.help && !a.version, 1);
    const CountArgs b = parse_count_args({"--format=json", "--input-format=fasta", "--min-count=4", "--min-quality=0", "--save=s", "--devices=0,2,5", "--quiet", "1", "-"});
    expect_s("count = error", b.error, "");
    expect_s("count = texts", b.path + "|" + b.save, "-|s");
    expect_u("count = numbers", b.k * 1000 + b.min_count * 100 + (uint64_t)b.min_quality * 10 + b.devices.size(), 1403);
    expect_u("count = devices", (uint64_t)(b.devices[0] * 100 + b.devices[1] * 10 + b.devices[2]), 25);
    expect_u("count = formats", (uint64_t)b.format * 10 + (uint64_t)b.input_format, (uint64_t)OutputFormat::Json * 10 + (uint64_t)SequenceFormat::Fasta);
    const CountArgs c = parse_count_args({"--format", "histogram", "--input-format", "auto", "--min-count", "5", "--min-quality", "255", "--devices", "7", "--gpus=1", "2"});
    expect_s("count long error", c.error, "");
    expect_u("count long numbers", c.min_count * 1000 + (uint64_t)c.min_quality, 5255);
    expect_u("count long: the later of --devices and --gpus", c.devices.size() * 10 + (uint64_t)c.devices[0], 10);
    expect_u("count long formats", (uint64_t)c.format * 10 + (uint64_t)c.input_format, (uint64_t)OutputFormat::Histogram * 10 + (uint64_t)SequenceFormat::Auto);
    const CountArgs e = parse_count_args({"-ffasta", "-ifastq", "-m6", "-Q7", "9"});
    expect_s("count attached error", e.error, "");
    expect_u("count attached", (uint64_t)e.format * 1000 + (uint64_t)e.input_format * 100 + e.min_count * 10 + (uint64_t)e.min_quality, 267);
    expect_u("count --gpus then --devices", parse_count_args({"5", "--gpus", "4", "--devices", "9"}).devices.size(), 1);
    for (const A &h : {A{"-h"}, A{"--help"}, A{"5", "--help", "--bogus"}, A{"-h", "-V"}}) {
        const CountArgs x = parse_count_args(h);
        expect_s("count help error", x.error, "");
        expect_u("count help", x.help && !x.version, 1);
    }
    for (const A &h : {A{"-V"}, A{"--version"}, A{"-V", "-h"}, A{"-f", "tsv", "--version", "-m", "x"}}) {
        const CountArgs x = parse_count_args(h);
        expect_s("count version error", x.error, "");
        expect_u("count version", x.version && !x.help, 1);
    }

    const std::string none = missing("  <K>", "<K> [PATH]");
    expect_s("count nothing", parse_count_args({}).error, none);
    expect_s("count no k", parse_count_args({"-q", "-m", "2"}).error, none);
    expect_s("count third", parse_count_args({"5", "a", "b"}).error, unexpected("b"));
    for (const char *u : {"--bogus", "--", "-5", "-x", "--sorted=1", "--quiet=1", "--help=1", "-qq", "-v", "--sequences", "--max-kmers", "--__batch-kb", "-c"})
        expect_s(std::string("count ") + u, parse_count_args({"5", u}).error, unexpected(u));
    expect_s("count k 0", parse_count_args({"0"}).error, "invalid value '0' for '<K>': k-mer length must be at least 1");
    expect_s("count k 33", parse_count_args({"33"}).error, "invalid value '33' for '<K>': k-mer length must be at most 32");
    expect_u("count k 32", parse_count_args({"32"}).k, 32);
    for (const char *k : {"abc", "", "-", "+5", "5x", "99999999999999999999"})
        expect_s(std::string("count k ") + k, parse_count_args({k, "x.fa"}).error, std::string("invalid value '") + k + "' for '<K>': '" + k + "' is not a valid number");
    expect_s("count k 19 nines", parse_count_args({"9999999999999999999"}).error, "invalid value '9999999999999999999' for '<K>': k-mer length must be at most 32");
    for (const char *key : {"-f", "--format"}) {
        expect_s("count format", parse_count_args({"5", key, "xml"}).error, possible("xml", "--format <FORMAT>", "fasta, tsv, json, histogram"));
        expect_s("count format none", parse_count_args({"5", key}).error, needs("--format <FORMAT>"));
    }
    expect_s("count format =", parse_count_args({"5", "-f=json"}).error, possible("=json", "--format <FORMAT>", "fasta, tsv, json, histogram"));
    expect_s("count format empty", parse_count_args({"5", "--format="}).error, possible("", "--format <FORMAT>", "fasta, tsv, json, histogram"));
    expect_s("count input format", parse_count_args({"5", "-i", "bam"}).error, possible("bam", "--input-format <INPUT_FORMAT>", "auto, fasta, fastq"));
    expect_s("count input format none", parse_count_args({"5", "--input-format"}).error, needs("--input-format <INPUT_FORMAT>"));
    expect_s("count save none", parse_count_args({"5", "--save"}).error, needs("--save <SAVE>"));
    expect_s("count gpus 0", parse_count_args({"5", "--gpus", "0"}).error, "invalid value '0' for '--gpus <N>': at least one GPU is needed");
    expect_s("count gpus 00", parse_count_args({"5", "--gpus", "00"}).error, "invalid value '0' for '--gpus <N>': at least one GPU is needed");
    expect_u("count gpus 64", parse_count_args({"5", "--gpus", "64"}).devices.size(), 64);
    expect_s("count gpus 65", parse_count_args({"5", "--gpus", "65"}).error, large("65", "--gpus <N>"));
    expect_s("count gpus 2^64 - 1", parse_count_args({"5", "--gpus", U64}).error, large(U64, "--gpus <N>"));
    expect_s("count gpus x", parse_count_args({"5", "--gpus=two"}).error, digit("two", "--gpus <N>"));
    expect_s("count gpus none", parse_count_args({"5", "--gpus"}).error, needs("--gpus <N>"));
    expect_u("count devices 1023", (uint64_t)parse_count_args({"5", "--devices", "0,1023"}).devices[1], 1023);
    expect_s("count devices 1024", parse_count_args({"5", "--devices", "0,1024"}).error, large("1024", "--devices <LIST>"));
    expect_s("count devices 2^64", parse_count_args({"5", "--devices", OVER}).error, large(OVER, "--devices <LIST>"));
    for (const char *l : {"", "0,", ",1", "0,,1"}) expect_s(std::string("count devices ") + l, parse_count_args({"5", "--devices", l}).error, digit("", "--devices <LIST>"));
    expect_s("count devices x", parse_count_args({"5", "--devices=0,x"}).error, digit("x", "--devices <LIST>"));
    expect_s("count devices none", parse_count_args({"5", "--devices"}).error, needs("--devices <LIST>"));

    expect_s("count first: option, unknown", parse_count_args({"-f", "xml", "--bogus"}).error, possible("xml", "--format <FORMAT>", "fasta, tsv, json, histogram"));
    expect_s("count first: unknown, option", parse_count_args({"--bogus", "-f", "xml"}).error, unexpected("--bogus"));
    expect_s("count first: two numbers", parse_count_args({"5", "-Q", "999", "-m", "x"}).error, large("999", "--min-quality <MIN_QUALITY>"));
    expect_s("count first: the walk before k", parse_count_args({"0", "-m", "x"}).error, digit("x", "--min-count <MIN_COUNT>"));
    expect_s("count first: the walk before the missing k", parse_count_args({"-m", "x"}).error, digit("x", "--min-count <MIN_COUNT>"));
    expect_s("count first: an error before --help", parse_count_args({"--bogus", "-h"}).error, unexpected("--bogus"));
    expect_u("count first: an error before --help is no help", parse_count_args({"--bogus", "-h"}).help, 0);

    expect_s("count - is stdin", parse_count_args({"5", "-"}).path, "-");
    expect_s("count - as k", parse_count_args({"-", "x.fa"}).error, "invalid value '-' for '<K>': '-' is not a valid number");
    expect_s("count a value may start with -", parse_count_args({"5", "--save", "-q"}).save, "-q");

    const A base = {"5", "x.fa"};
    check_number("count -m", parse_count_args, base, "-m", "--min-count <MIN_COUNT>", UINT64_MAX, [](const CountArgs &x) { return x.min_count; });
    check_number("count -Q", parse_count_args, base, "--min-quality", "--min-quality <MIN_QUALITY>", 255, [](const CountArgs &x) { return (uint64_t)x.min_quality; });
}

static void check_query_sequences() {
    const std::string usage = "query <INDEX> --sequences <PATH>";
    const QuerySequencesArgs d = parse_query_sequences_args({"i.kmix", "--sequences", "r.fa"});
    expect_s("qseq defaults error", d.error, "");
    expect_s("qseq defaults texts", d.index + "|" + d.path, "i.kmix|r.fa");
    expect_u("qseq defaults", (uint64_t)d.format + (uint64_t)d.input_format + (uint64_t)(d.min_quality + 1) + d.batch_bytes + d.quiet, 0);
    const QuerySequencesArgs a = parse_query_sequences_args({"-q", "-f", "profile", "-i", "fastq", "-Q", "20", "--__batch-kb", "4", "--sequences=r.fq", "i"});
    expect_s("qseq short error", a.error, "");
    expect_s("qseq short texts", a.index + "|" + a.path, "i|r.fq");
    expect_u("qseq short", (uint64_t)a.format * 1000 + (uint64_t)a.input_format * 100 + (uint64_t)a.min_quality + a.quiet, 1000 + 200 + 21);
    expect_u("qseq short batch", a.batch_bytes, 4096);
    const QuerySequencesArgs b = parse_query_sequences_args({"i", "--quiet", "--format=summary", "--input-format=fasta", "--min-quality=3", "--__batch-kb=1", "--sequences", "-"});
    expect_s("qseq = error", b.error, "");
    expect_s("qseq = path", b.path, "-");
    expect_u("qseq =", (uint64_t)b.format * 1000 + (uint64_t)b.input_format * 100 + (uint64_t)b.min_quality + b.quiet + b.batch_bytes, 100 + 4 + 1024);
    const QuerySequencesArgs c = parse_query_sequences_args({"i", "--format", "profile", "--input-format", "auto", "--min-quality", "9", "-fsummary", "-ifastq", "-Q7", "--sequences", ""});
    expect_s("qseq long and attached error", c.error, "");
    expect_u("qseq long and attached: the later wins", (uint64_t)c.format * 1000 + (uint64_t)c.input_format * 100 + (uint64_t)c.min_quality, 207);
    expect_s("qseq an empty path is a path", c.path, "");

    expect_s("qseq no index", parse_query_sequences_args({"--sequences", "r.fa"}).error, missing("  <INDEX>", usage));
    expect_s("qseq no path", parse_query_sequences_args({"i"}).error, missing("  --sequences <PATH>", usage));
    expect_s("qseq nothing", parse_query_sequences_args({}).error, missing("  <INDEX>", usage));
    expect_s("qseq two", parse_query_sequences_args({"i", "j", "--sequences", "r"}).error, unexpected("j"));
    for (const char *u : {"--bogus", "--", "-5", "-h", "--help", "-V", "--quiet=1", "--sorted", "-m", "--save", "-v"})
        expect_s(std::string("qseq ") + u, parse_query_sequences_args({"i", "--sequences", "r", u}).error, unexpected(u));
    expect_s("qseq format", parse_query_sequences_args({"i", "-f", "tsv"}).error, possible("tsv", "--format <FORMAT>", "summary, profile"));
    expect_s("qseq format none", parse_query_sequences_args({"i", "-f"}).error, needs("--format <FORMAT>"));
    expect_s("qseq input format", parse_query_sequences_args({"i", "--input-format=bam"}).error, possible("bam", "--input-format <INPUT_FORMAT>", "auto, fasta, fastq"));
    expect_s("qseq input format none", parse_query_sequences_args({"i", "-i"}).error, needs("--input-format <INPUT_FORMAT>"));
    expect_s("qseq sequences none", parse_query_sequences_args({"i", "--sequences"}).error, needs("--sequences <PATH>"));
    expect_s("qseq first: option, unknown", parse_query_sequences_args({"-f", "x", "--bogus"}).error, possible("x", "--format <FORMAT>", "summary, profile"));
    expect_s("qseq first: unknown, option", parse_query_sequences_args({"--bogus", "-f", "x"}).error, unexpected("--bogus"));
    expect_s("qseq first: the walk before what is missing", parse_query_sequences_args({"-Q", "x"}).error, digit("x", "--min-quality <MIN_QUALITY>"));
    expect_s("qseq - as index", parse_query_sequences_args({"-", "--sequences", "r"}).index, "-");
    const A base = {"i", "--sequences", "r"};
    check_number("qseq -Q", parse_query_sequences_args, base, "-Q", "--min-quality <MIN_QUALITY>", 255, [](const QuerySequencesArgs &x) { return (uint64_t)x.min_quality; });
    check_number("qseq batch", parse_query_sequences_args, base, "--__batch-kb", "--__batch-kb <N>", 1u << 22, [](const QuerySequencesArgs &x) { return (uint64_t)x.batch_bytes >> 10; });
}

static void check_filter() {
    const std::string usage = "filter <INDEX> <PATH>";
    const FilterArgs d = parse_filter_args({"i.kmix", "r.fa"});
    expect_s("filter defaults error", d.error, "");
    expect_s("filter defaults texts", d.index + "|" + d.path, "i.kmix|r.fa");
    expect_u("filter defaults", (uint64_t)d.input_format + (uint64_t)(d.min_quality + 1) + d.batch_bytes + d.quiet + d.rule.invert, 0);
    expect_u("filter defaults rule", d.rule.min_count * 10 + d.rule.min_kmers + (d.rule.max_count == 0xFFFFFFFEu ? 0 : 5) + (d.rule.min_fraction == 0.0 ? 0 : 7), 11);
    const FilterArgs a = parse_filter_args({"-q", "-v", "-i", "fastq", "-Q", "20", "--min-count", "2", "--max-count", "9", "--min-kmers", "4", "--min-fraction", "0.5", "--__batch-kb", "4", "i", "-"});
    expect_s("filter short error", a.error, "");
    expect_s("filter short texts", a.index + "|" + a.path, "i|-");
    expect_u("filter short", (uint64_t)a.input_format * 100 + (uint64_t)a.min_quality + a.quiet + a.rule.invert, 222);
    expect_u("filter short rule", a.rule.min_count * 100 + a.rule.max_count * 10 + a.rule.min_kmers + (a.rule.min_fraction == 0.5 ? 0 : 1000), 294);
    expect_u("filter short batch", a.batch_bytes, 4096);
    const FilterArgs b = parse_filter_args({"i", "r", "--quiet", "--invert", "--input-format=fasta", "--min-quality=3", "--min-count=5", "--max-count=6", "--min-kmers=7", "--min-fraction=1", "--__batch-kb=1"});
    expect_s("filter = error", b.error, "");
    expect_u("filter =", (uint64_t)b.input_format * 100 + (uint64_t)b.min_quality + b.quiet + b.rule.invert, 105);
    expect_u("filter = rule", b.rule.min_count * 100 + b.rule.max_count * 10 + b.rule.min_kmers + (b.rule.min_fraction == 1.0 ? 0 : 1000), 567);
    const FilterArgs c = parse_filter_args({"i", "r", "--input-format", "auto", "--min-quality", "9", "-ifastq", "-Q7", "--min-fraction", "1e-3"});
    expect_s("filter long and attached error", c.error, "");
    expect_u("filter long and attached: the later wins", (uint64_t)c.input_format * 100 + (uint64_t)c.min_quality + (c.rule.min_fraction == 1e-3 ? 0 : 1000), 207);

    expect_s("filter nothing", parse_filter_args({}).error, missing("  <INDEX>\n  <PATH>", usage));
    expect_s("filter no path", parse_filter_args({"i", "-v"}).error, missing("  <PATH>", usage));
    expect_s("filter three", parse_filter_args({"i", "r", "s"}).error, unexpected("s"));
    for (const char *u : {"--bogus", "--", "-5", "-h", "--help", "-V", "--invert=1", "--sorted", "-m", "-f", "--save"})
        expect_s(std::string("filter ") + u, parse_filter_args({"i", "r", u}).error, unexpected(u));
    expect_s("filter input format", parse_filter_args({"i", "r", "-i", "bam"}).error, possible("bam", "--input-format <INPUT_FORMAT>", "auto, fasta, fastq"));
    expect_s("filter input format none", parse_filter_args({"i", "r", "-i"}).error, needs("--input-format <INPUT_FORMAT>"));
    for (const char *f : {"half", "", "0.5x", "nan", "1e", "inf", "0x1"}) expect_s(std::string("filter fraction ") + f, parse_filter_args({"i", "r", "--min-fraction", f}).error,
                                                                                     std::string("invalid value '") + f + "' for '--min-fraction <F>': invalid float literal");
    for (const char *f : {"1.5", "-0.5", "1e3"}) expect_s(std::string("filter fraction ") + f, parse_filter_args({"i", "r", "--min-fraction", f}).error,
                                                            std::string("invalid value '") + f + "' for '--min-fraction <F>': must be between 0 and 1");
    expect_s("filter fraction none", parse_filter_args({"i", "r", "--min-fraction"}).error, needs("--min-fraction <F>"));
    expect_s("filter first: option, unknown", parse_filter_args({"--min-count", "x", "--bogus"}).error, digit("x", "--min-count <LO>"));
    expect_s("filter first: unknown, option", parse_filter_args({"--bogus", "--min-count", "x"}).error, unexpected("--bogus"));
    expect_s("filter first: the walk before what is missing", parse_filter_args({"i", "--min-fraction", "2"}).error, "invalid value '2' for '--min-fraction <F>': must be between 0 and 1");
    expect_s("filter - as index", parse_filter_args({"-", "-"}).index, "-");
    const A base = {"i", "r"};
    check_number("filter -Q", parse_filter_args, base, "-Q", "--min-quality <MIN_QUALITY>", 255, [](const FilterArgs &x) { return (uint64_t)x.min_quality; });
    check_number("filter lo", parse_filter_args, base, "--min-count", "--min-count <LO>", 0xFFFFFFFFull, [](const FilterArgs &x) { return (uint64_t)x.rule.min_count; });
    check_number("filter hi", parse_filter_args, base, "--max-count", "--max-count <HI>", 0xFFFFFFFFull, [](const FilterArgs &x) { return (uint64_t)x.rule.max_count; });
    check_number("filter kmers", parse_filter_args, base, "--min-kmers", "--min-kmers <N>", UINT64_MAX, [](const FilterArgs &x) { return x.rule.min_kmers; });
    check_number("filter batch", parse_filter_args, base, "--__batch-kb", "--__batch-kb <N>", 1u << 22, [](const FilterArgs &x) { return (uint64_t)x.batch_bytes >> 10; });
}

static void check_two_indexes() {
    const TwoIndexArgs d = parse_compare_args({"a", "b"});
    expect_s("compare defaults error", d.error, "");
    expect_s("compare defaults texts", d.index_a + "|" + d.index_b + "|" + d.save + "|" + d.op_name, "a|b||");
    expect_u("compare defaults", d.min_a * 100 + d.min_b * 10 + d.min_count + d.quiet + d.json + d.sorted + d.op, 111);
    const TwoIndexArgs a = parse_compare_args({"-q", "--min-count-a", "2", "--min-count-b=3", "-f", "json", "a", "-"});
    expect_s("compare all error", a.error, "");
    expect_s("compare all texts", a.index_a + "|" + a.index_b, "a|-");
    expect_u("compare all", a.min_a * 100 + a.min_b * 10 + a.quiet + a.json, 232);
    expect_u("compare --format=tsv", parse_compare_args({"a", "b", "--quiet", "--min-count-a=4", "--min-count-b", "5", "--format=tsv"}).json, 0);
    expect_u("compare -fjson, --format tsv", parse_compare_args({"a", "b", "-fjson", "--format", "tsv"}).json, 0);
    expect_u("compare --format json", parse_compare_args({"a", "b", "--format", "json"}).json, 1);
    const std::string cu = "compare <INDEX_A> <INDEX_B>";
    expect_s("compare nothing", parse_compare_args({}).error, missing("  <INDEX_A>\n  <INDEX_B>", cu));
    expect_s("compare one", parse_compare_args({"a", "-q"}).error, missing("  <INDEX_B>", cu));
    expect_s("compare three", parse_compare_args({"a", "b", "c"}).error, unexpected("c"));
    for (const char *u : {"--bogus", "--", "-5", "-h", "--help", "-V", "--quiet=1", "--sorted", "-m", "-c", "--calc", "--save", "--min-count"})
        expect_s(std::string("compare ") + u, parse_compare_args({"a", "b", u}).error, unexpected(u));
    expect_s("compare format", parse_compare_args({"a", "b", "-f", "fasta"}).error, possible("fasta", "--format <FORMAT>", "tsv, json"));
    expect_s("compare format none", parse_compare_args({"a", "b", "--format"}).error, needs("--format <FORMAT>"));
    expect_s("compare first: option, unknown", parse_compare_args({"-f", "x", "--bogus"}).error, possible("x", "--format <FORMAT>", "tsv, json"));
    expect_s("compare first: unknown, option", parse_compare_args({"--bogus", "-f", "x"}).error, unexpected("--bogus"));
    expect_s("compare - as index", parse_compare_args({"-", "-"}).index_a, "-");
    const A cbase = {"a", "b"};
    check_number("compare a", parse_compare_args, cbase, "--min-count-a", "--min-count-a <N>", UINT64_MAX, [](const TwoIndexArgs &x) { return x.min_a; });
    check_number("compare b", parse_compare_args, cbase, "--min-count-b", "--min-count-b <N>", UINT64_MAX, [](const TwoIndexArgs &x) { return x.min_b; });

    const TwoIndexArgs e = parse_combine_args({"union", "a", "b"});
    expect_s("combine defaults error", e.error, "");
    expect_s("combine defaults texts", e.index_a + "|" + e.index_b + "|" + e.save + "|" + e.op_name, "a|b||union");
    expect_u("combine defaults", e.min_a * 100 + e.min_b * 10 + e.min_count + e.quiet + e.json + e.sorted, 111);
    expect_u("combine defaults op, calc, format", e.op * 100 + e.calc * 10 + (uint64_t)e.format, KH_SET_UNION * 100 + KH_CALC_SUM * 10 + (uint64_t)OutputFormat::Fasta);
    const TwoIndexArgs f = parse_combine_args({"-q", "-c", "min", "-m", "7", "-f", "tsv", "--save", "o", "--sorted", "--min-count-a", "2", "--min-count-b", "3", "intersect", "a", "-"});
    expect_s("combine short error", f.error, "");
    expect_s("combine short texts", f.index_a + "|" + f.index_b + "|" + f.save + "|" + f.op_name, "a|-|o|intersect");
    expect_u("combine short", f.min_a * 100 + f.min_b * 10 + f.min_count + f.quiet + f.sorted, 239);
    expect_u("combine short op, calc, format", f.op * 100 + f.calc * 10 + (uint64_t)f.format, KH_SET_INTERSECT * 100 + KH_CALC_MIN * 10 + (uint64_t)OutputFormat::Tsv);
    const TwoIndexArgs g = parse_combine_args({"subtract", "--calc=max", "--min-count=8", "--format=json", "--save=p", "--quiet", "a", "b"});
    expect_s("combine = error", g.error, "");
    expect_u("combine = op, calc, format", g.op * 100 + g.calc * 10 + (uint64_t)g.format, KH_SET_SUBTRACT * 100 + KH_CALC_MAX * 10 + (uint64_t)OutputFormat::Json);
    expect_s("combine = save", g.save, "p");
    expect_u("combine = min_count", g.min_count, 8);
    const TwoIndexArgs h = parse_combine_args({"count-subtract", "--calc", "left", "--min-count", "9", "--format", "histogram", "a", "b"});
    expect_u("combine long op, calc, format", h.op * 100 + h.calc * 10 + (uint64_t)h.format, KH_SET_COUNT_SUBTRACT * 100 + KH_CALC_LEFT * 10 + (uint64_t)OutputFormat::Histogram);
    expect_u("combine long min_count", h.min_count, 9);
    const TwoIndexArgs i = parse_combine_args({"union", "-cright", "-m2", "-ffasta", "a", "b"});
    expect_u("combine attached", i.calc * 100 + i.min_count * 10 + (uint64_t)i.format, KH_CALC_RIGHT * 100 + 20);
    expect_u("combine -c sum", parse_combine_args({"union", "a", "b", "-c", "sum"}).calc, KH_CALC_SUM);
    const std::string bu = "combine <OP> <INDEX_A> <INDEX_B>", ops = "intersect, union, subtract, count-subtract";
    expect_s("combine nothing", parse_combine_args({}).error, missing("  <OP>\n  <INDEX_A>\n  <INDEX_B>", bu));
    expect_s("combine op only", parse_combine_args({"union"}).error, missing("  <INDEX_A>\n  <INDEX_B>", bu));
    expect_s("combine one index", parse_combine_args({"union", "a"}).error, missing("  <INDEX_B>", bu));
    expect_s("combine four", parse_combine_args({"union", "a", "b", "c"}).error, unexpected("c"));
    expect_s("combine op", parse_combine_args({"merge", "a", "b"}).error, possible("merge", "<OP>", ops));
    expect_s("combine op before what is missing", parse_combine_args({"merge"}).error, possible("merge", "<OP>", ops));
    expect_s("combine op after the walk", parse_combine_args({"merge", "a", "b", "c"}).error, unexpected("c"));
    expect_s("combine op after the walk 2", parse_combine_args({"merge", "-f", "x"}).error, possible("x", "--format <FORMAT>", "fasta, tsv, json, histogram"));
    expect_s("combine - as op", parse_combine_args({"-", "a", "b"}).error, possible("-", "<OP>", ops));
    for (const char *u : {"--bogus", "--", "-5", "-h", "--help", "-V", "--quiet=1", "--sorted=1", "--gpus", "-i"})
        expect_s(std::string("combine ") + u, parse_combine_args({"union", "a", "b", u}).error, unexpected(u));
    expect_s("combine format", parse_combine_args({"union", "a", "b", "-f", "summary"}).error, possible("summary", "--format <FORMAT>", "fasta, tsv, json, histogram"));
    expect_s("combine format none", parse_combine_args({"union", "a", "b", "-f"}).error, needs("--format <FORMAT>"));
    expect_s("combine calc", parse_combine_args({"union", "a", "b", "-c", "avg"}).error, possible("avg", "--calc <CALC>", "min, max, sum, left, right"));
    expect_s("combine calc none", parse_combine_args({"union", "a", "b", "--calc"}).error, needs("--calc <CALC>"));
    expect_s("combine save none", parse_combine_args({"union", "a", "b", "--save"}).error, needs("--save <SAVE>"));
    expect_s("combine first: option, unknown", parse_combine_args({"-c", "x", "--bogus"}).error, possible("x", "--calc <CALC>", "min, max, sum, left, right"));
    expect_s("combine first: unknown, option", parse_combine_args({"--bogus", "-c", "x"}).error, unexpected("--bogus"));
    const A bbase = {"union", "a", "b"};
    check_number("combine a", parse_combine_args, bbase, "--min-count-a", "--min-count-a <N>", UINT64_MAX, [](const TwoIndexArgs &x) { return x.min_a; });
    check_number("combine b", parse_combine_args, bbase, "--min-count-b", "--min-count-b <N>", UINT64_MAX, [](const TwoIndexArgs &x) { return x.min_b; });
    check_number("combine -m", parse_combine_args, bbase, "-m", "--min-count <MIN_COUNT>", UINT64_MAX, [](const TwoIndexArgs &x) { return x.min_count; });
}

// graph, unitigs and gfa: <INDEX>, -m, -f with the command's own list, and --sorted for graph alone
template <class Parse>
static void check_index_command(const std::string &cmd, Parse parse, const std::vector<std::string> &formats, bool sorted_ok) {
    std::string list;
    for (size_t i = 0; i < formats.size(); ++i) list += (i ? ", " : "") + formats[i];
    const IndexArgs d = parse({"i.kmix"});
    expect_s(cmd + " defaults error", d.error, "");
    expect_s(cmd + " defaults index", d.index, "i.kmix");
    expect_u(cmd + " defaults", d.min_count * 10 + d.format + d.sorted, 10);
    for (size_t i = 0; i < formats.size(); ++i) {
        expect_u(cmd + " -f " + formats[i], parse({"i", "-f", formats[i]}).format, i);
        expect_u(cmd + " -f" + formats[i], parse({"-f" + formats[i], "i"}).format, i);
        expect_u(cmd + " --format " + formats[i], parse({"--format", formats[i], "i"}).format, i);
        expect_u(cmd + " --format=" + formats[i], parse({"i", "--format=" + formats[i]}).format, i);
    }
    expect_u(cmd + " -m 3", parse({"i", "-m", "3"}).min_count, 3);
    expect_u(cmd + " -m3", parse({"-m3", "i"}).min_count, 3);
    expect_u(cmd + " --min-count 3", parse({"--min-count", "3", "i"}).min_count, 3);
    expect_u(cmd + " --min-count=3", parse({"i", "--min-count=3"}).min_count, 3);
    if (sorted_ok) expect_u(cmd + " --sorted", parse({"i", "--sorted"}).sorted, 1);
    else expect_s(cmd + " --sorted", parse({"i", "--sorted"}).error, unexpected("--sorted"));
    expect_s(cmd + " nothing", parse({}).error, missing("  <INDEX>", cmd + " <INDEX>"));
    expect_s(cmd + " no index", parse({"-m", "2"}).error, missing("  <INDEX>", cmd + " <INDEX>"));
    expect_s(cmd + " two", parse({"i", "j"}).error, unexpected("j"));
    for (const char *u : {"--bogus", "--", "-5", "-q", "--quiet", "-h", "--help", "-V", "--sorted=1", "--save", "--rounds", "-i"})
        expect_s(cmd + " " + u, parse({"i", u}).error, unexpected(u));
    expect_s(cmd + " format", parse({"i", "-f", "xml"}).error, possible("xml", "--format <FORMAT>", list));
    expect_s(cmd + " format none", parse({"i", "--format"}).error, needs("--format <FORMAT>"));
    expect_s(cmd + " first: option, unknown", parse({"-f", "xml", "--bogus"}).error, possible("xml", "--format <FORMAT>", list));
    expect_s(cmd + " first: unknown, option", parse({"--bogus", "-f", "xml"}).error, unexpected("--bogus"));
    expect_s(cmd + " first: two options", parse({"-m", "x", "-f", "xml"}).error, digit("x", "--min-count <MIN_COUNT>"));
    expect_s(cmd + " first: the walk before what is missing", parse({"-f", "xml"}).error, possible("xml", "--format <FORMAT>", list));
    expect_s(cmd + " - as index", parse({"-"}).index, "-");
    expect_s(cmd + " - as index, no error", parse({"-"}).error, "");
    check_number(cmd + " -m", parse, {"i"}, "--min-count", "--min-count <MIN_COUNT>", UINT64_MAX, [](const IndexArgs &x) { return x.min_count; });
}

static void check_clip() {  // (tests/clip_host_check.cpp has the rest)
    const A base = {"i"};
    check_number("clip -m", parse_clip_args, base, "-m", "--min-count <MIN_COUNT>", UINT64_MAX, [](const ClipArgs &x) { return x.min_count; });
    check_number("clip max-kmers", parse_clip_args, base, "--max-kmers", "--max-kmers <L>", UINT64_MAX, [](const ClipArgs &x) { return x.max_kmers; });
    check_number("clip rounds", parse_clip_args, base, "--rounds", "--rounds <R>", UINT64_MAX, [](const ClipArgs &x) { return x.rounds; });
    expect_u("clip have_max_kmers", parse_clip_args({"i", "--max-kmers", "0"}).have_max_kmers, 1);
    expect_u("clip have_max_kmers after a refusal", parse_clip_args({"i", "--max-kmers", "x"}).have_max_kmers, 0);
    for (const char *u : {"--", "-5", "-h", "--help", "-V", "--sorted=1", "--quiet=1", "-i", "-c"}) expect_s(std::string("clip ") + u, parse_clip_args({"i", u}).error, unexpected(u));
    expect_s("clip save none", parse_clip_args({"i", "--save"}).error, needs("--save <SAVE>"));
    expect_s("clip first: option, unknown", parse_clip_args({"-f", "gfa", "--bogus"}).error, possible("gfa", "--format <FORMAT>", "fasta, tsv, json, histogram"));
    expect_s("clip first: unknown, option", parse_clip_args({"--bogus", "-f", "gfa"}).error, unexpected("--bogus"));
    expect_s("clip - as index", parse_clip_args({"-"}).index, "-");
    expect_u("clip -ftsv --format=json --format histogram", (uint64_t)parse_clip_args({"i", "-ftsv", "--format=json", "--format", "histogram"}).format, (uint64_t)OutputFormat::Histogram);
}

int main() {
    // a format is stored as its position in the list of spellings: the lists are in the order of the enums
    expect_u("OutputFormat", (uint64_t)OutputFormat::Fasta * 1000 + (uint64_t)OutputFormat::Tsv * 100 + (uint64_t)OutputFormat::Json * 10 + (uint64_t)OutputFormat::Histogram, 123);
    expect_u("SequenceFormat", (uint64_t)SequenceFormat::Auto * 100 + (uint64_t)SequenceFormat::Fasta * 10 + (uint64_t)SequenceFormat::Fastq, 12);
    expect_u("ProfileFormat", (uint64_t)ProfileFormat::Summary * 10 + (uint64_t)ProfileFormat::Profile, 1);
    expect_u("GraphFormat", (uint64_t)GraphFormat::Summary * 100 + (uint64_t)GraphFormat::Tsv * 10 + (uint64_t)GraphFormat::Json, 12);
    expect_u("UnitigFormat", (uint64_t)UnitigFormat::Fasta * 10 + (uint64_t)UnitigFormat::Summary, 1);
    expect_u("GfaFormat", (uint64_t)GfaFormat::Gfa * 10 + (uint64_t)GfaFormat::Summary, 1);
    check_parser();
    check_count();
    check_query_sequences();
    check_filter();
    check_two_indexes();
    check_index_command("graph", parse_graph_args, {"summary", "tsv", "json"}, true);
    check_index_command("unitigs", parse_unitigs_args, {"fasta", "summary"}, false);
    check_index_command("gfa", parse_gfa_args, {"gfa", "summary"}, false);
    check_clip();
    if (failures) {
        printf("cli_args_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("cli_args_check ok\n");
    return 0;
}
