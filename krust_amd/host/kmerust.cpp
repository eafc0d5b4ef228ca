// kmerust.cpp -- the `kmerust` command line over the HIP path.
// Mirrors src/cli.rs:33-144 (flags, defaults, parse_k messages) and src/main.rs:34-299 (banner on
// stderr unless --quiet, exit 1 on a missing file, warnings for -Q with FASTA / stdin, --save,
// `query`).  Colour escapes are not reproduced (cosmetic).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include <algorithm>
#include <unordered_map>
#include <vector>

#include "kmerust_host.h"

#include <chrono>
#include <unistd.h>

namespace kmerust {

static const char *USAGE =
    "Usage: kmerust [OPTIONS] <K> [PATH]\n"
    "       kmerust query <INDEX> <KMER>\n"
    "       kmerust query <INDEX> --sequences <PATH> [-i <INPUT_FORMAT>] [-Q <MIN_QUALITY>] [-f summary|profile] [-q]\n"
    "       kmerust filter <INDEX> <PATH> [-i <INPUT_FORMAT>] [-Q <MIN_QUALITY>] [--min-count <LO>] [--max-count <HI>]\n"
    "                      [--min-kmers <N>] [--min-fraction <F>] [-v] [-q]\n"
    "       kmerust compare <INDEX_A> <INDEX_B> [--min-count-a <N>] [--min-count-b <N>] [-f tsv|json]\n"
    "       kmerust combine <intersect|union|subtract|count-subtract> <INDEX_A> <INDEX_B> [-c min|max|sum|left|right]\n"
    "                       [--min-count-a <N>] [--min-count-b <N>] [-m <MIN_COUNT>] [-f <FORMAT>] [--save <SAVE>] [--sorted] [-q]\n"
    "       kmerust graph <INDEX> [-m <MIN_COUNT>] [-f summary|tsv|json] [--sorted]\n"
    "       kmerust unitigs <INDEX> [-m <MIN_COUNT>] [-f fasta|summary]\n"
    "       kmerust gfa <INDEX> [-m <MIN_COUNT>] [-f gfa|summary]\n"
    "       kmerust clip <INDEX> [-m <MIN_COUNT>] [--max-kmers <L>] [--rounds <R>] [-f <FORMAT>] [--save <SAVE>] [--sorted] [-q]\n"
    "\n"
    "Arguments:\n"
    "  <K>     K-mer length (1-32)\n"
    "  [PATH]  Path to a FASTA/FASTQ file (use '-' or omit for stdin) [default: -]\n"
    "\n"
    "Options:\n"
    "  -f, --format <FORMAT>              Output format [default: fasta] [possible values: fasta, tsv, json, histogram]\n"
    "  -m, --min-count <MIN_COUNT>        Minimum count threshold [default: 1]\n"
    "  -q, --quiet                        Suppress informational output\n"
    "  -i, --input-format <INPUT_FORMAT>  Input file format [default: auto] [possible values: auto, fasta, fastq]\n"
    "      --save <SAVE>                  Save k-mer counts to an index file (.kmix, .kmix.gz)\n"
    "  -Q, --min-quality <MIN_QUALITY>    Minimum Phred quality score (0-93) for FASTQ bases\n"
    "      --gpus <N>                     Count on the first N GPUs of the node (RCCL merge of the per-GPU tables) [default: 1]\n"
    "      --devices <LIST>               The same with explicit HIP device ordinals, e.g. 0,2,5\n"
    "      --sorted                       Records (and the pairs of --save) in ascending k-mer order, sorted on the device:\n"
    "                                     the same input gives the same bytes.  Changes nothing for -f histogram\n"
    "\n"
    "query --sequences: the index's count of the k-mer at every base of the sequences in <PATH>, one line per record.\n"
    "  -f summary (default)  {record}\\t{windows}\\t{present}\\t{min}\\t{max}\\t{sum}\n"
    "  -f profile            one count per window start, '-' where there is no k-mer (N, soft mask, low quality)\n"
    "\n"
    "filter: the records of <PATH> with at least N k-mers (and a share F of their k-mers) whose count in the index is in LO..HI,\n"
    "  written as they were read (FASTA or FASTQ); {records}\\t{kept} on stderr.\n"
    "      --min-count <LO>               Lowest count that is in range [default: 1]\n"
    "      --max-count <HI>               Highest count that is in range [default: 4294967294]\n"
    "      --min-kmers <N>                K-mers in range a record needs [default: 1]\n"
    "      --min-fraction <F>             ... and their share of the record's k-mers, 0-1 [default: 0]\n"
    "  -v, --invert                       Write the records the rule drops instead\n"
    "\n"
    "compare: two indexes set against each other on the device; one line per number: distinct_a, distinct_b, shared, sum_a, sum_b,\n"
    "  shared_sum_a, shared_sum_b, sum_min, then jaccard, containment_a, containment_b, bray_curtis (nan where a divisor is 0).\n"
    "combine: a set operation of two indexes, written like a count (-f, -m, --save): intersect and union give a k-mer of both\n"
    "  indexes the count -c says [default: sum]; subtract keeps the k-mers of A that B lacks; count-subtract keeps count A - count B > 0.\n"
    "      --min-count-a <N>              A k-mer of A below this count is taken as absent [default: 1]\n"
    "      --min-count-b <N>              ... and of B [default: 1]\n"
    "\n"
    "graph: the de Bruijn graph of the index's k-mers with a count of at least -m: which of the four possible successors and\n"
    "  predecessors of each k-mer (of its canonical string) are there too, computed on the device.\n"
    "  -f summary (default)  one {name}\\t{value} line each: nodes, kmers, arcs, isolated, dead_ends, branching, simple, and the 25\n"
    "                        deg_<l>_<r> (nodes of left degree l and right degree r); -f json: the same as one object\n"
    "  -f tsv                {kmer}\\t{count}\\t{left}\\t{right} per node: the letters that extend it, '.' for none (--sorted:\n"
    "                        in ascending k-mer order)\n"
    "\n"
    "unitigs: the maximal non-branching paths of that graph, built on the device, in ascending order of their first k-mers.\n"
    "  -f fasta (default)    >{i} LN:i:{bases} KC:i:{count sum} km:f:{mean count}, ' CR:i:1' on a circular one, then the sequence\n"
    "  -f summary            one {name}\\t{value} line each: unitigs, kmers, bases, circular, longest, n50\n"
    "\n"
    "gfa: those unitigs and the links between their ends, built on the device, as GFA 1.0.\n"
    "  -f gfa (default)      H\\tVN:Z:1.0, then S\\t{i}\\t{sequence} with the tags of unitigs -f fasta, then per link, in ascending\n"
    "                        order, L\\t{from}\\t{+|-}\\t{to}\\t{+|-}\\t{k-1}M\n"
    "  -f summary            one {name}\\t{value} line each: unitigs, links, self_links, dead_ends, isolated, tips\n"
    "\n"
    "clip: tip clipping of that graph on the device, written like a count (-f, -m, --save, --sorted): a unitig of at most L k-mers\n"
    "  with exactly one dead end goes when, at every link out of its other end, a longer or better covered branch enters the same\n"
    "  place.  One round decides from the graph as it is; the k-mers of the surviving unitigs are the next round's index.\n"
    "      --max-kmers <L>                The longest unitig, in k-mers, that can be clipped [default: k]\n"
    "      --rounds <R>                   Rounds to run at most; 0: until a round clips nothing [default: 1]\n"
    "  stderr, unless -q: round\\tunitigs\\tcandidates\\tclipped\\tclipped_kmers\\tkept_kmers, one line per round\n"
    "\n"
    "  -h, --help                         Print help\n"
    "  -V, --version                      Print version\n";

[[noreturn]] static void usage_error(const std::string &msg) {
    fprintf(stderr, "error: %s\n\nFor more information, try '--help'.\n", msg.c_str());
    exit(2);  // clap's usage-error status
}

// parse_k, src/cli.rs:103-114
static size_t parse_k(const std::string &s) {
    if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos || s.size() > 19)
        usage_error("invalid value '" + s + "' for '<K>': '" + s + "' is not a valid number");
    const unsigned long long k = strtoull(s.c_str(), nullptr, 10);
    if (k == 0) usage_error("invalid value '" + s + "' for '<K>': k-mer length must be at least 1");
    if (k > 32) usage_error("invalid value '" + s + "' for '<K>': k-mer length must be at most 32");
    return (size_t)k;
}

static uint64_t parse_u64(const std::string &s, const char *what, uint64_t max) {
    if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos || s.size() > 19)
        usage_error("invalid value '" + s + "' for '" + what + "': invalid digit found in string");
    const unsigned long long v = strtoull(s.c_str(), nullptr, 10);
    if (v > max) usage_error("invalid value '" + s + "' for '" + what + "': number too large to fit in target type");
    return v;
}

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define KMERUST_UNDER_ASAN 1
#endif
#endif
// kmerust query <INDEX> --sequences <PATH> [-i FMT] [-Q N] [-f summary|profile] [-q]: per-base abundance (no reference counterpart)
static int run_query_sequences(int argc, char **argv) {
    std::string index, path;
    bool have_index = false, have_path = false, quiet = false;
    SequenceFormat in_fmt = SequenceFormat::Auto;
    ProfileFormat fmt = ProfileFormat::Summary;
    const char *fmt_name = "summary";
    int min_quality = -1;
    size_t batch_bytes = 0;
    auto value_of = [&](int &i, const std::string &arg, const char *name) -> std::string {
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) return arg.substr(eq + 1);
        if (arg.rfind("--", 0) != 0 && arg.size() > 2) return arg.substr(2);  // -fVALUE
        if (i + 1 >= argc) usage_error(std::string("a value is required for '") + name + "' but none was supplied");
        return argv[++i];
    };
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        const std::string key = a.rfind("--", 0) == 0 ? a.substr(0, a.find('=')) : a.substr(0, 2);
        if (a == "-q" || a == "--quiet") {
            quiet = true;
        } else if (key == "--sequences") {
            path = value_of(i, a, "--sequences <PATH>");
            have_path = true;
        } else if (key == "-f" || key == "--format") {
            const std::string v = value_of(i, a, "--format <FORMAT>");
            if (v == "summary") fmt = ProfileFormat::Summary, fmt_name = "summary";
            else if (v == "profile") fmt = ProfileFormat::Profile, fmt_name = "profile";
            else usage_error("invalid value '" + v + "' for '--format <FORMAT>'\n  [possible values: summary, profile]");
        } else if (key == "-i" || key == "--input-format") {
            const std::string v = value_of(i, a, "--input-format <INPUT_FORMAT>");
            if (v == "auto") in_fmt = SequenceFormat::Auto;
            else if (v == "fasta") in_fmt = SequenceFormat::Fasta;
            else if (v == "fastq") in_fmt = SequenceFormat::Fastq;
            else usage_error("invalid value '" + v + "' for '--input-format <INPUT_FORMAT>'\n  [possible values: auto, fasta, fastq]");
        } else if (key == "-Q" || key == "--min-quality") {
            min_quality = (int)parse_u64(value_of(i, a, "--min-quality <MIN_QUALITY>"), "--min-quality <MIN_QUALITY>", 255);
        } else if (key == "--__batch-kb") {  // hidden test hook, as __parse: KiB of flat records per kh_profile call
            batch_bytes = (size_t)parse_u64(value_of(i, a, "--__batch-kb <N>"), "--__batch-kb <N>", 1u << 22) << 10;
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            usage_error("unexpected argument '" + a + "' found");
        } else if (!have_index) {
            index = a;
            have_index = true;
        } else {
            usage_error("unexpected argument '" + a + "' found");
        }
    }
    if (!have_index) usage_error("the following required arguments were not provided:\n  <INDEX>\n\nUsage: kmerust query <INDEX> --sequences <PATH>");
    if (!have_path) usage_error("the following required arguments were not provided:\n  --sequences <PATH>\n\nUsage: kmerust query <INDEX> --sequences <PATH>");
    const bool from_stdin = is_stdin_path(path);
    if (!from_stdin) {
        struct stat st;
        if (stat(path.c_str(), &st) != 0) {
            fprintf(stderr, "Problem with arguments:\n File not found: %s\n", path.c_str());
            return 1;
        }
    }
    const SequenceFormat resolved = resolve_format(in_fmt, from_stdin ? nullptr : &path);
    if (!quiet) {  // (the counting command's banner, with the index where that has k)
        fprintf(stderr, "index: %s\n", index.c_str());
        fprintf(stderr, "data: %s\n", from_stdin ? "<stdin>" : path.c_str());
        if (in_fmt == SequenceFormat::Auto) fprintf(stderr, "input-format: %s (auto-detected)\n", format_name(resolved));
        else fprintf(stderr, "input-format: %s\n", format_name(in_fmt));
        fprintf(stderr, "reader: kmerhip\n");
        fprintf(stderr, "output-format: %s\n", fmt_name);
        if (min_quality >= 0) fprintf(stderr, "min-quality: %d\n", min_quality);
        fprintf(stderr, "\n");
    }
    if (min_quality >= 0 && resolved == SequenceFormat::Fasta) fprintf(stderr, "warning: --min-quality is ignored for FASTA input\n");
    if (min_quality >= 0 && from_stdin) fprintf(stderr, "warning: --min-quality is not yet supported for stdin input\n");
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (as cli_main)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        query_sequences(index, path, in_fmt, min_quality, fmt, stdout, batch_bytes);
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n %s\n", e.what());
        return 1;
    }
    return 0;
}

// kmerust filter <INDEX> <PATH> [-i FMT] [-Q N] [--min-count LO] [--max-count HI] [--min-kmers N] [--min-fraction F] [-v] [-q]:
// reads kept or dropped by the abundance of their k-mers in the index (no reference counterpart)
static int run_filter(int argc, char **argv) {
    std::string index, path;
    bool have_index = false, have_path = false, quiet = false;
    SequenceFormat in_fmt = SequenceFormat::Auto;
    FilterRule rule;
    int min_quality = -1;
    size_t batch_bytes = 0;
    auto value_of = [&](int &i, const std::string &arg, const char *name) -> std::string {
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) return arg.substr(eq + 1);
        if (arg.rfind("--", 0) != 0 && arg.size() > 2) return arg.substr(2);  // -QVALUE
        if (i + 1 >= argc) usage_error(std::string("a value is required for '") + name + "' but none was supplied");
        return argv[++i];
    };
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        const std::string key = a.rfind("--", 0) == 0 ? a.substr(0, a.find('=')) : a.substr(0, 2);
        if (a == "-q" || a == "--quiet") {
            quiet = true;
        } else if (a == "-v" || a == "--invert") {
            rule.invert = true;
        } else if (key == "-i" || key == "--input-format") {
            const std::string v = value_of(i, a, "--input-format <INPUT_FORMAT>");
            if (v == "auto") in_fmt = SequenceFormat::Auto;
            else if (v == "fasta") in_fmt = SequenceFormat::Fasta;
            else if (v == "fastq") in_fmt = SequenceFormat::Fastq;
            else usage_error("invalid value '" + v + "' for '--input-format <INPUT_FORMAT>'\n  [possible values: auto, fasta, fastq]");
        } else if (key == "-Q" || key == "--min-quality") {
            min_quality = (int)parse_u64(value_of(i, a, "--min-quality <MIN_QUALITY>"), "--min-quality <MIN_QUALITY>", 255);
        } else if (key == "--min-count") {
            rule.min_count = (uint32_t)parse_u64(value_of(i, a, "--min-count <LO>"), "--min-count <LO>", 0xFFFFFFFFull);
        } else if (key == "--max-count") {
            rule.max_count = (uint32_t)parse_u64(value_of(i, a, "--max-count <HI>"), "--max-count <HI>", 0xFFFFFFFFull);
        } else if (key == "--min-kmers") {
            rule.min_kmers = parse_u64(value_of(i, a, "--min-kmers <N>"), "--min-kmers <N>", UINT64_MAX);
        } else if (key == "--min-fraction") {
            const std::string v = value_of(i, a, "--min-fraction <F>");
            char *end = nullptr;
            const double f = v.empty() ? -1.0 : strtod(v.c_str(), &end);
            if (v.empty() || *end || v.find_first_not_of("0123456789.eE+-") != std::string::npos)
                usage_error("invalid value '" + v + "' for '--min-fraction <F>': invalid float literal");
            if (!(f >= 0.0 && f <= 1.0)) usage_error("invalid value '" + v + "' for '--min-fraction <F>': must be between 0 and 1");
            rule.min_fraction = f;
        } else if (key == "--__batch-kb") {  // hidden test hook, as for query --sequences
            batch_bytes = (size_t)parse_u64(value_of(i, a, "--__batch-kb <N>"), "--__batch-kb <N>", 1u << 22) << 10;
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            usage_error("unexpected argument '" + a + "' found");
        } else if (!have_index) {
            index = a;
            have_index = true;
        } else if (!have_path) {
            path = a;
            have_path = true;
        } else {
            usage_error("unexpected argument '" + a + "' found");
        }
    }
    if (!have_index) usage_error("the following required arguments were not provided:\n  <INDEX>\n  <PATH>\n\nUsage: kmerust filter <INDEX> <PATH>");
    if (!have_path) usage_error("the following required arguments were not provided:\n  <PATH>\n\nUsage: kmerust filter <INDEX> <PATH>");
    const bool from_stdin = is_stdin_path(path);
    if (!from_stdin) {
        struct stat st;
        if (stat(path.c_str(), &st) != 0) {
            fprintf(stderr, "Problem with arguments:\n File not found: %s\n", path.c_str());
            return 1;
        }
    }
    const SequenceFormat resolved = resolve_format(in_fmt, from_stdin ? nullptr : &path);
    if (!quiet) {  // (the banner of query --sequences, with the rule where that has the output format)
        fprintf(stderr, "index: %s\n", index.c_str());
        fprintf(stderr, "data: %s\n", from_stdin ? "<stdin>" : path.c_str());
        if (in_fmt == SequenceFormat::Auto) fprintf(stderr, "input-format: %s (auto-detected)\n", format_name(resolved));
        else fprintf(stderr, "input-format: %s\n", format_name(in_fmt));
        fprintf(stderr, "reader: kmerhip\n");
        fprintf(stderr, "keep: %s%llu k-mers and %g of the record's with a count in %u..%u\n", rule.invert ? "fewer than " : "at least ",
                (unsigned long long)rule.min_kmers, rule.min_fraction, rule.min_count, rule.max_count);
        if (min_quality >= 0) fprintf(stderr, "min-quality: %d\n", min_quality);
        fprintf(stderr, "\n");
    }
    if (min_quality >= 0 && resolved == SequenceFormat::Fasta) fprintf(stderr, "warning: --min-quality is ignored for FASTA input\n");
    if (min_quality >= 0 && from_stdin) fprintf(stderr, "warning: --min-quality is not yet supported for stdin input\n");
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (as cli_main)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        uint64_t records = 0, kept = 0;
        filter_sequences(index, path, in_fmt, min_quality, rule, stdout, &records, &kept, batch_bytes);
        if (!quiet) fprintf(stderr, "%llu\t%llu\n", (unsigned long long)records, (unsigned long long)kept);
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n %s\n", e.what());
        return 1;
    }
    return 0;
}

// kmerust compare <INDEX_A> <INDEX_B> ... and kmerust combine <OP> <INDEX_A> <INDEX_B> ...: two indexes against each other (no
// reference counterpart)
static int run_two_indexes(int argc, char **argv, bool combine) {
    const char *cmd = combine ? "combine" : "compare";
    const std::string usage = combine ? "Usage: kmerust combine <OP> <INDEX_A> <INDEX_B>" : "Usage: kmerust compare <INDEX_A> <INDEX_B>";
    std::vector<std::string> pos;
    std::string save;
    bool quiet = false, json = false, sorted = false;
    OutputFormat fmt = combine ? OutputFormat::Fasta : OutputFormat::Tsv;
    uint32_t calc = KH_CALC_SUM;
    const char *calc_name = "sum";
    uint64_t min_a = 1, min_b = 1, min_count = 1;
    auto value_of = [&](int &i, const std::string &arg, const char *name) -> std::string {
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) return arg.substr(eq + 1);
        if (arg.rfind("--", 0) != 0 && arg.size() > 2) return arg.substr(2);  // -fVALUE
        if (i + 1 >= argc) usage_error(std::string("a value is required for '") + name + "' but none was supplied");
        return argv[++i];
    };
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        const std::string key = a.rfind("--", 0) == 0 ? a.substr(0, a.find('=')) : a.substr(0, 2);
        if (a == "-q" || a == "--quiet") {
            quiet = true;
        } else if (key == "--min-count-a") {
            min_a = parse_u64(value_of(i, a, "--min-count-a <N>"), "--min-count-a <N>", UINT64_MAX);
        } else if (key == "--min-count-b") {
            min_b = parse_u64(value_of(i, a, "--min-count-b <N>"), "--min-count-b <N>", UINT64_MAX);
        } else if (key == "-f" || key == "--format") {
            const std::string v = value_of(i, a, "--format <FORMAT>");
            if (!combine) {
                if (v == "tsv") json = false;
                else if (v == "json") json = true;
                else usage_error("invalid value '" + v + "' for '--format <FORMAT>'\n  [possible values: tsv, json]");
            } else if (v == "fasta") fmt = OutputFormat::Fasta;
            else if (v == "tsv") fmt = OutputFormat::Tsv;
            else if (v == "json") fmt = OutputFormat::Json;
            else if (v == "histogram") fmt = OutputFormat::Histogram;
            else usage_error("invalid value '" + v + "' for '--format <FORMAT>'\n  [possible values: fasta, tsv, json, histogram]");
        } else if (combine && (key == "-c" || key == "--calc")) {
            const std::string v = value_of(i, a, "--calc <CALC>");
            if (v == "min") calc = KH_CALC_MIN, calc_name = "min";
            else if (v == "max") calc = KH_CALC_MAX, calc_name = "max";
            else if (v == "sum") calc = KH_CALC_SUM, calc_name = "sum";
            else if (v == "left") calc = KH_CALC_LEFT, calc_name = "left";
            else if (v == "right") calc = KH_CALC_RIGHT, calc_name = "right";
            else usage_error("invalid value '" + v + "' for '--calc <CALC>'\n  [possible values: min, max, sum, left, right]");
        } else if (combine && (key == "-m" || key == "--min-count")) {
            min_count = parse_u64(value_of(i, a, "--min-count <MIN_COUNT>"), "--min-count <MIN_COUNT>", UINT64_MAX);
        } else if (combine && key == "--save") {
            save = value_of(i, a, "--save <SAVE>");
        } else if (combine && a == "--sorted") {
            sorted = true;
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            usage_error("unexpected argument '" + a + "' found");
        } else if (pos.size() < (combine ? 3u : 2u)) {
            pos.push_back(a);
        } else {
            usage_error("unexpected argument '" + a + "' found");
        }
    }
    uint32_t op = 0;
    if (combine && !pos.empty()) {
        const std::string &v = pos[0];
        if (v == "intersect") op = KH_SET_INTERSECT;
        else if (v == "union") op = KH_SET_UNION;
        else if (v == "subtract") op = KH_SET_SUBTRACT;
        else if (v == "count-subtract") op = KH_SET_COUNT_SUBTRACT;
        else usage_error("invalid value '" + v + "' for '<OP>'\n  [possible values: intersect, union, subtract, count-subtract]");
    }
    static const char *const names[3] = {"<OP>", "<INDEX_A>", "<INDEX_B>"};
    const size_t need = combine ? 3 : 2;
    if (pos.size() < need) {
        std::string msg = "the following required arguments were not provided:";
        for (size_t j = pos.size(); j < need; ++j) msg += std::string("\n  ") + names[j + (combine ? 0 : 1)];
        usage_error(msg + "\n\n" + usage);
    }
    const std::string &ia = pos[need - 2], &ib = pos[need - 1];
    if (!quiet) {
        if (combine) fprintf(stderr, "operation: %s\n", pos[0].c_str());
        fprintf(stderr, "index-a: %s\nindex-b: %s\n", ia.c_str(), ib.c_str());
        if (combine && (op == KH_SET_INTERSECT || op == KH_SET_UNION)) fprintf(stderr, "calc: %s\n", calc_name);
        if (min_a > 1) fprintf(stderr, "min-count-a: %llu\n", (unsigned long long)min_a);
        if (min_b > 1) fprintf(stderr, "min-count-b: %llu\n", (unsigned long long)min_b);
        if (combine && min_count > 1) fprintf(stderr, "min-count: %llu\n", (unsigned long long)min_count);
        if (!save.empty()) fprintf(stderr, "save-index: %s\n", save.c_str());
        fprintf(stderr, "\n");
    }
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (as cli_main)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        if (combine) {
            uint64_t n = 0;
            combine_indexes(op, calc, ia, ib, min_a, min_b, min_count, fmt, save, stdout, &n, sorted);
            if (!quiet && !save.empty()) fprintf(stderr, "saved: %s (%llu k-mers)\n", save.c_str(), (unsigned long long)n);
        } else {
            compare_indexes(ia, ib, min_a, min_b, json, stdout);
        }
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n %s: %s\n", cmd, e.what());
        return 1;
    }
    return 0;
}

// kmerust graph <INDEX> [-m N] [-f summary|tsv|json] [--sorted]: the de Bruijn graph degrees of an index (no reference counterpart)
static int run_graph(int argc, char **argv) {
    std::string index;
    bool have_index = false, sorted = false;
    GraphFormat fmt = GraphFormat::Summary;
    uint64_t min_count = 1;
    auto value_of = [&](int &i, const std::string &arg, const char *name) -> std::string {
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) return arg.substr(eq + 1);
        if (arg.rfind("--", 0) != 0 && arg.size() > 2) return arg.substr(2);  // -fVALUE
        if (i + 1 >= argc) usage_error(std::string("a value is required for '") + name + "' but none was supplied");
        return argv[++i];
    };
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        const std::string key = a.rfind("--", 0) == 0 ? a.substr(0, a.find('=')) : a.substr(0, 2);
        if (key == "-f" || key == "--format") {
            const std::string v = value_of(i, a, "--format <FORMAT>");
            if (v == "summary") fmt = GraphFormat::Summary;
            else if (v == "tsv") fmt = GraphFormat::Tsv;
            else if (v == "json") fmt = GraphFormat::Json;
            else usage_error("invalid value '" + v + "' for '--format <FORMAT>'\n  [possible values: summary, tsv, json]");
        } else if (key == "-m" || key == "--min-count") {
            min_count = parse_u64(value_of(i, a, "--min-count <MIN_COUNT>"), "--min-count <MIN_COUNT>", UINT64_MAX);
        } else if (a == "--sorted") {
            sorted = true;
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            usage_error("unexpected argument '" + a + "' found");
        } else if (!have_index) {
            index = a;
            have_index = true;
        } else {
            usage_error("unexpected argument '" + a + "' found");
        }
    }
    if (!have_index) usage_error("the following required arguments were not provided:\n  <INDEX>\n\nUsage: kmerust graph <INDEX>");
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (as cli_main)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        graph_index(index, min_count, fmt, sorted, stdout);
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n graph: %s\n", e.what());
        return 1;
    }
    return 0;
}

// kmerust unitigs <INDEX> [-m N] [-f fasta|summary]: the unitigs of an index's de Bruijn graph (no reference counterpart)
static int run_unitigs(int argc, char **argv) {
    std::string index;
    bool have_index = false;
    UnitigFormat fmt = UnitigFormat::Fasta;
    uint64_t min_count = 1;
    auto value_of = [&](int &i, const std::string &arg, const char *name) -> std::string {
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) return arg.substr(eq + 1);
        if (arg.rfind("--", 0) != 0 && arg.size() > 2) return arg.substr(2);  // -fVALUE
        if (i + 1 >= argc) usage_error(std::string("a value is required for '") + name + "' but none was supplied");
        return argv[++i];
    };
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        const std::string key = a.rfind("--", 0) == 0 ? a.substr(0, a.find('=')) : a.substr(0, 2);
        if (key == "-f" || key == "--format") {
            const std::string v = value_of(i, a, "--format <FORMAT>");
            if (v == "fasta") fmt = UnitigFormat::Fasta;
            else if (v == "summary") fmt = UnitigFormat::Summary;
            else usage_error("invalid value '" + v + "' for '--format <FORMAT>'\n  [possible values: fasta, summary]");
        } else if (key == "-m" || key == "--min-count") {
            min_count = parse_u64(value_of(i, a, "--min-count <MIN_COUNT>"), "--min-count <MIN_COUNT>", UINT64_MAX);
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            usage_error("unexpected argument '" + a + "' found");
        } else if (!have_index) {
            index = a;
            have_index = true;
        } else {
            usage_error("unexpected argument '" + a + "' found");
        }
    }
    if (!have_index) usage_error("the following required arguments were not provided:\n  <INDEX>\n\nUsage: kmerust unitigs <INDEX>");
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (as cli_main)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        unitigs_index(index, min_count, fmt, stdout);
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n unitigs: %s\n", e.what());
        return 1;
    }
    return 0;
}

// kmerust gfa <INDEX> [-m N] [-f gfa|summary]: the unitigs of an index and the links between them (no reference counterpart)
static int run_gfa(int argc, char **argv) {
    std::string index;
    bool have_index = false;
    GfaFormat fmt = GfaFormat::Gfa;
    uint64_t min_count = 1;
    auto value_of = [&](int &i, const std::string &arg, const char *name) -> std::string {
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) return arg.substr(eq + 1);
        if (arg.rfind("--", 0) != 0 && arg.size() > 2) return arg.substr(2);  // -fVALUE
        if (i + 1 >= argc) usage_error(std::string("a value is required for '") + name + "' but none was supplied");
        return argv[++i];
    };
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        const std::string key = a.rfind("--", 0) == 0 ? a.substr(0, a.find('=')) : a.substr(0, 2);
        if (key == "-f" || key == "--format") {
            const std::string v = value_of(i, a, "--format <FORMAT>");
            if (v == "gfa") fmt = GfaFormat::Gfa;
            else if (v == "summary") fmt = GfaFormat::Summary;
            else usage_error("invalid value '" + v + "' for '--format <FORMAT>'\n  [possible values: gfa, summary]");
        } else if (key == "-m" || key == "--min-count") {
            min_count = parse_u64(value_of(i, a, "--min-count <MIN_COUNT>"), "--min-count <MIN_COUNT>", UINT64_MAX);
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            usage_error("unexpected argument '" + a + "' found");
        } else if (!have_index) {
            index = a;
            have_index = true;
        } else {
            usage_error("unexpected argument '" + a + "' found");
        }
    }
    if (!have_index) usage_error("the following required arguments were not provided:\n  <INDEX>\n\nUsage: kmerust gfa <INDEX>");
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (as cli_main)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        gfa_index(index, min_count, fmt, stdout);
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n gfa: %s\n", e.what());
        return 1;
    }
    return 0;
}

// kmerust clip <INDEX> [-m N] [--max-kmers L] [--rounds R] [-f FORMAT] [--sorted] [--save OUT] [-q]: tip clipping of an index's unitig
// graph (no reference counterpart)
static int run_clip(int argc, char **argv) {
    const ClipArgs args = parse_clip_args(std::vector<std::string>(argv + 2, argv + argc));
    if (!args.error.empty()) usage_error(args.error);
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (as cli_main)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        uint64_t n = 0;
        clip_index(args, stdout, args.quiet ? nullptr : stderr, args.save.empty() ? nullptr : &n);
        if (!args.quiet && !args.save.empty()) fprintf(stderr, "saved: %s (%llu k-mers)\n", args.save.c_str(), (unsigned long long)n);
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n clip: %s\n", e.what());
        return 1;
    }
    return 0;
}

static int run_query(int argc, char **argv) {
    for (int i = 2; i < argc; ++i)
        if (!strncmp(argv[i], "--sequences", 11) && (argv[i][11] == 0 || argv[i][11] == '=')) return run_query_sequences(argc, argv);
    if (argc != 4) usage_error("the following required arguments were not provided: <INDEX> <KMER>");
    PackedCounts idx;
    try {
        idx = load_index(argv[2]);
    } catch (const Error &e) {
        fprintf(stderr, "Failed to load index:\n %s\n", e.what());
        return 1;
    }
    std::string q = argv[3];
    for (char &c : q) c = (char)toupper((unsigned char)c);
    if (q.size() != idx.k) {
        fprintf(stderr, "Query error:\n k-mer length mismatch: query has %zu bases, index has k=%u\n", q.size(), idx.k);
        return 1;
    }
    uint64_t packed = 0, canon = 0;
    uint32_t pos = 0;
    if (kh_pack(reinterpret_cast<const uint8_t *>(q.data()), idx.k, &packed, &pos) != KH_OK) {
        const unsigned char b = (unsigned char)q[pos];
        if (b >= 0x20 && b < 0x7F) fprintf(stderr, "Invalid k-mer:\n invalid base '%c' (0x%02x) at position %u\n", b, b, pos);
        else fprintf(stderr, "Invalid k-mer:\n invalid base 0x%02x at position %u\n", b, pos);
        return 1;
    }
    kh_canonical(packed, idx.k, &canon, nullptr);
    uint64_t count = 0;
    for (size_t i = 0; i < idx.keys.size(); ++i)
        if (idx.keys[i] == canon) {
            count = idx.counts[i];
            break;
        }
    printf("%llu\n", (unsigned long long)count);
    return 0;
}

// hidden test hook (no device needed): dump the reader's flat batches
static int run_parse_dump(int argc, char **argv) {
    if (argc < 3) return 2;
    SequenceFormat f = SequenceFormat::Auto;
    bool qual = false;
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "fasta")) f = SequenceFormat::Fasta;
        else if (!strcmp(argv[i], "fastq")) f = SequenceFormat::Fastq;
        else if (!strcmp(argv[i], "--qual")) qual = true;
    }
    try {
        const uint64_t n = read_sequences(argv[2], f, qual, 1u << 20, [&](const Batch &b) {
            printf("BATCH records=%llu bytes=%zu\n", (unsigned long long)b.records, b.bases.size());
            fwrite(b.bases.data(), 1, b.bases.size(), stdout);
            if (!b.qual.empty()) {
                printf("QUAL\n");
                fwrite(b.qual.data(), 1, b.qual.size(), stdout);
            }
        });
        printf("RECORDS %llu\n", (unsigned long long)n);
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n %s\n", e.what());
        return 1;
    }
    return 0;
}

int cli_main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "query")) return run_query(argc, argv);  // src/main.rs:39-47
    if (argc > 1 && !strcmp(argv[1], "filter")) return run_filter(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "compare")) return run_two_indexes(argc, argv, false);
    if (argc > 1 && !strcmp(argv[1], "combine")) return run_two_indexes(argc, argv, true);
    if (argc > 1 && !strcmp(argv[1], "graph")) return run_graph(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "unitigs")) return run_unitigs(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "gfa")) return run_gfa(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "clip")) return run_clip(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "__parse")) return run_parse_dump(argc, argv);

    std::string k_arg, path = "-", save;
    bool have_k = false, have_path = false, quiet = false, sorted = false;
    OutputFormat fmt = OutputFormat::Fasta;
    const char *fmt_name = "fasta";
    SequenceFormat in_fmt = SequenceFormat::Auto;
    uint64_t min_count = 1;
    int min_quality = -1;
    std::vector<int> devices;  // extension: several GPUs (no counterpart in src/cli.rs)

    auto value_of = [&](int &i, const std::string &arg, const char *name) -> std::string {
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) return arg.substr(eq + 1);
        if (arg.rfind("--", 0) != 0 && arg.size() > 2) return arg.substr(2);  // -fVALUE
        if (i + 1 >= argc) usage_error(std::string("a value is required for '") + name + "' but none was supplied");
        return argv[++i];
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const std::string key = a.rfind("--", 0) == 0 ? a.substr(0, a.find('=')) : a.substr(0, 2);
        if (a == "-h" || a == "--help") {
            fputs("MI355X-native canonical k-mer counter (krust-compatible command line)\n\n", stdout);
            fputs(USAGE, stdout);
            return 0;
        } else if (a == "-V" || a == "--version") {
            puts("kmerust 0.3.1 (kmerhip, MI355X)");
            return 0;
        } else if (a == "-q" || a == "--quiet") {
            quiet = true;
        } else if (key == "-f" || key == "--format") {
            const std::string v = value_of(i, a, "--format <FORMAT>");
            if (v == "fasta") fmt = OutputFormat::Fasta, fmt_name = "fasta";
            else if (v == "tsv") fmt = OutputFormat::Tsv, fmt_name = "tsv";
            else if (v == "json") fmt = OutputFormat::Json, fmt_name = "json";
            else if (v == "histogram") fmt = OutputFormat::Histogram, fmt_name = "histogram";
            else usage_error("invalid value '" + v + "' for '--format <FORMAT>'\n  [possible values: fasta, tsv, json, histogram]");
        } else if (key == "-i" || key == "--input-format") {
            const std::string v = value_of(i, a, "--input-format <INPUT_FORMAT>");
            if (v == "auto") in_fmt = SequenceFormat::Auto;
            else if (v == "fasta") in_fmt = SequenceFormat::Fasta;
            else if (v == "fastq") in_fmt = SequenceFormat::Fastq;
            else usage_error("invalid value '" + v + "' for '--input-format <INPUT_FORMAT>'\n  [possible values: auto, fasta, fastq]");
        } else if (key == "-m" || key == "--min-count") {
            min_count = parse_u64(value_of(i, a, "--min-count <MIN_COUNT>"), "--min-count <MIN_COUNT>", UINT64_MAX);
        } else if (key == "-Q" || key == "--min-quality") {
            min_quality = (int)parse_u64(value_of(i, a, "--min-quality <MIN_QUALITY>"), "--min-quality <MIN_QUALITY>", 255);
        } else if (key == "--save") {
            save = value_of(i, a, "--save <SAVE>");
        } else if (a == "--sorted") {
            sorted = true;
        } else if (key == "--gpus") {
            const uint64_t n = parse_u64(value_of(i, a, "--gpus <N>"), "--gpus <N>", 64);
            if (n == 0) usage_error("invalid value '0' for '--gpus <N>': at least one GPU is needed");
            devices.clear();
            for (uint64_t d = 0; d < n; ++d) devices.push_back((int)d);
        } else if (key == "--devices") {
            const std::string v = value_of(i, a, "--devices <LIST>");
            devices.clear();
            size_t pos = 0;
            while (pos <= v.size()) {
                const size_t comma = std::min(v.find(',', pos), v.size());
                devices.push_back((int)parse_u64(v.substr(pos, comma - pos), "--devices <LIST>", 1023));
                pos = comma + 1;
            }
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            usage_error("unexpected argument '" + a + "' found");
        } else if (!have_k) {
            k_arg = a;
            have_k = true;
        } else if (!have_path) {
            path = a;
            have_path = true;
        } else {
            usage_error("unexpected argument '" + a + "' found");
        }
    }
    if (!have_k) usage_error("the following required arguments were not provided:\n  <K>\n\nUsage: kmerust <K> [PATH]");
    const size_t k = parse_k(k_arg);

    const bool from_stdin = is_stdin_path(path);
    if (!from_stdin) {  // src/main.rs:58-67
        struct stat st;
        if (stat(path.c_str(), &st) != 0) {
            fprintf(stderr, "Problem with arguments:\n File not found: %s\n", path.c_str());
            return 1;
        }
    }
    const SequenceFormat resolved = resolve_format(in_fmt, from_stdin ? nullptr : &path);
    if (!quiet) {  // src/main.rs:75-134
        fprintf(stderr, "k-length: %zu\n", k);
        fprintf(stderr, "data: %s\n", from_stdin ? "<stdin>" : path.c_str());
        if (in_fmt == SequenceFormat::Auto) fprintf(stderr, "input-format: %s (auto-detected)\n", format_name(resolved));
        else fprintf(stderr, "input-format: %s\n", format_name(in_fmt));
        fprintf(stderr, "reader: kmerhip\n");
        fprintf(stderr, "output-format: %s\n", fmt_name);
        if (min_count > 1) fprintf(stderr, "min-count: %llu\n", (unsigned long long)min_count);
        if (min_quality >= 0) fprintf(stderr, "min-quality: %d\n", min_quality);
        if (!save.empty()) fprintf(stderr, "save-index: %s\n", save.c_str());
        fprintf(stderr, "\n");
    }
    if (min_quality >= 0 && resolved == SequenceFormat::Fasta)  // src/main.rs:137-143
        fprintf(stderr, "warning: --min-quality is ignored for FASTA input\n");
    if (min_quality >= 0 && from_stdin)  // src/main.rs:145-152
        fprintf(stderr, "warning: --min-quality is not yet supported for stdin input\n");

    const auto t_begin = std::chrono::steady_clock::now();
    struct TimingPrinter {  // KMERUST_TIMING=1: one JSON line on stderr when the command is done (bench.py's `cli` leg reads it)
        std::chrono::steady_clock::time_point t0;
        ~TimingPrinter() {
            const char *e = getenv("KMERUST_TIMING");
            if (!e || !e[0] || e[0] == '0') return;
            const Timing &t = timing();
            const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            fprintf(stderr, "{\"kmerust_timing\": {\"total_s\": %.6f, \"create_s\": %.6f, \"read_s\": %.6f, \"push_s\": %.6f, \"finish_s\": %.6f, "
                            "\"result_s\": %.6f, \"write_s\": %.6f, \"buffers_s\": %.6f, \"destroy_s\": %.6f, \"bytes_read\": %llu, \"chunks\": %llu, \"device_record_scan\": %s, \"writer\": \"%s\"}}\n",
                    total, t.create_s, t.read_s, t.push_s, t.finish_s, t.result_s, t.write_s, t.buffers_s, t.destroy_s, (unsigned long long)t.bytes_read,
                    (unsigned long long)t.chunks, t.text_path ? "true" : "false", t.device_writer ? "device" : "host");
        }
    } timing_printer{t_begin};
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define KMERUST_UNDER_ASAN 1
#endif
#endif
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (gcc / clang / make asan)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        KmerCounter kc;
        kc.k(k).min_count(min_count).format(fmt).input_format(in_fmt).min_quality(min_quality).devices(devices).sorted(sorted);
        if (const char *h = getenv("KMERHIP_CAPACITY_HINT")) kc.capacity_hint(strtoull(h, nullptr, 10));
        if (!save.empty()) {  // src/main.rs:155-212: the index holds ALL k-mers, stdout honours --min-count
            bool saved = false;  // (one count: the pairs for the index, then stdout -- device text where the format has it)
            kc.count_keep_and_write(path, stdout, [&](const PackedCounts &all) {
                try {
                    save_index(all, save);
                } catch (const Error &e) {
                    fprintf(stderr, "Failed to save index:\n %s\n", e.what());
                    return false;
                }
                if (!quiet) fprintf(stderr, "saved: %s (%zu k-mers)\n", save.c_str(), all.keys.size());
                return saved = true;
            });
            if (!saved) return 1;
        } else {
            kc.run(path);
        }
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // namespace kmerust

int main(int argc, char **argv) {
    const int rc = kmerust::cli_main(argc, argv);
    if (kmerust::leak_at_exit()) {  // one count per process: leave without the runtime's piecemeal teardown (see kmerust_host.cpp)
        fflush(nullptr);
        _exit(rc);
    }
    return rc;
}
