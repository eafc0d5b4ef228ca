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

using Args = std::vector<std::string>;  // what follows the command's word on the command line

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define KMERUST_UNDER_ASAN 1
#endif
#endif
// The work of a command behind its arguments: fn's status, or 1 and "Application error:\n {prefix}{what}" for an Error it throws.
template <class Fn>
static int run_guarded(const char *prefix, Fn fn) {
#if !defined(__SANITIZE_ADDRESS__) && !defined(KMERUST_UNDER_ASAN) && !defined(KMERUST_ALWAYS_CLEAN_EXIT)  // (gcc / clang / make asan)
    leak_at_exit() = !getenv("KMERUST_CLEAN_EXIT");
#endif
    try {
        return fn();
    } catch (const Error &e) {
        fprintf(stderr, "Application error:\n %s%s\n", prefix, e.what());
        return 1;
    }
}

// The input side of the commands that read sequences (src/main.rs:58-152): false after "File not found" (exit 1); else, unless quiet,
// the banner -- `head`, the data / input-format / reader lines, `more`, the min-quality line, `tail` and a blank line --, and then the
// warnings for a --min-quality that will not be used.
static bool check_input(const std::string &path, SequenceFormat in_fmt, int min_quality, bool quiet, const std::string &head, const std::string &more,
                        const std::string &tail = "") {
    const bool from_stdin = is_stdin_path(path);
    if (!from_stdin) {
        struct stat st;
        if (stat(path.c_str(), &st) != 0) {
            fprintf(stderr, "Problem with arguments:\n File not found: %s\n", path.c_str());
            return false;
        }
    }
    const SequenceFormat resolved = resolve_format(in_fmt, from_stdin ? nullptr : &path);
    if (!quiet) {
        fputs(head.c_str(), stderr);
        fprintf(stderr, "data: %s\n", from_stdin ? "<stdin>" : path.c_str());
        if (in_fmt == SequenceFormat::Auto) fprintf(stderr, "input-format: %s (auto-detected)\n", format_name(resolved));
        else fprintf(stderr, "input-format: %s\n", format_name(in_fmt));
        fprintf(stderr, "reader: kmerhip\n");
        fputs(more.c_str(), stderr);
        if (min_quality >= 0) fprintf(stderr, "min-quality: %d\n", min_quality);
        fputs(tail.c_str(), stderr);
        fprintf(stderr, "\n");
    }
    if (min_quality >= 0 && resolved == SequenceFormat::Fasta) fprintf(stderr, "warning: --min-quality is ignored for FASTA input\n");
    if (min_quality >= 0 && from_stdin) fprintf(stderr, "warning: --min-quality is not yet supported for stdin input\n");
    return true;
}

// kmerust query <INDEX> --sequences <PATH> ...: per-base abundance (no reference counterpart)
static int run_query_sequences(const Args &args) {
    const QuerySequencesArgs a = parse_query_sequences_args(args);
    if (!a.error.empty()) usage_error(a.error);
    if (!check_input(a.path, a.input_format, a.min_quality, a.quiet, "index: " + a.index + "\n",
                     std::string("output-format: ") + PROFILE_FORMATS[(size_t)a.format] + "\n"))
        return 1;
    return run_guarded("", [&] {
        query_sequences(a.index, a.path, a.input_format, a.min_quality, a.format, stdout, a.batch_bytes);
        return 0;
    });
}

// kmerust filter <INDEX> <PATH> ...: reads kept or dropped by the abundance of their k-mers in the index (no reference counterpart)
static int run_filter(const Args &args) {
    const FilterArgs a = parse_filter_args(args);
    if (!a.error.empty()) usage_error(a.error);
    char keep[256];
    snprintf(keep, sizeof keep, "keep: %s%llu k-mers and %g of the record's with a count in %u..%u\n", a.rule.invert ? "fewer than " : "at least ",
             (unsigned long long)a.rule.min_kmers, a.rule.min_fraction, a.rule.min_count, a.rule.max_count);
    if (!check_input(a.path, a.input_format, a.min_quality, a.quiet, "index: " + a.index + "\n", keep)) return 1;
    return run_guarded("", [&] {
        uint64_t records = 0, kept = 0;
        filter_sequences(a.index, a.path, a.input_format, a.min_quality, a.rule, stdout, &records, &kept, a.batch_bytes);
        if (!a.quiet) fprintf(stderr, "%llu\t%llu\n", (unsigned long long)records, (unsigned long long)kept);
        return 0;
    });
}

// kmerust compare <INDEX_A> <INDEX_B> ... and kmerust combine <OP> <INDEX_A> <INDEX_B> ...: two indexes against each other (no
// reference counterpart)
static int run_two_indexes(const Args &args, bool combine) {
    const TwoIndexArgs a = parse_two_index_args(args, combine);
    if (!a.error.empty()) usage_error(a.error);
    if (!a.quiet) {
        if (combine) fprintf(stderr, "operation: %s\n", a.op_name.c_str());
        fprintf(stderr, "index-a: %s\nindex-b: %s\n", a.index_a.c_str(), a.index_b.c_str());
        if (a.op == KH_SET_INTERSECT || a.op == KH_SET_UNION) fprintf(stderr, "calc: %s\n", CALCS[a.calc - 1]);
        if (a.min_a > 1) fprintf(stderr, "min-count-a: %llu\n", (unsigned long long)a.min_a);
        if (a.min_b > 1) fprintf(stderr, "min-count-b: %llu\n", (unsigned long long)a.min_b);
        if (a.min_count > 1) fprintf(stderr, "min-count: %llu\n", (unsigned long long)a.min_count);
        if (!a.save.empty()) fprintf(stderr, "save-index: %s\n", a.save.c_str());
        fprintf(stderr, "\n");
    }
    return run_guarded(combine ? "combine: " : "compare: ", [&] {
        if (combine) {
            uint64_t n = 0;
            combine_indexes(a.op, a.calc, a.index_a, a.index_b, a.min_a, a.min_b, a.min_count, a.format, a.save, stdout, &n, a.sorted);
            if (!a.quiet && !a.save.empty()) fprintf(stderr, "saved: %s (%llu k-mers)\n", a.save.c_str(), (unsigned long long)n);
        } else {
            compare_indexes(a.index_a, a.index_b, a.min_a, a.min_b, a.json, stdout);
        }
        return 0;
    });
}
static int run_compare(const Args &args) { return run_two_indexes(args, false); }
static int run_combine(const Args &args) { return run_two_indexes(args, true); }

// KMERUST_TIMING=1: one JSON line on stderr when the command is done (bench.py's `cli` leg reads the count command's; `unitigs` and
// `gfa` print the same line: result_s = the unitigs' construction and the text's sizing, write_s = the text, writer = who formatted it)
struct TimingPrinter {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
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
};

// kmerust graph / unitigs / gfa <INDEX> ...: the de Bruijn graph of an index, its unitigs, and the links between them (no reference
// counterpart)
static int run_graph(const Args &args) {
    const IndexArgs a = parse_graph_args(args);
    if (!a.error.empty()) usage_error(a.error);
    return run_guarded("graph: ", [&] { return graph_index(a.index, a.min_count, (GraphFormat)a.format, a.sorted, stdout), 0; });
}
static int run_unitigs(const Args &args) {
    const IndexArgs a = parse_unitigs_args(args);
    if (!a.error.empty()) usage_error(a.error);
    TimingPrinter timing_printer;
    return run_guarded("unitigs: ", [&] { return unitigs_index(a.index, a.min_count, (UnitigFormat)a.format, stdout), 0; });
}
static int run_gfa(const Args &args) {
    const IndexArgs a = parse_gfa_args(args);
    if (!a.error.empty()) usage_error(a.error);
    TimingPrinter timing_printer;
    return run_guarded("gfa: ", [&] { return gfa_index(a.index, a.min_count, (GfaFormat)a.format, stdout), 0; });
}

// kmerust clip <INDEX> ...: tip clipping of an index's unitig graph (no reference counterpart)
static int run_clip(const Args &args) {
    const ClipArgs a = parse_clip_args(args);
    if (!a.error.empty()) usage_error(a.error);
    return run_guarded("clip: ", [&] {
        uint64_t n = 0;
        clip_index(a, stdout, a.quiet ? nullptr : stderr, a.save.empty() ? nullptr : &n);
        if (!a.quiet && !a.save.empty()) fprintf(stderr, "saved: %s (%llu k-mers)\n", a.save.c_str(), (unsigned long long)n);
        return 0;
    });
}

static int run_query(const Args &args) {  // src/main.rs:39-47
    for (const std::string &a : args)
        if (a.rfind("--sequences", 0) == 0 && (a.size() == 11 || a[11] == '=')) return run_query_sequences(args);
    if (args.size() != 2) usage_error("the following required arguments were not provided: <INDEX> <KMER>");
    PackedCounts idx;
    try {
        idx = load_index(args[0]);
    } catch (const Error &e) {
        fprintf(stderr, "Failed to load index:\n %s\n", e.what());
        return 1;
    }
    std::string q = args[1];
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
static int run_parse_dump(const Args &args) {
    if (args.empty()) return 2;
    SequenceFormat f = SequenceFormat::Auto;
    bool qual = false;
    for (size_t i = 1; i < args.size(); ++i) {
        if (args[i] == "fasta") f = SequenceFormat::Fasta;
        else if (args[i] == "fastq") f = SequenceFormat::Fastq;
        else if (args[i] == "--qual") qual = true;
    }
    try {
        const uint64_t n = read_sequences(args[0], f, qual, 1u << 20, [&](const Batch &b) {
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

// kmerust [OPTIONS] <K> [PATH]: the counting command
static int run_count(const Args &args) {
    const CountArgs a = parse_count_args(args);
    if (a.help) {
        fputs("MI355X-native canonical k-mer counter (krust-compatible command line)\n\n", stdout);
        fputs(USAGE, stdout);
        return 0;
    }
    if (a.version) {
        puts("kmerust 0.3.1 (kmerhip, MI355X)");
        return 0;
    }
    if (!a.error.empty()) usage_error(a.error);
    if (!check_input(a.path, a.input_format, a.min_quality, a.quiet, "k-length: " + std::to_string(a.k) + "\n",  // src/main.rs:75-134
                     std::string("output-format: ") + OUTPUT_FORMATS[(size_t)a.format] + "\n" +
                         (a.min_count > 1 ? "min-count: " + std::to_string(a.min_count) + "\n" : ""),
                     a.save.empty() ? "" : "save-index: " + a.save + "\n"))
        return 1;

    TimingPrinter timing_printer;
    return run_guarded("", [&] {
        KmerCounter kc;
        kc.k(a.k).min_count(a.min_count).format(a.format).input_format(a.input_format).min_quality(a.min_quality).devices(a.devices).sorted(a.sorted);
        if (const char *h = getenv("KMERHIP_CAPACITY_HINT")) kc.capacity_hint(strtoull(h, nullptr, 10));
        if (a.save.empty()) {
            kc.run(a.path);
            return 0;
        }
        bool saved = false;  // src/main.rs:155-212: the index holds ALL k-mers, stdout honours --min-count
        kc.count_keep_and_write(a.path, stdout, [&](const PackedCounts &all) {  // (one count: the pairs for the index, then stdout)
            try {
                save_index(all, a.save);
            } catch (const Error &e) {
                fprintf(stderr, "Failed to save index:\n %s\n", e.what());
                return false;
            }
            if (!a.quiet) fprintf(stderr, "saved: %s (%zu k-mers)\n", a.save.c_str(), all.keys.size());
            return saved = true;
        });
        return saved ? 0 : 1;
    });
}

int cli_main(int argc, char **argv) {
    static const struct {
        const char *word;
        int (*run)(const Args &);
    } commands[] = {{"query", run_query},     {"filter", run_filter}, {"compare", run_compare}, {"combine", run_combine},     {"graph", run_graph},
                    {"unitigs", run_unitigs}, {"gfa", run_gfa},       {"clip", run_clip},       {"__parse", run_parse_dump}};
    for (const auto &c : commands)
        if (argc > 1 && !strcmp(argv[1], c.word)) return c.run(Args(argv + 2, argv + argc));
    return run_count(Args(argv + (argc > 0 ? 1 : 0), argv + argc));
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
