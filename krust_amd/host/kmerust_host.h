// kmerust_host.h -- C++ host side above the C ABI (include/kmerhip.h).
//
// The reference's toolchain (Rust) is absent from this image, so the host layer that would be the
// `kmerust` crate is written in C++ and mirrors the reference's interface for this path:
//   SequenceFormat / from_extension / resolve      src/format.rs:47-102
//   Input ("-" = stdin)                            src/input.rs:28-70
//   reader::read / read_with_quality               src/reader.rs:58-79,82-144,167-247 (FASTA/FASTQ, gzip)
//   KmerCounter builder                            src/builder.rs:95-526
//   output_counts (fasta / tsv / json / histogram) src/run.rs:441-486
//   KMIX index save / load / query                 src/index.rs:7-23,222-431
//   CLI                                            src/cli.rs:33-144, src/main.rs:34-299
// Counting itself always goes through kh_* (the HIP path); there is no CPU counting here.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <numeric>
#include <queue>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/kmerhip.h"
#include "cli_args.h"

namespace kmerust {

enum class OutputFormat { Fasta, Tsv, Json, Histogram };  // src/cli.rs:90-101
enum class SequenceFormat { Auto, Fasta, Fastq };         // src/format.rs:20-33

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct KmerLengthError : Error {  // src/error.rs:86-95
    explicit KmerLengthError(size_t k)
        : Error("k-mer length " + std::to_string(k) + " is out of range: must be between 1 and 32"), k(k) {}
    size_t k;
};

// ---- format / input -------------------------------------------------------------------------
SequenceFormat format_from_extension(const std::string &path);          // src/format.rs:47-70
SequenceFormat resolve_format(SequenceFormat f, const std::string *path);  // src/format.rs:97-102
const char *format_name(SequenceFormat f);                                 // Display, src/format.rs:117-125
inline bool is_stdin_path(const std::string &p) { return p == "-"; }      // src/input.rs:55-61

// ---- reader ----------------------------------------------------------------------------------
// Streams a FASTA/FASTQ file (plain or gzip; "-" = stdin) into flat batches: records separated by
// '\n' in `bases`, and, when want_qual, a parallel `qual` buffer.  `sink` is called with whole
// records only (k-mers never span records).  Returns the number of records.
// Parsing choices where the reference's parser (rust-bio 3.0.0) is not pinned by its tests are
// listed in DESIGN.md: lines are right-trimmed of CR / blanks, FASTA sequence lines are
// concatenated, FASTQ records may wrap over several lines, a record header must start with '>' /
// '@', and a FASTQ quality string must be as long as its sequence.
// keep_text (for a caller that writes records out again, `kmerust filter`): `headers` holds every record's header line without
// its '>' / '@', and the qualities of a FASTQ file are kept whether want_qual or not.  Off, a Batch is what it always was.
struct Batch {
    std::vector<uint8_t> bases, qual;
    uint64_t records = 0;
    std::vector<std::string> headers;  // filled only with keep_text
};
using BatchSink = std::function<void(const Batch &)>;
uint64_t read_sequences(const std::string &path, SequenceFormat fmt, bool want_qual, size_t batch_bytes,
                        const BatchSink &sink, bool keep_text = false);

// ---- counting --------------------------------------------------------------------------------
struct PackedCounts {
    uint32_t k = 0;
    std::vector<uint64_t> keys, counts;  // packed canonical key, count
};

// The fluent builder of src/builder.rs:95-526 (same option names and defaults).
class KmerCounter {
public:
    KmerCounter &k(size_t k);  // throws KmerLengthError outside 1..=32 (builder.rs:120-128)
    KmerCounter &min_count(uint64_t n) { min_count_ = n; return *this; }
    KmerCounter &format(OutputFormat f) { format_ = f; return *this; }
    KmerCounter &input_format(SequenceFormat f) { input_format_ = f; return *this; }
    KmerCounter &min_quality(int q) { min_quality_ = q; return *this; }  // -1 = None
    KmerCounter &capacity_hint(uint64_t n) { capacity_hint_ = n; return *this; }
    KmerCounter &device(int d) { device_ = d; return *this; }
    // No reference counterpart (the reference is one process on CPU cores): count on several GPUs of the node,
    // one table per device, merged by the library's RCCL exchange (kh_group_*) into a table sharded by hash range.
    KmerCounter &devices(std::vector<int> d) { devices_ = std::move(d); return *this; }
    // No reference counterpart (HashMap order is unspecified there): records and index pairs in ascending key order -- the k-mer
    // strings in lexicographic order --, so that the same input gives the same bytes (`kmerust --sorted`).  Sorted on the device.
    KmerCounter &sorted(bool s) { sorted_ = s; return *this; }

    // count(): HashMap<String,u64> filtered by min_count (builder.rs:242-262)
    std::unordered_map<std::string, uint64_t> count(const std::string &path) const;
    // packed keys, UNfiltered unless apply_min_count (count_kmers_from_sequences shape, streaming.rs:198-204)
    PackedCounts count_packed(const std::string &path, bool apply_min_count = false) const;
    // histogram(): count -> frequency, ascending (builder.rs:289-307, histogram.rs:88-94)
    std::vector<std::pair<uint64_t, uint64_t>> histogram(const std::string &path) const;
    // run(): count and write to stdout in the configured format (builder.rs:366-373)
    void run(const std::string &path) const;
    // count_to_writer() (builder.rs:403-460)
    void count_to_writer(const std::string &path, FILE *out) const;
    // `kmerust --save`: ONE count; all pairs (for the index) go to `keep`, and when it returns true the records with
    // count >= min_count are written to `out` in the configured format (src/main.rs:155-212)
    void count_keep_and_write(const std::string &path, FILE *out, const std::function<bool(const PackedCounts &)> &keep) const;

    size_t get_k() const { return k_; }

private:
    friend struct Session;
    size_t k_ = 0;
    bool k_set_ = false;
    uint64_t min_count_ = 1;
    OutputFormat format_ = OutputFormat::Fasta;
    SequenceFormat input_format_ = SequenceFormat::Auto;
    int min_quality_ = -1;
    uint64_t capacity_hint_ = 0;
    int device_ = -1;
    std::vector<int> devices_;
    bool sorted_ = false;
};

// ---- pairs in ascending key order on the host (`--sorted` where the device cannot give the whole order) ----------------------
// N lists, each ascending by key, with pairwise disjoint key sets (the shards of a multi-GPU merge, each from kh_result_sorted)
// into one ascending list: an N-way merge over a heap of the lists' heads.  Correct, not fast: one heap step per pair.
inline PackedCounts merge_sorted(uint32_t k, const std::vector<PackedCounts> &lists) {
    PackedCounts out;
    out.k = k;
    size_t total = 0;
    for (const PackedCounts &l : lists) total += l.keys.size();
    out.keys.reserve(total);
    out.counts.reserve(total);
    using Head = std::pair<uint64_t, size_t>;  // (key, list)
    std::priority_queue<Head, std::vector<Head>, std::greater<Head>> heap;
    std::vector<size_t> pos(lists.size(), 0);
    for (size_t i = 0; i < lists.size(); ++i)
        if (!lists[i].keys.empty()) heap.push({lists[i].keys[0], i});
    while (!heap.empty()) {
        const size_t i = heap.top().second;
        heap.pop();
        out.keys.push_back(lists[i].keys[pos[i]]);
        out.counts.push_back(lists[i].counts[pos[i]]);
        if (++pos[i] < lists[i].keys.size()) heap.push({lists[i].keys[pos[i]], i});
    }
    return out;
}
// Pairs in any order into ascending key order, each count with its key (a library without kh_result_sorted: kh_result_copy, then this).
inline void sort_pairs(PackedCounts &pc) {
    std::vector<size_t> order(pc.keys.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return pc.keys[a] < pc.keys[b]; });
    std::vector<uint64_t> keys(order.size()), counts(order.size());
    for (size_t i = 0; i < order.size(); ++i) {
        keys[i] = pc.keys[order[i]];
        counts[i] = pc.counts[order[i]];
    }
    pc.keys.swap(keys);
    pc.counts.swap(counts);
}

// ---- phase walls of the last count (KMERUST_TIMING=1 makes the CLI print them as one JSON line on stderr) ---------
// Stands where the reference has its tracing spans "read_sequences" / "process_sequences" / "unpack_kmers"
// (src/run.rs:253-279, feature `tracing`).
struct Timing {
    double create_s = 0;   // device context(s): runtime start-up, table allocation
    double read_s = 0;     // file -> host buffer (pread / gzread / line parser)
    double push_s = 0;     // kh_push_text / kh_push: H2D, record scan, counting of the chunk
    double finish_s = 0;   // kh_finish (+ the multi-GPU merge)
    double result_s = 0;   // kh_histogram / kh_result_copy
    double write_s = 0;    // formatting and writing the output
    double buffers_s = 0;  // pinned chunk buffers (kh_host_alloc)
    double destroy_s = 0;  // releasing the device context(s)
    uint64_t bytes_read = 0, chunks = 0;
    bool text_path = false;  // records were found on the device (kh_push_text)
    bool device_writer = false;  // the output text was formatted on the device (kh_result_text_*), not by write_counts
};
Timing &timing();
bool &leak_at_exit();  // the CLI sets it: device contexts are not torn down before the process ends

// ---- output (src/run.rs:441-486) -------------------------------------------------------------
std::string unpack_to_string(uint64_t bits, uint32_t k);  // src/kmer.rs:451-456
void write_counts(FILE *out, const PackedCounts &pc, OutputFormat fmt, uint64_t min_count);
void write_histogram(FILE *out, const std::vector<std::pair<uint64_t, uint64_t>> &hist);

// ---- per-base abundance against an index (`kmerust query <INDEX> --sequences <PATH>`; no reference counterpart) ----------------
enum class ProfileFormat { Summary, Profile };
// One line per record of a flat batch -- a record is a '\n'-terminated run of `bases`, as read_sequences delivers it -- from the
// batch's profile (kh_profile: profile[i] = count of the window that starts at byte i, KH_PROFILE_NO_WINDOW where there is none):
//   Summary   {ordinal}\t{windows}\t{present}\t{min}\t{max}\t{sum}   windows = entries that are a window, present = those > 0,
//             min / max over the windows (0 when there is none), sum as u64
//   Profile   one token per window start 0 .. len-k, separated by single blanks: the count, or '-' where there is no window
//             (a record shorter than k: an empty line)
// Records are numbered from first_ordinal; returns the number of records written.
uint64_t write_profile_lines(FILE *out, const uint8_t *bases, const uint32_t *profile, size_t n, uint32_t k, ProfileFormat fmt,
                             uint64_t first_ordinal);
// The records of a flat batch as kh_profile_records takes them: the start byte of every '\n'-terminated run, and n behind the last
// (nrec + 1 entries; an unterminated last run is a record, as for write_profile_lines).
std::vector<uint64_t> record_starts(const uint8_t *bases, size_t n);
// The Summary lines from the rows of kh_profile_records (KH_REC_WORDS words per record): the same bytes as write_profile_lines.
void write_summary_rows(FILE *out, const uint32_t *rows, uint64_t nrec, uint64_t first_ordinal);
// load_index, the pairs into a device table (kh_merge_pairs), then per batch of read_sequences: Summary from kh_profile_records (the
// reduction runs on the device; KMERUST_HOST_SUMMARY=1, or a library without that call, keeps kh_profile + write_profile_lines),
// Profile from kh_profile and the lines above.
// min_quality: -1 = none; used for FASTQ files only, as in counting.  batch_bytes: flat record bytes per call (0 = 16 MiB).
// Throws Error.
void query_sequences(const std::string &index_path, const std::string &path, SequenceFormat fmt, int min_quality, ProfileFormat out_fmt,
                     FILE *out, size_t batch_bytes = 0);

// ---- reads kept or dropped by their k-mers' abundance (`kmerust filter <INDEX> <PATH>`; no reference counterpart) ----------------
struct FilterRule {
    uint32_t min_count = 1, max_count = 0xFFFFFFFEu;  // a window is in range when min_count <= count <= max_count
    uint64_t min_kmers = 1;                           // windows in range a record needs ...
    double min_fraction = 0.0;                        // ... and their share of the record's windows
    bool invert = false;                              // write the records the rule drops
};
// row: one row of kh_profile_records.  windows > 0 && in_range >= min_kmers && in_range >= min_fraction * windows (invert is the writer's)
bool filter_keeps(const uint32_t *row, const FilterRule &rule);
// ">{header}\n{sequence}\n", or with qual "@{header}\n{sequence}\n+\n{quality}\n", appended to dst
void append_record(std::string &dst, const std::string &header, const uint8_t *seq, size_t len, const uint8_t *qual);
// load_index into a device table, then per batch of read_sequences one kh_profile_records call and the records the rule keeps, in input
// order, to out.  min_quality masks on the device (FASTQ files only, as in counting).  Throws Error.
void filter_sequences(const std::string &index_path, const std::string &path, SequenceFormat fmt, int min_quality, const FilterRule &rule,
                      FILE *out, uint64_t *records, uint64_t *kept, size_t batch_bytes = 0);

// ---- two indexes against each other (`kmerust compare` / `kmerust combine`; no reference counterpart) -------------------------------
// The measures `kmerust compare` derives from the KH_CMP_WORDS words of kh_compare: jaccard = shared / (distinct_a + distinct_b -
// shared), containment_a = shared / distinct_a, containment_b = shared / distinct_b, bray_curtis = 1 - 2 sum_min / (sum_a + sum_b).
// A division by zero gives NaN.  Pure: no device, no library call.
struct CompareMeasures {
    double jaccard, containment_a, containment_b, bray_curtis;
};
inline CompareMeasures compare_measures(const uint64_t *words) {
    const double nan = std::nan("");
    const double da = (double)words[KH_CMP_DISTINCT_A], db = (double)words[KH_CMP_DISTINCT_B], sh = (double)words[KH_CMP_SHARED];
    const double sums = (double)words[KH_CMP_SUM_A] + (double)words[KH_CMP_SUM_B];
    CompareMeasures m;
    m.jaccard = da + db - sh > 0 ? sh / (da + db - sh) : nan;
    m.containment_a = da > 0 ? sh / da : nan;
    m.containment_b = db > 0 ? sh / db : nan;
    m.bray_curtis = sums > 0 ? 1.0 - 2.0 * (double)words[KH_CMP_SUM_MIN] / sums : nan;
    return m;
}
// "%.6f", or "nan" (never "-nan")
inline std::string format_measure(double v) {
    if (std::isnan(v)) return "nan";
    char buf[64];
    snprintf(buf, sizeof(buf), "%.6f", v);
    return buf;
}
// The eight words by name, then the four measures: tsv = one "{name}\t{value}" line each; json = one object on one line (a
// measure that is NaN is written as NaN).
void write_compare(FILE *out, const uint64_t *words, bool json);
// Both indexes into device tables (as `query --sequences` loads one), kh_compare, write_compare.  Indexes with different k: an Error
// that names both, before any device call.  Throws Error.
void compare_indexes(const std::string &index_a, const std::string &index_b, uint64_t min_a, uint64_t min_b, bool json, FILE *out);
// Both indexes into device tables, a third context of the same k, kh_combine_into(op, calc: KH_SET_* / KH_CALC_*), and that context
// through the writers of the counting command: `save` (unless empty) takes ALL result pairs as an index, `out` the records with
// count >= min_count in format `fmt` (the device text stream where the format has one).  *n_pairs (optional): pairs produced.
void combine_indexes(uint32_t op, uint32_t calc, const std::string &index_a, const std::string &index_b, uint64_t min_a, uint64_t min_b,
                     uint64_t min_count, OutputFormat fmt, const std::string &save, FILE *out, uint64_t *n_pairs = nullptr,
                     bool sorted = false);  // sorted: records and index pairs in ascending key order, as KmerCounter::sorted

// ---- the de Bruijn graph degrees of an index (`kmerust graph`; no reference counterpart) ---------------------------------------------
// What `kmerust graph -f summary` derives from the KH_GRAPH_WORDS words of kh_graph_stats (word m < 256: the nodes whose neighbour
// mask is m -- bits 0..3 the right neighbours by A, C, G, T, bits 4..7 the left ones).  With l / r = the number of left / right bits:
//   deg[l][r]  nodes of left degree l and right degree r      arcs       the sum over the nodes of l + r
//   isolated   mask 0                                         dead_ends  exactly one of l, r is 0
//   branching  l >= 2 or r >= 2                               simple     l == 1 and r == 1
// Sums are modulo 2^64, like the words.  Pure: no device, no library call.
struct GraphSummary {
    uint64_t nodes = 0, kmers = 0, arcs = 0, isolated = 0, dead_ends = 0, branching = 0, simple = 0;
    uint64_t deg[5][5] = {};
};
inline GraphSummary graph_summary(const uint64_t *words) {
    GraphSummary g;
    g.nodes = words[KH_GRAPH_NODES];
    g.kmers = words[KH_GRAPH_KMERS];
    for (unsigned m = 0; m < 256; ++m) {
        const unsigned l = (unsigned)__builtin_popcount(m >> 4), r = (unsigned)__builtin_popcount(m & 15u);
        const uint64_t n = words[m];
        g.deg[l][r] += n;
        g.arcs += n * (uint64_t)(l + r);
        if (m == 0) g.isolated += n;
        if ((l == 0) != (r == 0)) g.dead_ends += n;
        if (l >= 2 || r >= 2) g.branching += n;
        if (l == 1 && r == 1) g.simple += n;
    }
    return g;
}
// One line of `kmerust graph -f tsv`, appended to dst: "{kmer}\t{count}\t{left}\t{right}\n" -- left / right: the letters of the
// mask's set bits in ACGT order, "." when none is set.  Correct, not fast: the device has no formatter for this layout.
inline void format_graph_line(std::string &dst, uint64_t key, uint32_t k, uint64_t count, uint8_t mask) {
    static const char letters[5] = "ACGT";
    for (uint32_t i = 0; i < k; ++i) dst.push_back(letters[(key >> (2 * (k - 1 - i))) & 3u]);
    dst.push_back('\t');
    dst += std::to_string(count);
    for (unsigned side = 0; side < 2; ++side) {  // left (bits 4..7), then right (bits 0..3)
        const unsigned bits = side == 0 ? (unsigned)(mask >> 4) : (unsigned)(mask & 15u);
        dst.push_back('\t');
        if (!bits) dst.push_back('.');
        for (unsigned c = 0; c < 4; ++c)
            if (bits & (1u << c)) dst.push_back(letters[c]);
    }
    dst.push_back('\n');
}
enum class GraphFormat { Summary, Tsv, Json };
// The summary by name: nodes, kmers, arcs, isolated, dead_ends, branching, simple, then the 25 deg_{l}_{r}; tsv = one
// "{name}\t{value}" line each, json = one object on one line.
void write_graph_summary(FILE *out, const uint64_t *words, bool json);
// The index into a device table (as `compare` loads one); Summary / Json: kh_graph_stats and write_graph_summary; Tsv: the pairs with
// count >= min_count (kh_result_copy, or kh_result_sorted with `sorted`), kh_graph_masks over their keys, format_graph_line.
// Throws Error -- also against a library without the three kh_graph_* entry points.
void graph_index(const std::string &index, uint64_t min_count, GraphFormat fmt, bool sorted, FILE *out);

// ---- the unitigs of an index (`kmerust unitigs`; no reference counterpart) ---------------------------------------------------------------
// The header line of unitig i, WITHOUT the newline, from its KH_UNI_WORDS row:
//   ">{i} LN:i:{bases} KC:i:{count_sum} km:f:{count_sum / L, %.1f}" and " CR:i:1" behind it for a circular one
// (the tags BCALM writes; bases = L + k - 1).  Pure: no device, no library call.
inline std::string unitig_header(uint64_t i, const uint64_t *row, uint32_t k) {
    const uint64_t L = row[KH_UNI_KMERS], cs = row[KH_UNI_COUNT_SUM];
    char km[64];
    snprintf(km, sizeof km, "%.1f", L ? (double)cs / (double)L : 0.0);
    std::string h = ">" + std::to_string(i) + " LN:i:" + std::to_string(L + k - 1) + " KC:i:" + std::to_string(cs) + " km:f:" + km;
    if (row[KH_UNI_FLAGS] & KH_UNI_CIRCULAR) h += " CR:i:1";
    return h;
}
// What `kmerust unitigs -f summary` derives from the n rows: unitigs = n, kmers = the sum of L, bases = the sum of L + k - 1 (both
// modulo 2^64), circular, longest (bases), and n50 (bases): the largest length X such that the unitigs of at least X bases hold at
// least half of all bases -- 0 for no unitig.  Pure.
struct UnitigSummary {
    uint64_t unitigs = 0, kmers = 0, bases = 0, circular = 0, longest = 0, n50 = 0;
};
inline UnitigSummary unitig_summary(const uint64_t *rows, uint64_t n, uint32_t k) {
    UnitigSummary u;
    u.unitigs = n;
    std::vector<uint64_t> len(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t *r = rows + KH_UNI_WORDS * i;
        len[i] = r[KH_UNI_KMERS] + k - 1;
        u.kmers += r[KH_UNI_KMERS];
        u.bases += len[i];
        if (r[KH_UNI_FLAGS] & KH_UNI_CIRCULAR) ++u.circular;
        if (len[i] > u.longest) u.longest = len[i];
    }
    std::sort(len.begin(), len.end(), [](uint64_t a, uint64_t b) { return a > b; });
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; ++i) {
        run += len[i];
        if (run >= u.bases - run) {  // (run >= half of the bases, without doubling)
            u.n50 = len[i];
            break;
        }
    }
    return u;
}
enum class UnitigFormat { Fasta, Summary };
// "{name}\t{value}" lines: unitigs, kmers, bases, circular, longest, n50.
void write_unitig_summary(FILE *out, const UnitigSummary &u);
// The index into a device table (as `graph` loads one), kh_unitigs_begin / kh_unitigs_copy / kh_unitigs_end; Fasta: unitig_header and
// the unitig's bases, one record each -- the same bytes formatted on the device and streamed out (kh_unitigs_text_*) where the library
// has those calls and KMERUST_HOST_FORMAT=1 is not set; Summary: unitig_summary of the rows.  Throws Error -- also against a library
// without the four kh_unitigs_* entry points.
void unitigs_index(const std::string &index, uint64_t min_count, UnitigFormat fmt, FILE *out);

// ---- the unitig graph of an index as GFA (`kmerust gfa`; no reference counterpart) ------------------------------------------------------
// The tags of unitig_header() as GFA fields: "LN:i:{bases}\tKC:i:{count_sum}\tkm:f:{%.1f}" and "\tCR:i:1" behind them for a circular one.
inline std::string gfa_segment_tags(const uint64_t *row, uint32_t k) {
    const uint64_t L = row[KH_UNI_KMERS], cs = row[KH_UNI_COUNT_SUM];
    char km[64];
    snprintf(km, sizeof km, "%.1f", L ? (double)cs / (double)L : 0.0);
    std::string t = "LN:i:" + std::to_string(L + k - 1) + "\tKC:i:" + std::to_string(cs) + "\tkm:f:" + km;
    if (row[KH_UNI_FLAGS] & KH_UNI_CIRCULAR) t += "\tCR:i:1";
    return t;
}
// The S line of unitig i, WITHOUT the newline: "S\t{i}\t{sequence}\t{tags}".  Pure.
inline std::string gfa_segment_line(uint64_t i, const uint64_t *row, uint32_t k, const char *seq, size_t len) {
    std::string s = "S\t" + std::to_string(i) + "\t";
    s.append(seq, len);
    s.push_back('\t');
    s += gfa_segment_tags(row, k);
    return s;
}
// The L line of a link word (include/kmerhip.h), WITHOUT the newline: "L\t{from}\t{+|-}\t{to}\t{+|-}\t{k-1}M".  Pure.
inline std::string gfa_link_line(uint64_t w, uint32_t k) {
    return "L\t" + std::to_string(KH_UNI_LINK_FROM(w)) + (KH_UNI_LINK_FROM_SIGN(w) ? "\t-\t" : "\t+\t") + std::to_string(KH_UNI_LINK_TO(w)) +
           (KH_UNI_LINK_TO_SIGN(w) ? "\t-\t" : "\t+\t") + std::to_string(k - 1) + "M";
}
// What `kmerust gfa -f summary` derives from the n rows and the m link words: unitigs = n, links = m, self_links (from-unitig =
// to-unitig), dead_ends (end states with no link out), isolated (unitigs with both ends dead) and tips (non-circular unitigs with
// exactly one dead end and KMERS <= k).  A link whose from-unitig is not below n is not counted for any end.  Pure.
struct LinkSummary {
    uint64_t unitigs = 0, links = 0, self_links = 0, dead_ends = 0, isolated = 0, tips = 0;
};
inline LinkSummary link_summary(const uint64_t *rows, uint64_t n, const uint64_t *links, uint64_t m, uint32_t k) {
    LinkSummary s;
    s.unitigs = n;
    s.links = m;
    std::vector<uint8_t> out(n, 0);  // bit e: end e has a link out
    for (uint64_t j = 0; j < m; ++j) {
        const uint64_t from = KH_UNI_LINK_FROM(links[j]);
        if (from == KH_UNI_LINK_TO(links[j])) ++s.self_links;
        if (from < n) out[from] |= (uint8_t)(1u << KH_UNI_LINK_FROM_SIGN(links[j]));
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t *r = rows + KH_UNI_WORDS * i;
        const unsigned dead = 2u - (out[i] & 1u) - ((out[i] >> 1) & 1u);
        s.dead_ends += dead;
        if (dead == 2) ++s.isolated;
        if (dead == 1 && !(r[KH_UNI_FLAGS] & KH_UNI_CIRCULAR) && r[KH_UNI_KMERS] <= k) ++s.tips;
    }
    return s;
}
enum class GfaFormat { Gfa, Summary };
// "{name}\t{value}" lines: unitigs, links, self_links, dead_ends, isolated, tips.
void write_link_summary(FILE *out, const LinkSummary &s);
// The index into a device table (as `unitigs` loads one), kh_unitigs_begin_linked / kh_unitigs_copy / kh_unitigs_links_copy /
// kh_unitigs_end; Gfa: the header line, one S line per unitig, one L line per link in link order (from the device's kh_unitigs_text_*
// stream, or by the writers above under KMERUST_HOST_FORMAT=1 / against a library without it); Summary: link_summary.  Throws
// Error -- also against a library without the kh_unitigs_begin_linked / kh_unitigs_links_copy entry points.
void gfa_index(const std::string &index, uint64_t min_count, GfaFormat fmt, FILE *out);

// ---- tip clipping of an index's unitig graph (`kmerust clip`; no reference counterpart) -------------------------------------------------
// kmerust clip <INDEX> [-m N] [--max-kmers L] [--rounds R] [-f fasta|tsv|json|histogram] [--sorted] [--save OUT] [-q]
// What the arguments behind "clip" say.  `error` is empty, or the text of a usage error (what follows "error: ").  Pure.
struct ClipArgs {
    std::string index, save, error;
    bool have_index = false, have_max_kmers = false, sorted = false, quiet = false;
    uint64_t min_count = 1, max_kmers = 0, rounds = 1;  // max_kmers without --max-kmers: k, which the index says; rounds 0: until nothing is clipped
    OutputFormat format = OutputFormat::Fasta;
};
// args: what follows "kmerust clip" on the command line (with the other commands' parsers, below)
inline ClipArgs parse_clip_args(const std::vector<std::string> &args);
// Whether the loop ends behind a round: it clipped nothing, or `limit` rounds have run (limit 0: no limit).  Pure.
inline bool clip_stops(uint64_t rounds_done, uint64_t limit, uint64_t clipped) { return clipped == 0 || (limit != 0 && rounds_done >= limit); }
// The stderr line of round `round` (from 1), WITH the newline, from the KH_CLIP_WORDS words of kh_clip_tips_into:
// "{round}\t{unitigs}\t{candidates}\t{clipped}\t{clipped_kmers}\t{kept_kmers}\n".  Pure.
inline std::string clip_round_line(uint64_t round, const uint64_t *words) {
    return std::to_string(round) + "\t" + std::to_string(words[KH_CLIP_UNITIGS]) + "\t" + std::to_string(words[KH_CLIP_CANDIDATES]) + "\t" +
           std::to_string(words[KH_CLIP_CLIPPED]) + "\t" + std::to_string(words[KH_CLIP_CLIPPED_KMERS]) + "\t" + std::to_string(words[KH_CLIP_KEPT_KMERS]) +
           "\n";
}
// The index into a device table (as `unitigs` loads one), then rounds between two further contexts: kh_clip_tips_into, kh_reset of the
// table just read, swap -- until clip_stops().  The last table through the writers of `combine` (format, min_count, sorted, save).
// log (unless NULL): the header line "round\tunitigs\tcandidates\tclipped\tclipped_kmers\tkept_kmers" and one clip_round_line per round.
// *n_pairs (optional): the pairs of the last table.  Throws Error -- also against a library without kh_clip_tips_into.
void clip_index(const ClipArgs &args, FILE *out, FILE *log, uint64_t *n_pairs = nullptr);

// ---- KMIX index (src/index.rs) -----------------------------------------------------------------
uint32_t crc32_ieee(const uint8_t *data, size_t n, uint32_t crc = 0);  // src/index.rs:404-431
void save_index(const PackedCounts &pc, const std::string &path);      // gzip if path ends in .gz
PackedCounts load_index(const std::string &path);                      // validates magic/version/k/size/CRC

// ---- CLI ---------------------------------------------------------------------------------------
int cli_main(int argc, char **argv);

// What the arguments of each command say (src/cli.rs:33-144 for the counting command; the sub-commands have no reference
// counterpart).  Every parse_*_args takes what follows the command's word on the command line and is pure (cli_args.h): `error` is
// empty, or the text of the usage error.  A list of spellings is in the order of the enum or the KH_* constants it stands for.
inline const Choices OUTPUT_FORMATS = {"fasta", "tsv", "json", "histogram"};
inline const Choices INPUT_FORMATS = {"auto", "fasta", "fastq"};
inline const Choices PROFILE_FORMATS = {"summary", "profile"};
inline const Choices COMPARE_FORMATS = {"tsv", "json"};
inline const Choices GRAPH_FORMATS = {"summary", "tsv", "json"};
inline const Choices UNITIG_FORMATS = {"fasta", "summary"};
inline const Choices GFA_FORMATS = {"gfa", "summary"};
inline const Choices CALCS = {"min", "max", "sum", "left", "right"};                  // KH_CALC_*: position + 1
inline const Choices SET_OPS = {"intersect", "union", "subtract", "count-subtract"};  // KH_SET_*: position + 1
static_assert(KH_CALC_MIN == 1 && KH_CALC_SUM == 3 && KH_CALC_RIGHT == 5 && KH_SET_INTERSECT == 1 && KH_SET_COUNT_SUBTRACT == 4,
              "CALCS and SET_OPS are in the order of the constants");

// parse_k, src/cli.rs:103-114 (to: size_t)
inline std::string check_k(const std::string &s, const std::string &what, void *to) {
    uint64_t k = 0;
    if (s.size() > 19 || !parse_u64(s, what, UINT64_MAX, &k).empty()) return invalid_value(s, what, ": '" + s + "' is not a valid number");
    if (k == 0) return invalid_value(s, what, ": k-mer length must be at least 1");
    if (k > 32) return invalid_value(s, what, ": k-mer length must be at most 32");
    *static_cast<size_t *>(to) = (size_t)k;
    return "";
}
// --min-fraction (to: double)
inline std::string check_fraction(const std::string &v, const std::string &what, void *to) {
    char *end = nullptr;
    const double f = v.empty() ? -1.0 : strtod(v.c_str(), &end);
    if (v.empty() || *end || v.find_first_not_of("0123456789.eE+-") != std::string::npos) return invalid_value(v, what, ": invalid float literal");
    if (!(f >= 0.0 && f <= 1.0)) return invalid_value(v, what, ": must be between 0 and 1");
    *static_cast<double *>(to) = f;
    return "";
}
// --gpus N: the ordinals 0 .. N-1; --devices a,b,c: those (to: std::vector<int>; the later of the two options wins)
inline std::string check_gpus(const std::string &v, const std::string &what, void *to) {
    uint64_t n = 0;
    const std::string err = parse_u64(v, what, 64, &n);
    if (!err.empty()) return err;
    if (n == 0) return invalid_value("0", what, ": at least one GPU is needed");
    std::vector<int> &devices = *static_cast<std::vector<int> *>(to);
    devices.clear();
    for (uint64_t d = 0; d < n; ++d) devices.push_back((int)d);
    return "";
}
inline std::string check_devices(const std::string &v, const std::string &what, void *to) {
    std::vector<int> devices;
    for (size_t pos = 0; pos <= v.size();) {
        const size_t comma = std::min(v.find(',', pos), v.size());
        uint64_t d = 0;
        const std::string err = parse_u64(v.substr(pos, comma - pos), what, 1023, &d);
        if (!err.empty()) return err;
        devices.push_back((int)d);
        pos = comma + 1;
    }
    *static_cast<std::vector<int> *>(to) = devices;
    return "";
}

// kmerust [OPTIONS] <K> [PATH]
struct CountArgs {
    std::string error, path = "-", save;
    bool help = false, version = false;  // -h / -V: the walk ended there, and nothing behind it was looked at
    bool quiet = false, sorted = false;
    size_t k = 0;
    OutputFormat format = OutputFormat::Fasta;
    SequenceFormat input_format = SequenceFormat::Auto;
    uint64_t min_count = 1;
    int min_quality = -1;      // -1: none
    std::vector<int> devices;  // extension: several GPUs (no counterpart in src/cli.rs)
};
inline CountArgs parse_count_args(const std::vector<std::string> &args) {
    CountArgs c;
    size_t fmt = 0, in_fmt = 0;
    uint64_t quality = 0;
    bool have_quality = false;
    std::vector<std::string> pos;
    const Command cmd = {{flag("-h", "--help", &c.help, true), flag("-V", "--version", &c.version, true), flag("-q", "--quiet", &c.quiet),
                          choice("-f", "--format", "<FORMAT>", OUTPUT_FORMATS, &fmt), choice("-i", "--input-format", "<INPUT_FORMAT>", INPUT_FORMATS, &in_fmt),
                          number("-m", "--min-count", "<MIN_COUNT>", &c.min_count), number("-Q", "--min-quality", "<MIN_QUALITY>", &quality, 255, &have_quality),
                          text(nullptr, "--save", "<SAVE>", &c.save), flag(nullptr, "--sorted", &c.sorted),
                          custom(nullptr, "--gpus", "<N>", check_gpus, &c.devices), custom(nullptr, "--devices", "<LIST>", check_devices, &c.devices)},
                         {"<K>", "[PATH]"}, 1, "Usage: kmerust <K> [PATH]"};
    c.error = parse_args(cmd, args, &pos);
    if (c.help || c.version) return c;
    if (c.error.empty()) c.error = missing_args(cmd, pos);
    if (c.error.empty()) c.error = check_k(pos[0], "<K>", &c.k);
    if (pos.size() > 1) c.path = pos[1];
    c.format = (OutputFormat)fmt;
    c.input_format = (SequenceFormat)in_fmt;
    if (have_quality) c.min_quality = (int)quality;
    return c;
}

// kmerust query <INDEX> --sequences <PATH> [-i FMT] [-Q N] [-f summary|profile] [-q]
struct QuerySequencesArgs {
    std::string error, index, path;
    bool quiet = false;
    SequenceFormat input_format = SequenceFormat::Auto;
    ProfileFormat format = ProfileFormat::Summary;
    int min_quality = -1;
    size_t batch_bytes = 0;  // --__batch-kb, a hidden test hook as __parse: KiB of flat records per kh_profile call
};
inline QuerySequencesArgs parse_query_sequences_args(const std::vector<std::string> &args) {
    QuerySequencesArgs c;
    size_t fmt = 0, in_fmt = 0;
    uint64_t quality = 0, batch_kb = 0;
    bool have_quality = false, have_path = false;
    std::vector<std::string> pos;
    const Command cmd = {{flag("-q", "--quiet", &c.quiet), text(nullptr, "--sequences", "<PATH>", &c.path, &have_path),
                          choice("-f", "--format", "<FORMAT>", PROFILE_FORMATS, &fmt), choice("-i", "--input-format", "<INPUT_FORMAT>", INPUT_FORMATS, &in_fmt),
                          number("-Q", "--min-quality", "<MIN_QUALITY>", &quality, 255, &have_quality), number(nullptr, "--__batch-kb", "<N>", &batch_kb, 1u << 22)},
                         {"<INDEX>"}, 1, "Usage: kmerust query <INDEX> --sequences <PATH>"};
    c.error = parse_args(cmd, args, &pos);
    if (c.error.empty()) c.error = missing_args(cmd, pos);
    if (c.error.empty() && !have_path) c.error = std::string("the following required arguments were not provided:\n  --sequences <PATH>\n\n") + cmd.usage;
    if (!pos.empty()) c.index = pos[0];
    c.format = (ProfileFormat)fmt;
    c.input_format = (SequenceFormat)in_fmt;
    if (have_quality) c.min_quality = (int)quality;
    c.batch_bytes = (size_t)batch_kb << 10;
    return c;
}

// kmerust filter <INDEX> <PATH> [-i FMT] [-Q N] [--min-count LO] [--max-count HI] [--min-kmers N] [--min-fraction F] [-v] [-q]
struct FilterArgs {
    std::string error, index, path;
    bool quiet = false;
    SequenceFormat input_format = SequenceFormat::Auto;
    FilterRule rule;
    int min_quality = -1;
    size_t batch_bytes = 0;  // --__batch-kb, as for query --sequences
};
inline FilterArgs parse_filter_args(const std::vector<std::string> &args) {
    FilterArgs c;
    size_t in_fmt = 0;
    uint64_t quality = 0, batch_kb = 0, lo = c.rule.min_count, hi = c.rule.max_count;
    bool have_quality = false;
    std::vector<std::string> pos;
    const Command cmd = {{flag("-q", "--quiet", &c.quiet), flag("-v", "--invert", &c.rule.invert),
                          choice("-i", "--input-format", "<INPUT_FORMAT>", INPUT_FORMATS, &in_fmt),
                          number("-Q", "--min-quality", "<MIN_QUALITY>", &quality, 255, &have_quality),
                          number(nullptr, "--min-count", "<LO>", &lo, 0xFFFFFFFFull), number(nullptr, "--max-count", "<HI>", &hi, 0xFFFFFFFFull),
                          number(nullptr, "--min-kmers", "<N>", &c.rule.min_kmers), custom(nullptr, "--min-fraction", "<F>", check_fraction, &c.rule.min_fraction),
                          number(nullptr, "--__batch-kb", "<N>", &batch_kb, 1u << 22)},
                         {"<INDEX>", "<PATH>"}, 2, "Usage: kmerust filter <INDEX> <PATH>"};
    c.error = parse_args(cmd, args, &pos);
    if (c.error.empty()) c.error = missing_args(cmd, pos);
    if (pos.size() > 0) c.index = pos[0];
    if (pos.size() > 1) c.path = pos[1];
    c.input_format = (SequenceFormat)in_fmt;
    c.rule.min_count = (uint32_t)lo;
    c.rule.max_count = (uint32_t)hi;
    if (have_quality) c.min_quality = (int)quality;
    c.batch_bytes = (size_t)batch_kb << 10;
    return c;
}

// kmerust compare <INDEX_A> <INDEX_B> [--min-count-a N] [--min-count-b N] [-f tsv|json] [-q]
// kmerust combine <OP> <INDEX_A> <INDEX_B> [-c CALC] [--min-count-a N] [--min-count-b N] [-m N] [-f FORMAT] [--save OUT] [--sorted] [-q]
struct TwoIndexArgs {
    std::string error, op_name, index_a, index_b, save;  // op_name ... sorted: combine only
    bool quiet = false, json = false, sorted = false;
    OutputFormat format = OutputFormat::Fasta;
    uint32_t op = 0, calc = KH_CALC_SUM;  // KH_SET_*, KH_CALC_*
    uint64_t min_a = 1, min_b = 1, min_count = 1;
};
inline TwoIndexArgs parse_two_index_args(const std::vector<std::string> &args, bool combine) {
    TwoIndexArgs c;
    size_t fmt = 0, calc = KH_CALC_SUM - 1, op = 0;
    std::vector<std::string> pos;
    Command cmd = {{flag("-q", "--quiet", &c.quiet), number(nullptr, "--min-count-a", "<N>", &c.min_a), number(nullptr, "--min-count-b", "<N>", &c.min_b),
                    choice("-f", "--format", "<FORMAT>", combine ? OUTPUT_FORMATS : COMPARE_FORMATS, &fmt)},
                   {"<INDEX_A>", "<INDEX_B>"}, 2, "Usage: kmerust compare <INDEX_A> <INDEX_B>"};
    if (combine) {
        cmd.opts.insert(cmd.opts.end(), {choice("-c", "--calc", "<CALC>", CALCS, &calc), number("-m", "--min-count", "<MIN_COUNT>", &c.min_count),
                                         text(nullptr, "--save", "<SAVE>", &c.save), flag(nullptr, "--sorted", &c.sorted)});
        cmd.positionals.insert(cmd.positionals.begin(), "<OP>");
        cmd.required = 3;
        cmd.usage = "Usage: kmerust combine <OP> <INDEX_A> <INDEX_B>";
    }
    c.error = parse_args(cmd, args, &pos);
    if (c.error.empty() && combine && !pos.empty()) c.error = parse_choice(pos[0], "<OP>", SET_OPS, &op);  // (before a missing index is)
    if (c.error.empty()) c.error = missing_args(cmd, pos);
    if (!c.error.empty()) return c;
    if (combine) c.op_name = pos[0], c.op = (uint32_t)op + 1, c.calc = (uint32_t)calc + 1, c.format = (OutputFormat)fmt;
    else c.json = fmt == 1;
    c.index_a = pos[cmd.required - 2];
    c.index_b = pos[cmd.required - 1];
    return c;
}
inline TwoIndexArgs parse_compare_args(const std::vector<std::string> &args) { return parse_two_index_args(args, false); }
inline TwoIndexArgs parse_combine_args(const std::vector<std::string> &args) { return parse_two_index_args(args, true); }

// kmerust graph <INDEX> [-m N] [-f summary|tsv|json] [--sorted], kmerust unitigs <INDEX> [-m N] [-f fasta|summary] and
// kmerust gfa <INDEX> [-m N] [-f gfa|summary].  format: the position in the command's list = the value of its GraphFormat / UnitigFormat /
// GfaFormat.
struct IndexArgs {
    std::string error, index;
    uint64_t min_count = 1;
    size_t format = 0;
    bool sorted = false;  // graph only
};
inline IndexArgs parse_index_args(const std::vector<std::string> &args, const Choices &formats, bool with_sorted, const char *usage) {
    IndexArgs c;
    std::vector<std::string> pos;
    Command cmd = {{choice("-f", "--format", "<FORMAT>", formats, &c.format), number("-m", "--min-count", "<MIN_COUNT>", &c.min_count)}, {"<INDEX>"}, 1, usage};
    if (with_sorted) cmd.opts.push_back(flag(nullptr, "--sorted", &c.sorted));
    c.error = parse_args(cmd, args, &pos);
    if (c.error.empty()) c.error = missing_args(cmd, pos);
    if (!pos.empty()) c.index = pos[0];
    return c;
}
inline IndexArgs parse_graph_args(const std::vector<std::string> &args) { return parse_index_args(args, GRAPH_FORMATS, true, "Usage: kmerust graph <INDEX>"); }
inline IndexArgs parse_unitigs_args(const std::vector<std::string> &args) { return parse_index_args(args, UNITIG_FORMATS, false, "Usage: kmerust unitigs <INDEX>"); }
inline IndexArgs parse_gfa_args(const std::vector<std::string> &args) { return parse_index_args(args, GFA_FORMATS, false, "Usage: kmerust gfa <INDEX>"); }

inline ClipArgs parse_clip_args(const std::vector<std::string> &args) {
    ClipArgs c;
    size_t fmt = 0;
    std::vector<std::string> pos;
    const Command cmd = {{flag("-q", "--quiet", &c.quiet), flag(nullptr, "--sorted", &c.sorted), choice("-f", "--format", "<FORMAT>", OUTPUT_FORMATS, &fmt),
                          number("-m", "--min-count", "<MIN_COUNT>", &c.min_count), number(nullptr, "--max-kmers", "<L>", &c.max_kmers, UINT64_MAX, &c.have_max_kmers),
                          number(nullptr, "--rounds", "<R>", &c.rounds), text(nullptr, "--save", "<SAVE>", &c.save)},
                         {"<INDEX>"}, 1, "Usage: kmerust clip <INDEX>"};
    c.error = parse_args(cmd, args, &pos);
    if (c.error.empty()) c.error = missing_args(cmd, pos);
    c.have_index = !pos.empty();
    if (c.have_index) c.index = pos[0];
    c.format = (OutputFormat)fmt;
    return c;
}

}  // namespace kmerust
