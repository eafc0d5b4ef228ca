// filter_check.cpp -- drives the host side of `kmerust filter` and of the device summary (krust_amd/host/kmerust_host.cpp) without a
// device: tests/test_filter_host.py compiles this file with the host library's source and the recording kh_* stub
// (tests/host_asan/stub_kmerhip.cpp) with a plain g++.  One case per input line, one output line per case:
//   keep <min_count> <max_count> <min_kmers> <min_fraction> <8 row words, comma separated>   ->  0 | 1         (filter_keeps)
//   record <hex header or -> <hex sequence or -> <hex quality or ->                            ->  hex           (append_record)
//   starts <hex bases or ->                                                                    ->  offsets, comma separated
//   summary <first ordinal> <row words, comma separated, or ->                                 ->  hex           (write_summary_rows)
//   read <path> <auto|fasta|fastq> <want_qual 0|1> <keep_text 0|1>   ->  records, then per record: header / sequence / quality in hex
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../krust_amd/host/kmerust_host.h"

static std::vector<uint8_t> unhex(const std::string &hex) {
    std::vector<uint8_t> v;
    if (hex != "-")
        for (size_t i = 0; i + 1 < hex.size(); i += 2) v.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
    return v;
}
static void put_hex(const uint8_t *p, size_t n) {
    if (n == 0) printf("-");
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static std::vector<uint32_t> words(const std::string &s) {
    std::vector<uint32_t> v;
    if (s == "-") return v;
    std::istringstream es(s);
    std::string tok;
    while (std::getline(es, tok, ',')) v.push_back((uint32_t)strtoull(tok.c_str(), nullptr, 10));
    return v;
}

int main() {
    using namespace kmerust;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "keep") {
            FilterRule rule;
            unsigned long long lo, hi, nk;
            std::string w;
            in >> lo >> hi >> nk >> rule.min_fraction >> w;
            rule.min_count = (uint32_t)lo, rule.max_count = (uint32_t)hi, rule.min_kmers = nk;
            const std::vector<uint32_t> row = words(w);
            if (row.size() != KH_REC_WORDS) {
                puts("ERR row");
                continue;
            }
            printf("%d\n", filter_keeps(row.data(), rule) ? 1 : 0);
        } else if (cmd == "record") {
            std::string h, s, q;
            in >> h >> s >> q;
            const std::vector<uint8_t> hv = unhex(h), sv = unhex(s), qv = unhex(q);
            std::string out = "x";  // (appended, not assigned)
            append_record(out, std::string(hv.begin(), hv.end()), sv.data(), sv.size(), q == "-" ? nullptr : qv.data());
            put_hex(reinterpret_cast<const uint8_t *>(out.data()) + 1, out.size() - 1);
            printf("\n");
        } else if (cmd == "starts") {
            std::string h;
            in >> h;
            const std::vector<uint8_t> b = unhex(h);
            const std::vector<uint64_t> rs = record_starts(b.data(), b.size());
            for (size_t i = 0; i < rs.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long)rs[i]);
            printf("\n");
        } else if (cmd == "summary") {
            unsigned long long first;
            std::string w;
            in >> first >> w;
            const std::vector<uint32_t> rows = words(w);
            char *buf = nullptr;
            size_t len = 0;
            FILE *f = open_memstream(&buf, &len);
            write_summary_rows(f, rows.data(), rows.size() / KH_REC_WORDS, first);
            fclose(f);
            put_hex(reinterpret_cast<const uint8_t *>(buf), len);
            printf("\n");
            free(buf);
        } else if (cmd == "read") {
            std::string path, fmt;
            int want_qual = 0, keep_text = 0;
            in >> path >> fmt >> want_qual >> keep_text;
            const SequenceFormat f = fmt == "fasta" ? SequenceFormat::Fasta : fmt == "fastq" ? SequenceFormat::Fastq : SequenceFormat::Auto;
            try {
                std::string out;
                const BatchSink sink = [&](const Batch &b) {
                    const std::vector<uint64_t> rs = record_starts(b.bases.data(), b.bases.size());
                    char t[64];
                    snprintf(t, sizeof t, " batch:%llu:%zu:%zu:%zu", (unsigned long long)b.records, b.headers.size(), b.bases.size(), b.qual.size());
                    out += t;
                    for (size_t r = 0; r + 1 < rs.size(); ++r) {
                        out += " |";
                        auto hex = [&](const uint8_t *p, size_t n) {
                            out += " ";
                            if (!n) out += "-";
                            for (size_t i = 0; i < n; ++i) {
                                snprintf(t, sizeof t, "%02x", p[i]);
                                out += t;
                            }
                        };
                        const size_t s = rs[r], len = rs[r + 1] - s - 1;
                        if (r < b.headers.size()) hex(reinterpret_cast<const uint8_t *>(b.headers[r].data()), b.headers[r].size());
                        hex(b.bases.data() + s, len);
                        if (!b.qual.empty()) hex(b.qual.data() + s, len);
                    }
                };
                const uint64_t n = keep_text ? read_sequences(path, f, want_qual != 0, 1u << 20, sink, true)
                                             : read_sequences(path, f, want_qual != 0, 1u << 20, sink);
                printf("%llu%s\n", (unsigned long long)n, out.c_str());
            } catch (const Error &e) {
                printf("ERR %s\n", e.what());
            }
        } else {
            puts("ERR command");
        }
    }
    puts("FILTER_CHECK_DONE");
    return 0;
}
