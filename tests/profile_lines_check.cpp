// profile_lines_check.cpp -- drives the line writer of `kmerust query --sequences` (write_profile_lines, krust_amd/host/kmerust_host.cpp)
// without a device: tests/test_profile_host.py compiles this file with the host library's source and the recording kh_* stub
// (tests/host_asan/stub_kmerhip.cpp) with a plain g++.
// One case per input line:   <k> <summary|profile> <first ordinal> <hex of the flat bases, or -> <profile entries, comma separated, or ->
// One output line per case:  <records written> <hex of the bytes written, or ->
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../krust_amd/host/kmerust_host.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned k;
        std::string fmt, hex, entries;
        unsigned long long first;
        if (!(in >> k >> fmt >> first >> hex >> entries)) {
            puts("ERR parse");
            continue;
        }
        std::vector<uint8_t> bases;
        if (hex != "-")
            for (size_t i = 0; i + 1 < hex.size(); i += 2) bases.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
        std::vector<uint32_t> prof;
        if (entries != "-") {
            std::istringstream es(entries);
            std::string tok;
            while (std::getline(es, tok, ',')) prof.push_back((uint32_t)strtoull(tok.c_str(), nullptr, 10));
        }
        if (prof.size() != bases.size()) {
            puts("ERR sizes");
            continue;
        }
        char *buf = nullptr;
        size_t len = 0;
        FILE *f = open_memstream(&buf, &len);
        const uint64_t n = kmerust::write_profile_lines(f, bases.data(), prof.data(), bases.size(), k,
                                                        fmt == "profile" ? kmerust::ProfileFormat::Profile : kmerust::ProfileFormat::Summary, first);
        fclose(f);
        printf("%llu ", (unsigned long long)n);
        if (len == 0) printf("-");
        for (size_t i = 0; i < len; ++i) printf("%02x", (unsigned char)buf[i]);
        printf("\n");
        free(buf);
    }
    puts("PROFILE_LINES_CHECK_DONE");
    return 0;
}
