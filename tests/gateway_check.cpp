// gateway_check.cpp -- TEST ONLY: the engine's host-compilable gateway parser
// (sentinel_amd/csrc/sf_gateway.h: gw_hash, gw_equal, gw_contains, gw_match,
// gw_parse) against cases the Python model wrote, run under ASan + UBSan by
// tests/test_gateway_model.py.  Every value and pattern is copied into a heap
// block of exactly its length, so a read past a string's last byte is an
// AddressSanitizer report.
//
// Input: one case per line,
//   <parse> <match> <flags> <present 0|1> <pattern hex|-> <value hex|-> <tag> <bits hex>
// ("-": an empty string).  Output: "ok <cases>" or one line per mismatch, exit 1.
#define SF_GATEWAY_HOST_ONLY
#include "../sentinel_amd/csrc/sf_gateway.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static uint8_t* exact(const std::string& hex, uint32_t* len) {
    const std::string h = hex == "-" ? "" : hex;
    *len = (uint32_t)(h.size() / 2);
    uint8_t* p = (uint8_t*)std::malloc(*len);                     // (zero length: any read is out of bounds)
    for (uint32_t i = 0; i < *len; i++) p[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
    return p;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: gateway_check cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    long n = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        int parse, match, flags, present, tag;
        std::string pat_hex, val_hex, bits_hex;
        ls >> parse >> match >> flags >> present >> pat_hex >> val_hex >> tag >> bits_hex;
        uint32_t pl = 0, vl = 0;
        uint8_t* pat = exact(pat_hex, &pl);
        uint8_t* val = exact(val_hex, &vl);
        sf::GwSlot s{};
        s.field_id = 0; s.parse = parse; s.match = match; s.pat_off = 0; s.pat_len = pl;
        uint8_t got_tag = 0xEE;
        uint64_t got_bits = 0;
        sf::gw_parse(s, pat, present != 0, val, vl, (uint8_t)flags, &got_tag, &got_bits);
        const uint64_t want_bits = std::stoull(bits_hex, nullptr, 16);
        if (got_tag != (uint8_t)tag || got_bits != want_bits) {
            std::printf("case %ld: got (%u, %016llx), the model (%d, %016llx): %s\n", n, got_tag,
                        (unsigned long long)got_bits, tag, (unsigned long long)want_bits, line.c_str());
            bad++;
        }
        std::free(pat);
        std::free(val);
        n++;
    }
    if (bad) return 1;
    std::printf("ok %ld\n", n);
    return 0;
}
