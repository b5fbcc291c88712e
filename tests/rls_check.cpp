// TEST-ONLY stand-alone host program: the key code of the Envoy rate-limit
// service path (sentinel_amd/csrc/sf_rls.h: UTF-8 decoder / validator, running
// String.hashCode, blank test, flowId) against the answers of the Python model
// (tests/rls_model.py), built with -fsanitize=address,undefined by
// tests/test_rls_model.py.
//
// Case file, one case per line:  <hex bytes or -> <ok> <blank> <hash> <flow id> <hash of "ab|" + string>
// (all but ok are read only when ok is 1).  Every string is copied
// into a heap block of exactly its length, so a read past its end is reported.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define SF_RLS_KEYS_ONLY
#include "../sentinel_amd/csrc/sf_rls.h"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: rls_check CASES\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<char> line(1 << 20);
    unsigned cases = 0, failures = 0;
    while (std::fgets(line.data(), (int)line.size(), f)) {
        std::vector<char> hex(line.size());
        int ok = 0, blank = 0;
        long long hash = 0, id = 0, hash2 = 0;
        if (std::sscanf(line.data(), "%s %d %d %lld %lld %lld", hex.data(), &ok, &blank, &hash, &id, &hash2) != 6) continue;
        const size_t len = std::strcmp(hex.data(), "-") == 0 ? 0 : std::strlen(hex.data()) / 2;
        uint8_t* p = (uint8_t*)std::malloc(len ? len : 1);
        for (size_t i = 0; i < len; i++) {
            unsigned v = 0;
            std::sscanf(hex.data() + 2 * i, "%2x", &v);
            p[i] = (uint8_t)v;
        }
        sf::RlsKey k = sf::rls_key_begin();
        sf::rls_key_feed(k, len ? p : nullptr, (uint32_t)len);
        bool good = (int)k.ok == ok;
        if (good && ok) good = (int)k.blank == blank && (int32_t)k.h == (int32_t)hash && sf::rls_key_id(k) == (int64_t)id;
        // the same string after the prefix "ab|": the hash continues from the prefix's state, the key is not blank
        if (good && ok) {
            sf::RlsKey k2 = sf::rls_key_begin();
            sf::rls_key_cp(k2, 'a'); sf::rls_key_cp(k2, 'b'); sf::rls_key_cp(k2, '|');
            sf::rls_key_feed(k2, len ? p : nullptr, (uint32_t)len);
            good = k2.ok && !k2.blank && (int32_t)k2.h == (int32_t)hash2;
        }
        if (!good) {
            failures++;
            std::printf("case %u (%s): ok %d blank %d hash %d id %" PRId64 ", want %d %d %lld %lld\n", cases, hex.data(),
                        (int)k.ok, (int)k.blank, (int32_t)k.h, sf::rls_key_id(k), ok, blank, hash, id);
        }
        std::free(p);
        cases++;
    }
    std::fclose(f);
    std::printf("%u cases, %u failures\n", cases, failures);
    return failures ? 1 : 0;
}
