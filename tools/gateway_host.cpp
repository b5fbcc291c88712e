// gateway_host.cpp -- MEASUREMENT TOOL: the one-core rate of the engine's
// host-compilable gateway parser (sentinel_amd/csrc/sf_gateway.h: gw_entry, the
// function the kernel k_gw_args runs one lane per entry) on a batch that
// tools/gateway_bench.py wrote.  Built and run by that tool; no GPU.
//
// Input file: 8 uint32 {n, n_ent, n_val, n_str, n_bytes, R, n_desc, n_pat}, then
// the arrays in the order read below, each padded to 8 bytes.
// Output: one JSON line {"entries", "passes", "ns_per_entry_best", "checksum"}.
#define SF_GATEWAY_HOST_ONLY
#include "../sentinel_amd/csrc/sf_gateway.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <class T> static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n ? n : 1);
    const size_t bytes = n * sizeof(T), padded = (bytes + 7) & ~(size_t)7;
    std::vector<char> raw(padded ? padded : 1);
    if (padded && std::fread(raw.data(), 1, padded, f) != padded) { std::fprintf(stderr, "short file\n"); std::exit(2); }
    for (size_t i = 0; i < bytes; i++) ((char*)v.data())[i] = raw[i];
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: gateway_host batch.bin [passes]\n"); return 2; }
    const int passes = argc > 2 ? std::atoi(argv[2]) : 3;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const std::vector<uint32_t> h = take<uint32_t>(f, 8);
    const uint32_t n = h[0], n_ent = h[1], n_val = h[2], n_str = h[3], n_bytes = h[4], R = h[5], n_desc = h[6], n_pat = h[7];
    auto ts = take<int64_t>(f, n); auto count = take<int32_t>(f, n); auto flags = take<uint8_t>(f, n);
    auto res_off = take<uint32_t>(f, n + 1); auto res_id = take<uint32_t>(f, n_ent); auto res_mode = take<int32_t>(f, n_ent);
    auto val_off = take<uint32_t>(f, n + 1); auto val_field = take<uint32_t>(f, n_val); auto val_str = take<uint32_t>(f, n_val);
    auto str_off = take<uint32_t>(f, n_str + 1); auto bytes = take<uint8_t>(f, n_bytes); auto ev_index = take<uint32_t>(f, n);
    auto of = take<uint32_t>(f, R); auto desc = take<sf::GwDesc>(f, n_desc); auto pat = take<uint8_t>(f, n_pat);
    std::fclose(f);
    sf::GwTables t{of.data(), desc.data(), pat.data(), R, 1, 0};
    sf::GwBatch b{};
    b.n = n; b.n_ent = n_ent; b.n_val = n_val; b.n_str = n_str; b.n_total = n_ent;
    b.ts = ts.data(); b.count = count.data(); b.flags = flags.data(); b.res_off = res_off.data(); b.res_id = res_id.data();
    b.res_mode = res_mode.data(); b.val_off = val_off.data(); b.val_field = val_field.data(); b.val_str = val_str.data();
    b.str_off = str_off.data(); b.bytes = bytes.data(); b.ev_index = ev_index.data();
    std::vector<uint32_t> o_res(n_ent); std::vector<int64_t> o_ts(n_ent); std::vector<int32_t> o_cnt(n_ent);
    std::vector<uint8_t> o_fl(n_ent), o_na(n_ent), o_tag((size_t)n_ent * sf::GW_MAX_SLOTS);
    std::vector<uint64_t> o_bits((size_t)n_ent * sf::GW_MAX_SLOTS);
    sf::GwOut o{o_res.data(), o_ts.data(), o_cnt.data(), o_fl.data(), o_na.data(), o_tag.data(), o_bits.data()};
    double best = 1e300;
    for (int p = 0; p < passes; p++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t d = 0; d < n_ent; d++) sf::gw_entry(t, b, o, d);
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
        if (ns / n_ent < best) best = ns / n_ent;
    }
    uint64_t sum = 0;                                         // of every output: compared with the device's by the tool
    for (size_t k = 0; k < o_bits.size(); k++) sum += o_bits[k] * (k + 1) + o_tag[k];
    for (size_t k = 0; k < n_ent; k++) sum += (uint64_t)o_na[k] * 31 + o_res[k];
    std::printf("{\"entries\": %u, \"passes\": %d, \"ns_per_entry_best\": %.3f, \"checksum\": %llu}\n", n_ent, passes, best,
                (unsigned long long)sum);
    return 0;
}
