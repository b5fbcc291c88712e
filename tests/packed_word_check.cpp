// TEST-ONLY stand-alone host program: the sorted-event word (sf_decide.h).
// ev_pack -> ev_time / ev_count / ev_flags must give back the full-width
// values, through the two escapes where the word cannot hold them, for a
// SortedEv (what the device reads) and for a SegIO with and without words
// (the host build's full-width fallback).  Exit status 0: every case equal.
#include <cstdio>
#include <vector>

#include "../sentinel_amd/csrc/sf_decide.h"

using namespace sf;

// the flag byte ev_pack must produce (the rule stated independently of it)
static uint8_t want_flags(uint8_t f, uint8_t sr) {
    uint8_t fl = f & 0x0Fu;
    if ((f & SF_EV_BLOCKED) && !(f & SF_EV_EXIT)) return fl | EVF_SYSBLK | (uint8_t)(SYSR_OTHER << EVF_SYSREASON_SHIFT);
    if ((f & SF_EV_IN) && !(f & SF_EV_EXIT) && sr < SYS_INERT) return fl | EVF_SYSBLK | (uint8_t)(sr << EVF_SYSREASON_SHIFT);
    return fl;
}

int main() {
    const int64_t T0 = 1700000000000LL;
    const int64_t offs[] = {0, 1, 65534, 65535, 1000000000LL};
    const int32_t cnts[] = {-1, 0, 1, 255, 256, 70000};
    const uint8_t srs[] = {0, 1, 2, 3, 4, SYS_INERT, SYS_NONE};
    struct Ev { int64_t ts; int32_t c; uint8_t f, sr; };
    std::vector<Ev> evs;
    evs.push_back({T0, 1, SF_EV_IN, SYS_NONE});                          // event 0 fixes the batch's first time
    for (int64_t o : offs)
        for (int32_t c : cnts)
            for (int f = 0; f < 256; f++)                                // every caller flag byte
                for (uint8_t sr : srs) {
                    // (the planner's mask only matters for IN entries: one value for the others)
                    if (sr != SYS_NONE && !((f & SF_EV_IN) && !(f & SF_EV_EXIT))) continue;
                    evs.push_back({T0 + o, c, (uint8_t)f, sr});
                }
    const uint32_t n = (uint32_t)evs.size();
    // the "sort": sorted position j holds submission index perm[j] = n - 1 - j
    std::vector<int64_t> b_ts(n), s_ts(n);
    std::vector<int32_t> b_cnt(n), s_cnt(n);
    std::vector<uint8_t> s_fl(n);
    std::vector<uint32_t> perm(n), meta(n);
    for (uint32_t i = 0; i < n; i++) { b_ts[i] = evs[i].ts; b_cnt[i] = evs[i].c; }
    uint32_t far = 0, cesc = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t i = n - 1 - j;
        perm[j] = i;
        meta[j] = ev_pack(evs[i].ts, b_ts[0], evs[i].f, evs[i].sr, evs[i].c);
        s_ts[j] = evs[i].ts; s_cnt[j] = evs[i].c; s_fl[j] = want_flags(evs[i].f, evs[i].sr);
        far += (meta[j] & 0xffffu) == PV_DTS_FAR;
        cesc += (meta[j] >> 24) == 0;
    }
    SortedEv sv{meta.data(), perm.data(), b_ts.data(), b_cnt.data(), 0};
    ev_open(sv);
    SegIO packed{};                                   // words only: no full-width array to fall back to
    packed.ev = sv;
    SegIO full{s_ts.data(), s_cnt.data(), s_fl.data()};   // positional, as the host simulator builds it
    long bad = 0;
    auto check = [&](const char* what, uint32_t j, long long got, long long want) {
        if (got == want) return;
        if (bad++ < 10) std::printf("%s j=%u: got %lld want %lld (word %08x)\n", what, j, got, want, meta[j]);
    };
    for (uint32_t j = 0; j < n; j++) {
        check("SortedEv time", j, ev_time(sv, j), s_ts[j]);
        check("SortedEv count", j, ev_count(sv, j), s_cnt[j]);
        check("SortedEv flags", j, ev_flags(sv, j), s_fl[j]);
        const uint32_t m = ev_word(packed, j);
        check("SegIO word", j, m, meta[j]);
        check("SegIO time", j, ev_time(packed, m, j), s_ts[j]);
        check("SegIO count", j, ev_count(packed, m, j), s_cnt[j]);
        check("SegIO flags", j, ev_flags(m), s_fl[j]);
        const uint32_t mf = ev_word(full, j);
        check("fallback time", j, ev_time(full, mf, j), s_ts[j]);
        check("fallback count", j, ev_count(full, mf, j), s_cnt[j]);
        check("fallback flags", j, ev_flags(mf), s_fl[j]);
        check("fallback time(j)", j, ev_time(full, j), s_ts[j]);
        check("fallback count(j)", j, ev_count(full, j), s_cnt[j]);
        check("fallback flags(j)", j, ev_flags(full, j), s_fl[j]);
    }
    // the escapes were taken exactly where the word cannot hold the value
    for (uint32_t j = 0; j < n; j++) {
        const int64_t d = s_ts[j] - b_ts[0];
        check("far escape", j, (meta[j] & 0xffffu) == PV_DTS_FAR, d >= 65535);
        check("count escape", j, (meta[j] >> 24) == 0, s_cnt[j] < 1 || s_cnt[j] > 255);
    }
    std::printf("%u events, %u time escapes, %u count escapes, %ld mismatches\n", n, far, cesc, bad);
    return bad ? 1 : (far && cesc ? 0 : 2);
}
