// TEST-ONLY: the chunk solver of the concurrency-token walk (sf_concur.h,
// cc_solve_chunk) on the host wave, against the reference's one-by-one loop
// (ConcurrentClusterFlowChecker.java:57-70, :96-98) on random chunks.
// Usage: concur_check [chunks] [seed].  Prints the outcome counts; exit 1 on
// the first difference, 2 when one of the three outcomes never occurred.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#define SF_HOSTSIM
#include "../../sentinel_amd/csrc/sf_concur.h"

using namespace sf;

// the reference, one request at a time, Java int arithmetic
static uint64_t serial(const int32_t* d, int L, double thr, int32_t* x) {
    uint32_t v = (uint32_t)*x;
    uint64_t pass = 0;
    for (int l = 0; l < L; l++) {
        const uint32_t nv = v + (uint32_t)d[l];
        if (d[l] < 0) v = nv;
        else if (d[l] > 0 && !((double)(int32_t)nv > thr)) { v = nv; pass |= 1ull << l; }
    }
    *x = (int32_t)v;
    return pass;
}

int main(int argc, char** argv) {
    const long chunks = argc > 1 ? atol(argv[1]) : 100000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 20240607ull);
    auto uni = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    long all_pass = 0, one_round_blocked = 0, multi_round = 0;
    CcWaveHost w;
    for (long c = 0; c < chunks; c++) {
        const int L = (int)uni(1, 64);
        const int rel_pct = (int)uni(0, 60);
        const int regime = (int)uni(0, 9);
        // thresholds from 0 to above INT32_MAX; most near the counts in play so that all regimes occur
        double thr;
        if (regime == 0) thr = 0;
        else if (regime == 1) thr = (double)INT32_MAX + (double)uni(1, 1000000);
        else if (regime == 2) thr = (double)uni(INT32_MAX - 200, INT32_MAX);
        else thr = (double)uni(1, 200) + (regime == 3 ? 0.5 : 0.0);
        const bool big = regime == 2 || uni(0, 19) == 0;          // some counts near INT32_MAX
        int32_t x0;
        if (regime == 2) x0 = (int32_t)uni(INT32_MAX - 300, INT32_MAX);
        else if (regime == 1) x0 = (int32_t)uni(-100, 100);
        else x0 = (int32_t)uni(-20, (int64_t)thr + 20);
        CcWaveHost::Vec d{};
        for (int l = 0; l < L; l++) {
            int32_t cnt = (int32_t)uni(1, 5);
            if (big && uni(0, 9) == 0) cnt = (int32_t)uni(INT32_MAX - 5, INT32_MAX);
            d.v[l] = uni(0, 99) < rel_pct ? -cnt : cnt;
        }
        int32_t xs = x0, xg = x0;
        const uint64_t want = serial(d.v, L, thr, &xs);
        CcSolveCount cnt;
        const uint64_t got = cc_solve_chunk(w, d, thr, &xg, &cnt);
        if (got != want || xg != xs) {
            printf("chunk %ld differs: L=%d thr=%.1f x0=%d pass %016llx want %016llx x %d want %d\n", c, L, thr, x0,
                   (unsigned long long)got, (unsigned long long)want, xg, xs);
            return 1;
        }
        if (cnt.all_pass) all_pass++;
        else if (cnt.rounds == 1) one_round_blocked++;       // the first failure, then the all-blocked shortcut
        else multi_round++;
    }
    printf("chunks %ld all_pass %ld one_round_all_blocked %ld multi_round %ld\n", chunks, all_pass, one_round_blocked,
           multi_round);
    return all_pass && one_round_blocked && multi_round ? 0 : 2;
}
