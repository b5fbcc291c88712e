// sf_sysx.h — SystemRule on a resource-sharded node: the per-window exchange
// (product code; host-compilable for the CPU tests in tests/hostsim).
//
// SystemRuleManager.checkSystem (SystemRuleManager.java:291-348) reads the
// node-wide Constants.ENTRY_NODE.  With the resources hash-sharded over the
// GPUs of a node, rank r decides only its events, but an IN entry's system
// verdict depends on the passes of every earlier IN entry of the node.  For the
// inbound-QPS check (`passQps + acquireCount > qps`, :303-307; passQps =
// ENTRY_NODE's pass sum over the valid buckets / intervalSec,
// StatisticNode.java:205-214) the node-wide state an entry reads is one
// number, P(i) = P_p + (passes of IN entries of the node in [p, i)), so the
// ranks exchange per-window aggregates instead of events:
//
//  - the node's events carry global sequence numbers (submission order; time
//    is non-decreasing in it); a *plan window* is a run of events inside one
//    g-ms cell, g = gcd(bucket length, 1000), so it lies inside one
//    ENTRY_NODE second bucket and one minute bucket;
//  - ENTRY_NODE is identical on every rank and exact at seq s_p (every event
//    of the node before s_p is decided);
//  - each rank bins its undecided IN entries of [lo, hi) (seq space, SX_B
//    bins): u = sum of acquireCounts of the entries that can still pass (an
//    entry its first ParamFlow rule certainly blocks, sf_system.h
//    param_inert, counts 0), n = entries, min / max acquireCount;
//  - after an all-gather of those messages every rank holds the node-wide
//    prefix of u at every bin boundary, so it classifies whole bins the same
//    way: all entries certainly fire the QPS check (P_p / intervalSec + cmin >
//    qps: P only grows), all certainly pass it (even if every entry counted in
//    u before the bin's end passed), or the bin is the crossing bin, which the
//    next level splits into SX_B bins; a one-sequence-number bin is exact;
//  - q = the first crossing entry (or the window end): every IN entry of the
//    node in [s_p, q) has a certain system verdict, each rank decides its own
//    events before q with the verdicts forced (the ordinary pipeline), packs
//    its ENTRY_NODE contribution of them (one second and one minute bucket,
//    SX_DELTA words), and the next round's first message carries it: every
//    rank adds the node's sum and ENTRY_NODE is exact at q.
//
// The entry at s_p is always classified (its prefix is exact), so each round
// progresses.  Per round the exchange is SX_WORDS * 8 B per rank per level
// (<= 4.3 KB; about three levels per round).  Eligible SystemRules read only
// the QPS check (and the CPU check, a fixed input): no thread, average-RT or
// BBR check can fire.  The other kinds take the same rounds with the wide
// message format (below, "the wide kinds").
#pragma once
#include "sf_system.h"

namespace sf {

constexpr int SX_B = 128;                 // bins per level
constexpr int SX_DELTA = 16;              // int64 words of a rank's ENTRY_NODE contribution
constexpr int SX_WORDS = SX_DELTA + 4 * SX_B;
static_assert(SX_WORDS * 8 == SF_SYSX_MSG_BYTES, "sentinel_flow.h SF_SYSX_MSG_BYTES");
// message words: delta [0, 16): key (plan window index, -1: none), second
// bucket (pass, block, succ, rt, exc, touched), minute bucket (same), minRt of
// each, threads; then u[SX_B], n[SX_B], cmin[SX_B], cmax[SX_B]
enum : int { SXD_KEY = 0, SXD_SEC = 1, SXD_MIN = 7, SXD_MRS = 13, SXD_MRM = 14, SXD_THR = 15 };
enum : int { SXM_U = SX_DELTA, SXM_N = SX_DELTA + SX_B, SXM_CMIN = SX_DELTA + 2 * SX_B, SXM_CMAX = SX_DELTA + 3 * SX_B };

// one round's plan (host; identical on every rank)
struct SxPlan {
    int64_t lo, hi, w;            // level range [lo, hi) of sequence numbers, bin width
    int64_t ub;                   // node-wide u over [s_p, lo)
    int64_t P;                    // ENTRY_NODE pass sum the QPS check reads in this window (at s_p)
    int64_t q;                    // result: the sub-batch is [s_p, q)
    int32_t done, level;
};

// SystemRules whose verdicts the exchange decides: the QPS check and the CPU
// check only (SystemRuleManager.java:303-340: maxThread / maxRt unset, the
// load check's BBR never reached)
SF_HD bool sx_rule_ok(const SysRule& r) {
    return r.max_thread == INT64_MAX && r.max_rt == INT64_MAX && !(r.load_set && r.cur_load > r.highest_load);
}

SF_HD int64_t sx_sat(int64_t a, int64_t b) {            // (a, b >= 0)
    return a > INT64_MAX - b ? INT64_MAX : a + b;
}

// The system verdict of an IN entry of [s_p, q) with acquireCount c: the
// classification made it certain, so the QPS check fires iff it fires at the
// exact P_p (sys_classify's order: qps first, then the fixed CPU check).
SF_HD uint8_t sx_reason(const SysRule& r, int64_t P, double interval_sec, int32_t c) {
    if ((double)P / interval_sec + c > r.qps) return 0;
    if (r.cpu_set && r.cur_cpu > r.highest_cpu) return 4;
    return SYS_NONE;
}

SF_HD void sx_begin(SxPlan* pl, int64_t lo, int64_t hi) {
    pl->lo = lo; pl->hi = hi;
    pl->w = hi > lo ? (hi - lo + SX_B - 1) / SX_B : 1;
    pl->ub = 0; pl->q = hi; pl->done = hi <= lo ? 1 : 0; pl->level = 0;
}

// One level: the node-wide bins (N messages of SX_WORDS words, rank order)
// -> the crossing bin, the next level's range, or q.  pl->P is set.
SF_HD void sx_reduce(const int64_t* msgs, int N, SxPlan* pl, const SysRule& r, double interval_sec) {
    if (pl->done) return;
    int64_t G = pl->ub;
    const double base = (double)pl->P / interval_sec;
    for (int b = 0; b < SX_B; b++) {
        const int64_t lo_b = pl->lo + (int64_t)b * pl->w;
        if (lo_b >= pl->hi) break;
        int64_t U = 0, n = 0, cmn = INT64_MAX, cmx = INT64_MIN;
        for (int k = 0; k < N; k++) {
            const int64_t* m = msgs + (size_t)k * SX_WORDS;
            U = sx_sat(U, m[SXM_U + b]); n += m[SXM_N + b];
            if (m[SXM_CMIN + b] < cmn) cmn = m[SXM_CMIN + b];
            if (m[SXM_CMAX + b] > cmx) cmx = m[SXM_CMAX + b];
        }
        if (n == 0) continue;                                   // (u == 0)
        const bool fire_all = base + (double)cmn > r.qps;     // (the batch has no acquireCount < 0)
        if (!fire_all) {
            // the largest P an entry of the bin can read: every counted entry
            // before it passed (a bin of one sequence number: exactly its prefix)
            const int64_t top = sx_sat(sx_sat(pl->P < 0 ? 0 : pl->P, G), pl->w == 1 ? 0 : U);
            const bool pass_all = !((double)top / interval_sec + (double)cmx > r.qps);
            if (!pass_all) {
                if (pl->w == 1) { pl->q = lo_b; pl->done = 1; return; }
                pl->ub = G;
                pl->lo = lo_b;
                pl->hi = lo_b + pl->w < pl->hi ? lo_b + pl->w : pl->hi;
                pl->w = (pl->hi - pl->lo + SX_B - 1) / SX_B;
                pl->level++;
                return;
            }
        }
        G = sx_sat(G, U);
    }
    pl->q = pl->hi;
    pl->done = 1;
}

// ENTRY_NODE += the node's contribution of the last sub-batch (the sum of the
// ranks' deltas of one plan window: adds commute inside one bucket), with
// LeapArray.currentWindow's reset rule (a bucket of an older window is reset;
// ENTRY_NODE never borrows).
SF_HD void sx_merge(Bucket& bk, int64_t ws, const int64_t* s, int64_t minrt, int64_t max_rt) {
    if (bk.ws != ws) {
        if (bk.ws != WS_NONE && ws < bk.ws) return;        // older than the slot: a throwaway window
        bk = fresh_bucket(ws, max_rt);
    }
    bk.pass = wadd(bk.pass, s[0]); bk.block = wadd(bk.block, s[1]);
    bk.succ = wadd(bk.succ, s[2]); bk.rt = wadd(bk.rt, s[3]); bk.exc = wadd(bk.exc, s[4]);
    if (minrt < bk.min_rt) bk.min_rt = minrt;
}
// (stride: words per message, SX_WORDS or the wide kinds' SXW_WORDS)
SF_HD void sx_apply_delta(const int64_t* msgs, int N, EntryNode* en, int64_t ws_sec, int S, int wl, int64_t ws_min,
                          int64_t max_rt, size_t stride = SX_WORDS) {
    int64_t sec[6] = {0, 0, 0, 0, 0, 0}, mn[6] = {0, 0, 0, 0, 0, 0}, mrs = INT64_MAX, mrm = INT64_MAX, thr = 0;
    bool any = false;
    for (int k = 0; k < N; k++) {
        const int64_t* d = msgs + (size_t)k * stride;
        if (d[SXD_KEY] < 0) continue;
        any = true;
        for (int f = 0; f < 6; f++) { sec[f] = wadd(sec[f], d[SXD_SEC + f]); mn[f] = wadd(mn[f], d[SXD_MIN + f]); }
        if (d[SXD_MRS] < mrs) mrs = d[SXD_MRS];
        if (d[SXD_MRM] < mrm) mrm = d[SXD_MRM];
        thr = wadd(thr, d[SXD_THR]);
    }
    if (!any) return;
    if (sec[5]) sx_merge(en->second[(int)((ws_sec / wl) % S)], ws_sec, sec, mrs, max_rt);
    if (mn[5]) sx_merge(en->minute[(int)((ws_min / 1000) % MINUTE)], ws_min, mn, mrm, max_rt);
    en->threads = wadd(en->threads, thr);
}

// ---------------------------------------------------------------- the wide kinds
// SystemRules with a thread, average-RT or firing load (BBR) check (sx_rule_ok
// false) go through the same rounds with a second message format.  Everything
// sys_classify (sf_system.h) reads at an IN entry is a prefix, over the node's
// events since s_p, of commutative sums and minima: the exit side SysExitQ
// (certain and uncertain live exits) and the entry side SysEntQ (entries that
// can still pass).  An exit's entry is an event of the same resource, so of
// the same rank: each rank forms both with sys_exit_q over its own events,
// "certain" read locally (the entry lies before the rank's lp and its verdict
// is known, or in an earlier batch), "uncertain" = the entry lies at or after
// lp.  Per level a rank sends the per-bin sums of those (SXW_B bins); added
// over the ranks and scanned over the bins they give every rank the node-wide
// prefix at every bin boundary.  sxw_range then decides whether every IN entry
// of a bin has one certain outcome (pass, or block with one reason) under
// every prefix between the bin's two boundaries; a bin of one sequence number
// is sys_classify on its exact prefix, the single-engine classification.
// Settled bins are skipped and kept in a list (identical on every rank: the
// mask of the round), the first unsettled bin is the next level's range.
//
// Sums that saturate (xu_pos, and the RT check's in-bin extremes) travel as
// two plain sums, of the low and of the high 32 bits of every term: plain
// integer adds commute, so a message does not depend on the order of the
// atomics that built it, and the reader saturates once (sxw_join).
constexpr int SXW_B = 64;                 // bins per level
enum : int {
    SXW_XC = 0, SXW_XC_C, SXW_XC_RT, SXW_XU, SXW_XU_C, SXW_XUP_LO, SXW_XUP_HI, SXW_XU_BAD, SXW_XC_MIN, SXW_XU_MIN,
    SXW_NE,                               // SysExitQ of the bin (nneg: refused by the header)
    SXW_NB, SXW_NB_C,                     // SysEntQ: entries that can still pass (not inert)
    SXW_CMIN, SXW_CMAX,                   // acquireCount range of the bin's IN entries
    // certain exits of the bin, d = rt - maxRt * c: sum of max(0, d), of max(0, -d)
    SXW_RP_LO, SXW_RP_HI, SXW_RN_LO, SXW_RN_HI,
    // certain exits the in-bin bounds cannot take: c <= 0, rt < 0, |d| >= 2^62
    SXW_XBAD,
    SXW_F
};
constexpr int SXW_WORDS = SX_DELTA + SXW_F * SXW_B;       // word of field f, bin b: SX_DELTA + f * SXW_B + b
static_assert(SXW_WORDS * 8 == SF_SYSX_WIDE_MSG_BYTES, "sentinel_flow.h SF_SYSX_WIDE_MSG_BYTES");
static_assert(SF_SYSX_WIDE_MSG_BYTES <= 16384, "the wide message is at most 16 KiB per rank and level");

// the identity of field f (an empty bin)
SF_HD int64_t sxw_identity(int f) {
    return (f == SXW_XC_MIN || f == SXW_XU_MIN || f == SXW_CMIN) ? INT64_MAX : (f == SXW_CMAX ? INT64_MIN : 0);
}
// a saturating sum from its two parts
SF_HD int64_t sxw_join(int64_t lo, int64_t hi) {
    const __int128 v = ((__int128)hi << 32) + (__int128)lo;
    return v > (__int128)INT64_MAX ? INT64_MAX : (int64_t)v;
}

// one bin, node-wide
struct SxwBin {
    SysExitQ x;
    SysEntQ e;
    int64_t cmin, cmax, rpos, rneg, xbad;
};
// the ranks' messages (N x SXW_WORDS, any rank order: every field is a plain sum or a minimum) -> bin b
SF_HD SxwBin sxw_bin(const int64_t* msgs, int N, int b) {
    int64_t s[SXW_F];
    for (int f = 0; f < SXW_F; f++) s[f] = sxw_identity(f);
    for (int k = 0; k < N; k++) {
        const int64_t* m = msgs + (size_t)k * SXW_WORDS + SX_DELTA + b;
        for (int f = 0; f < SXW_F; f++) {
            const int64_t v = m[(size_t)f * SXW_B];
            if (f == SXW_XC_MIN || f == SXW_XU_MIN || f == SXW_CMIN) { if (v < s[f]) s[f] = v; }
            else if (f == SXW_CMAX) { if (v > s[f]) s[f] = v; }
            else s[f] = wadd(s[f], v);
        }
    }
    SxwBin o;
    o.x.clear(); o.e.clear();
    o.x.xc = s[SXW_XC]; o.x.xc_c = s[SXW_XC_C]; o.x.xc_rt = s[SXW_XC_RT];
    o.x.xu = s[SXW_XU]; o.x.xu_c = s[SXW_XU_C]; o.x.xu_pos = sxw_join(s[SXW_XUP_LO], s[SXW_XUP_HI]);
    o.x.xu_bad = s[SXW_XU_BAD]; o.x.xc_min = s[SXW_XC_MIN]; o.x.xu_min = s[SXW_XU_MIN]; o.x.ne = s[SXW_NE];
    o.e.nb = s[SXW_NB]; o.e.nb_c = s[SXW_NB_C];
    o.cmin = s[SXW_CMIN]; o.cmax = s[SXW_CMAX];
    o.rpos = sxw_join(s[SXW_RP_LO], s[SXW_RP_HI]); o.rneg = sxw_join(s[SXW_RN_LO], s[SXW_RN_HI]);
    o.xbad = s[SXW_XBAD];
    return o;
}

// The outcome every IN entry of a bin shares, or -1.  x0 / e0: the node-wide
// prefixes at the bin's start, bin: its sums, so an entry of the bin reads
// some (x, e) with x0 <= x <= x0 + bin.x and e <= e0 + bin.e, field by field
// (the sums are monotone: a bin with a certain exit of acquireCount <= 0 or
// rt < 0 is refused, xbad).  Each check is certain for the whole bin only
// when it is at both ends of every range it reads, in sys_classify's own
// arithmetic where that is monotone, in exact integers where it is not (the
// RT quotient, below).  Returns -2 certain pass, -1 not settled, else the
// block reason, in checkSystem's order.
SF_HD int sxw_range(const SysRule& r, const SysBase& b, int S, double interval_sec, const SysExitQ& x0,
                    const SysEntQ& e0, const SxwBin& bin) {
    constexpr int64_t BIG = (int64_t)1 << 52;
    SysExitQ x1 = x0;
    x1.add(bin.x);
    SysEntQ e1 = e0;
    e1.add(bin.e);
    int st[5];
    // the sums below must not wrap: anything this large is left to the exact one-number bins
    if (bin.xbad || b.P > BIG || b.P < -BIG || e1.nb_c > BIG || e1.nb_c < 0) return -1;
    // qps: P in [P_p, P_p + e1.nb_c], monotone in c
    {
        const double lo = (double)b.P / interval_sec, hi = (double)(b.P + e1.nb_c) / interval_sec;
        const bool fire = lo + (double)bin.cmin > r.qps, pass = !(hi + (double)bin.cmax > r.qps);
        st[0] = fire ? CK_FIRE : (pass ? CK_PASS : CK_UNKNOWN);
    }
    // thread: T - x.xc in [T - x1.xc, T - x0.xc], entries up to e1.nb
    const int64_t t_lo = b.T - x1.xc, t_hi = b.T + e1.nb - x0.xc, t_top = b.T + x1.ne - x0.xc;
    const bool t_ok = b.T >= INT32_MIN && b.T <= INT32_MAX && t_lo >= INT32_MIN && t_top <= INT32_MAX &&
                      b.T - x0.xc >= INT32_MIN;
    {
        const bool fire = t_ok && t_lo > r.max_thread, pass = t_ok && !(t_hi > r.max_thread);
        st[1] = fire ? CK_FIRE : (pass ? CK_PASS : CK_UNKNOWN);
    }
    // rt: the reference compares the double quotient RT / SU with maxRt.  With
    // 0 <= maxRt < 2^20, 0 <= SU < 2^32 and 0 <= RT < 2^52 both operands are exact
    // doubles and the quotient is correctly rounded, so it exceeds maxRt exactly
    // when D = RT - maxRt * SU > 0: D >= 1 puts the exact quotient at or above
    // maxRt + 2^-32, a double, and rounding is monotone.  Inside the bin D moves
    // between D0 - rneg and D0 + rpos.
    if (r.max_rt == INT64_MAX) st[2] = CK_PASS;
    else {
        const int64_t RT0 = wadd(b.RT, x0.xc_rt), SU0 = wadd(b.SU, x0.xc_c);
        const int64_t RT1 = wadd(b.RT, x1.xc_rt), SU1 = wadd(b.SU, x1.xc_c);
        const bool small = r.max_rt >= 0 && r.max_rt < ((int64_t)1 << 20) && b.RT >= 0 && b.SU >= 0 &&
                           x0.xc_rt >= 0 && x0.xc_c >= 0 && x1.xc_rt >= 0 && x1.xc_c >= 0 && RT0 >= 0 && RT1 >= 0 &&
                           RT1 < BIG && x1.xc_rt < BIG && b.RT < BIG && SU0 >= 0 && SU1 >= 0 &&
                           SU1 < ((int64_t)1 << 32) && x1.xc_c < ((int64_t)1 << 32) && b.SU < ((int64_t)1 << 32) &&
                           bin.rpos < BIG && bin.rneg < BIG;
        if (!small || (x1.xu != 0 && x1.xu_bad != 0)) st[2] = CK_UNKNOWN;
        else {
            const int64_t D0 = RT0 - r.max_rt * SU0;                       // |D0| < 2^53
            const __int128 worst = (__int128)D0 + bin.rpos + (__int128)x1.xu_pos;
            const bool pass = worst <= 0;                                  // every subset of the uncertain exits too
            const bool fire = x1.xu == 0 && SU0 > 0 && D0 - bin.rneg > 0;
            st[2] = fire ? CK_FIRE : (pass ? CK_PASS : CK_UNKNOWN);
        }
    }
    // load (BBR): monotone in the thread count, maxSuccessQps and minRt, so the
    // extremes sit at the ends of the ranges (sys_classify's expressions)
    if (!(r.load_set && r.cur_load > r.highest_load)) st[3] = CK_PASS;
    else if (!t_ok || x1.xu_bad || b.cur_succ < 0 || b.cur_succ > BIG || b.other_max_succ < 0 || x0.xc_c < 0 ||
             x1.xc_c < x0.xc_c || x1.xc_c > BIG || x1.xu_c < 0 || x1.xu_c > BIG)
        st[3] = CK_UNKNOWN;
    else {
        const int64_t cur_lo = b.cur_succ + x0.xc_c, cur_hi = b.cur_succ + x1.xc_c + x1.xu_c;
        int64_t ms_lo = cur_lo > b.other_max_succ ? cur_lo : b.other_max_succ;
        int64_t ms_hi = cur_hi > b.other_max_succ ? cur_hi : b.other_max_succ;
        ms_lo = ms_lo > 1 ? ms_lo : 1; ms_hi = ms_hi > 1 ? ms_hi : 1;
        int64_t mr_hi = b.min_rt < x0.xc_min ? b.min_rt : x0.xc_min;          // the fewest exits seen
        int64_t mr_lo = b.min_rt < x1.xc_min ? b.min_rt : x1.xc_min;          // every exit up to the bin's end
        mr_lo = mr_lo < x1.xu_min ? mr_lo : x1.xu_min;
        mr_hi = mr_hi > 1 ? mr_hi : 1; mr_lo = mr_lo > 1 ? mr_lo : 1;
        const double rhs_lo = (double)ms_lo * S / interval_sec * (double)mr_lo / 1000;
        const double rhs_hi = (double)ms_hi * S / interval_sec * (double)mr_hi / 1000;
        const int32_t th_lo = (int32_t)t_lo, th_hi = (int32_t)t_hi;
        const bool fire = th_lo > 1 && th_lo > rhs_hi;
        const bool pass = !(th_hi > 1 && th_hi > rhs_lo);
        st[3] = fire ? CK_FIRE : (pass ? CK_PASS : CK_UNKNOWN);
    }
    st[4] = (r.cpu_set && r.cur_cpu > r.highest_cpu) ? CK_FIRE : CK_PASS;
    for (int k = 0; k < 5; k++) {
        if (st[k] == CK_PASS) continue;
        return st[k] == CK_FIRE ? k : -1;
    }
    return -2;
}

// a run of settled bins: the IN entries with sequence numbers in [lo, hi) get `outcome`
struct SxwSeg {
    int64_t lo, hi;
    int64_t outcome;              // the forced reason, or SYS_NONE
};
constexpr int SXW_MAX_LEVELS = 64;
constexpr int SXW_MAX_SEGS = (SXW_MAX_LEVELS + 2) * SXW_B;

// one round's plan (host; identical on every rank)
struct SxwPlan {
    int64_t lo, hi, w;            // level range [lo, hi) of sequence numbers, bin width
    int64_t q;                    // result: the sub-batch is [s_p, q)
    int32_t done, level;
    SysBase base;                 // ENTRY_NODE at s_p (sys_base)
    SysExitQ x;                   // node-wide prefixes over [s_p, lo); e leaves out the
    SysEntQ e;                    //   entries of bins settled as blocked
    int32_t nseg, overflow;       // settled runs so far (segs), list full
};

SF_HD void sxw_begin(SxwPlan* pl, int64_t lo, int64_t hi) {
    pl->lo = lo; pl->hi = hi;
    pl->w = hi > lo ? (hi - lo + SXW_B - 1) / SXW_B : 1;
    pl->q = hi; pl->done = hi <= lo ? 1 : 0; pl->level = 0;
    pl->x.clear(); pl->e.clear();
    pl->nseg = 0; pl->overflow = 0;
}

// One level: sx_reduce's loop with the range test.  segs [SXW_MAX_SEGS]: the
// settled runs of the round, in sequence order (neighbours with one outcome joined).
SF_HD void sxw_reduce(const int64_t* msgs, int N, SxwPlan* pl, SxwSeg* segs, const SysRule& r, int S,
                      double interval_sec) {
    if (pl->done) return;
    for (int b = 0; b < SXW_B; b++) {
        const int64_t lo_b = pl->lo + (int64_t)b * pl->w;
        if (lo_b >= pl->hi) break;
        const int64_t hi_b = lo_b + pl->w < pl->hi ? lo_b + pl->w : pl->hi;
        const SxwBin bin = sxw_bin(msgs, N, b);
        if (bin.x.ne == 0) { pl->x.add(bin.x); continue; }      // exits only: the prefix moves on
        int o;
        if (pl->w == 1) {
            bool any = false;                                    // one entry: its exact prefix
            o = sys_classify(r, pl->base, S, interval_sec, pl->x, pl->e, (int32_t)bin.cmin, &any);
        } else {
            o = sxw_range(r, pl->base, S, interval_sec, pl->x, pl->e, bin);
        }
        if (o == -1) {
            if (pl->w == 1) { pl->q = lo_b; pl->done = 1; return; }
            pl->lo = lo_b; pl->hi = hi_b;
            pl->w = (pl->hi - pl->lo + SXW_B - 1) / SXW_B;
            pl->level++;
            return;
        }
        const int64_t oc = o >= 0 ? o : (int64_t)SYS_NONE;
        if (pl->nseg > 0 && segs[pl->nseg - 1].outcome == oc) segs[pl->nseg - 1].hi = hi_b;   // (no entry between them)
        else if (pl->nseg < SXW_MAX_SEGS) segs[pl->nseg++] = SxwSeg{lo_b, hi_b, oc};
        else pl->overflow = 1;
        pl->x.add(bin.x);
        if (o == -2) pl->e.add(bin.e);                           // blocked entries never count
    }
    pl->q = pl->hi;
    pl->done = 1;
}

}  // namespace sf

#ifndef SF_HOSTSIM
namespace sf {
// ---- launchers (sf_system.hip; sf_entry.hip for the delta) ----
struct SxArgs {
    DevBatch b;                   // this rank's whole batch (base 0)
    const int64_t* seq;           // its global sequence numbers (increasing)
    int64_t* msg;                 // this rank's message [SX_WORDS]
    SysRule r;
    int S, wl, interval;
    int64_t max_rt;
    double interval_sec;
    DevState st;                  // (param_inert probes)
    uint8_t* ibuf;                // [n] inert flags of the round (written at level 0)
    int64_t g, c0;                // plan-window cell length, the node's first cell
    const uint8_t* vstatus;       // the batch's verdicts, known before lp (wide kinds: certain exits)
};
// per batch: out[0..4] = first cell, last cell, last seq + 1, any IN entry with acquireCount < 0, n
hipError_t sx_header(const SxArgs& a, int64_t* out, hipStream_t s);
// per batch: out[k] = the first sequence number of this rank's events in plan window k (INT64_MAX: none)
hipError_t sx_winfirst(const SxArgs& a, int64_t* out, uint32_t nw, hipStream_t s);
// one level: clear this rank's bins (level 0 keeps the delta) and bin its IN entries of the plan's range
hipError_t sx_stats(const SxArgs& a, const SxPlan& pl, uint32_t lp, bool level0, hipStream_t s);
// *out = this rank's first event from lp with seq >= q
hipError_t sx_locate(const SxArgs& a, uint32_t lp, int64_t q, uint32_t* out, hipStream_t s);
// forced system verdicts of this rank's events [lp, lq) (P: ENTRY_NODE's pass sum at s_p)
hipError_t sx_mask(const SxArgs& a, uint8_t* mask, uint32_t lp, uint32_t lq, int64_t P, hipStream_t s);
// no delta in the message (key -1)
hipError_t sx_nodelta(int64_t* msg, hipStream_t s);
// the wide kinds (a.msg: [SXW_WORDS]): one level's bins of this rank's events from lp in the plan's range
hipError_t sxw_stats(const SxArgs& a, const SxwPlan& pl, uint32_t lp, bool level0, hipStream_t s);
// forced system verdicts of this rank's events [lp, lq) from the round's settled runs (device copy, sequence order)
hipError_t sxw_mask(const SxArgs& a, uint8_t* mask, uint32_t lp, uint32_t lq, const SxwSeg* segs, int nseg,
                    hipStream_t s);
hipError_t sxw_nodelta(int64_t* msg, hipStream_t s);
// the delta of a decided view (one plan window, `key`) into msg
hipError_t launch_entry_delta(const DevState& st, const DevBatch& v, const uint8_t* vstatus, EntryAcc* acc,
                              int64_t* msg, int64_t key, hipStream_t s);
}  // namespace sf
#endif
