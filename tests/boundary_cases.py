"""Workloads that put events on the internal borders of the hot path: tile and
word edges of the sort phase, the rings of the THREAD walks, the 64-ary team
search, the routing thresholds of k_classify and its fallbacks.  Random traffic
reaches these only by chance; every builder here is designed to sit on one of
them, and comes with a coverage guard that proves, from the batch and from the
ORACLE's verdicts alone, that the input does.

Shared by tests/test_boundary_cases.py (host build against the oracle, all
guards, the constant-drift check) and tests/test_gpu_boundary.py (the engine
against the oracle, plus routing guards from FlowEngine.heavy_profile()).

The constants below restate the engine's; source_constants() reads them back
from sentinel_amd/csrc as text, so a retune fails the drift test and tells
whoever retunes to move the cases.
"""
import os
import re

import numpy as np

from sentinel_amd import abi, trace

T0 = trace.T0
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sentinel_amd", "csrc")

# ---- the engine's constants, restated (test_constants_match_the_source) ----
RUN_RC = 8192               # sf_stream.h: run-mode live-exit counter ring (runs ahead)
LX_WORDS = 2048             # sf_stream.h: window-walk live-exit ring (64-event words)
SL_TILE = 4096              # sf_segs.hip: k_segs_red / k_segs_out positions per tile
RS_TILE = 4096              # sf_rsort.h RsGeom::TILE: radix pass tile
RS_CE = 16                  # sf_rsort.h: consecutive keys per thread of k_rs_count
FILL_TILE = 2048            # sf_internal.h: k_heavy_fill tile
OX_TILE = 2048              # sf_internal.h: origin pass block
SHORT_MAX = 8               # sf_internal.h: longest "short" light segment
THR_CH = 3072               # sf_stream.h: window-walk chunk
HS_CH = 2048                # sf_stream.h: RateLimiter chunk
SF_THR_RUN_AVG = 16         # sf_heavy.h: thr_run_mode, events per run
MAX_WINDOWS = 65536         # k_classify: more bucket windows than this -> SM_GENERIC
PARAM_MIN = 32              # k_classify: a ParamFlow-only segment longer than this is heavy (SM_PARAM)
HEAVY_MIN = 512             # sf_engine.cpp: default heavy_min
ACC_PER, ACC_LO_LOG2, ACC_HI_LOG2 = 64, 16, 24

RUN_FAR = RUN_RC - 1                    # first run distance that takes the HBM counter (thr_runs_segment)
LX_SPLIT = (LX_WORDS - 1) * 64          # thr_mark_exit: x - q below this stays in the LDS ring

SM_GENERIC, SM_QPS, SM_WARM, SM_RL, SM_NORULE, SM_THREAD, SM_PARAM = 1, 2, 3, 4, 5, 6, 7


def acc_cap(max_batch, heavy_min_events=0):
    """Work::acc_cap (sf_engine.cpp): window accumulator slots of one batch."""
    hm = heavy_min_events or HEAVY_MIN
    return min(max(max_batch // hm * ACC_PER, 1 << ACC_LO_LOG2), 1 << ACC_HI_LOG2)


def key_bits(R):
    kb = 1
    while (1 << kb) < R:
        kb += 1
    return kb


def source_constants():
    """The same constants, read from the source text."""
    def text(name):
        with open(os.path.join(_CSRC, name)) as f:
            return f.read()

    def one(src, pat):
        m = re.findall(pat, src)
        assert len(m) == 1, (pat, m)
        return m[0]
    stream, heavy, internal = text("sf_stream.h"), text("sf_heavy.h"), text("sf_internal.h")
    kern, rsort, eng = text("sf_segs.hip"), text("sf_rsort.h"), text("sf_engine.cpp")
    out = {}
    out["RUN_RC"] = int(one(stream, r"constexpr uint32_t RUN_RC = (\d+);"))
    out["LX_WORDS"] = int(one(stream, r"constexpr uint32_t LX_WORDS = (\d+);"))
    t, k = one(kern, r"constexpr int SL_T = (\d+), SL_K = (\d+), SL_TILE = SL_T \* SL_K;")
    out["SL_TILE"] = int(t) * int(k)
    one(rsort, r"(static constexpr int TILE = RS_W \* K \* 64;)")
    out["RS_TILE"] = int(one(rsort, r"#define SF_RS_W (\d+)")) * int(one(rsort, r"static constexpr int K = (\d+);")) * 64
    out["RS_CE"] = int(one(rsort, r"constexpr int RS_CE = (\d+);"))
    out["FILL_TILE"] = int(one(internal, r"#define SF_FILL_TILE (\d+)"))
    out["OX_TILE"] = int(one(internal, r"constexpr uint32_t OX_TILE = (\d+),"))
    out["SHORT_MAX"] = int(one(internal, r"#define SF_SHORT_MAX (\d+)"))
    one(stream, r"(constexpr uint32_t THR_CH = THR_WPC \* 64;)")
    out["THR_CH"] = int(one(stream, r"#define SF_THR_WPC (\d+)")) * 64
    one(stream, r"(constexpr int HS_CH = HS_T \* HS_PL;)")
    out["HS_CH"] = int(one(stream, r"constexpr int HS_T = (\d+);")) * int(one(stream, r"constexpr int HS_PL = (\d+);"))
    out["SF_THR_RUN_AVG"] = int(one(heavy, r"#define SF_THR_RUN_AVG (\d+)"))
    a, b = one(kern, r"if \(nh > (\d+) \|\| ns > (\d+)\) mode = SM_GENERIC;")
    assert a == b
    out["MAX_WINDOWS"] = int(a)
    out["PARAM_MIN"] = int(one(kern, r"if \(light && hi - lo > (\d+) && \(st\.rdesc\[res\]\.flags & RD_PRULE\)"))
    out["HEAVY_MIN"] = int(one(eng, r"w\.heavy_min = c\.heavy_min_events \? c\.heavy_min_events : (\d+);"))
    p, lo, hi = one(eng, r"w\.acc_cap = \(uint32_t\)std::min<size_t>\(std::max<size_t>\(N / w\.heavy_min \* (\d+), "
                         r"1 << (\d+)\), 1u << (\d+)\);")
    out["ACC"] = (int(p), int(lo), int(hi))
    # the two ring splits and the routing compares the cases are built around
    one(stream, r"(if \(x - q < \(LX_WORDS - 1\) \* 64u\))")
    one(stream, r"(if \(rc\.x - r < RUN_RC - 1\))")
    one(kern, r"(bool light = valid && !xs && hi - lo <= w\.heavy_min;)")
    one(kern, r"(const bool shrt = light && hi - lo <= SHORT_MAX;)")
    one(heavy, r"(\(uint64_t\)\(hi - lo\) >= \(uint64_t\)SF_THR_RUN_AVG \* nr;)")
    return out


MIRROR = dict(RUN_RC=RUN_RC, LX_WORDS=LX_WORDS, SL_TILE=SL_TILE, RS_TILE=RS_TILE, RS_CE=RS_CE, FILL_TILE=FILL_TILE,
              OX_TILE=OX_TILE, SHORT_MAX=SHORT_MAX, THR_CH=THR_CH, HS_CH=HS_CH, SF_THR_RUN_AVG=SF_THR_RUN_AVG,
              MAX_WINDOWS=MAX_WINDOWS, PARAM_MIN=PARAM_MIN, HEAVY_MIN=HEAVY_MIN,
              ACC=(ACC_PER, ACC_LO_LOG2, ACC_HI_LOG2))


# ---------------------------------------------------------------- helpers
def _qps(res, count, **kw):
    return abi.sf_flow_rule(resource=res, grade=abi.GRADE_QPS, count=float(count), strategy=0, control_behavior=0,
                            warm_up_period_sec=10, max_queueing_time_ms=500, **kw)


def _warm(res, count, period=10):
    return abi.sf_flow_rule(resource=res, grade=abi.GRADE_QPS, count=float(count), strategy=0,
                            control_behavior=abi.BEHAVIOR_WARM_UP, warm_up_period_sec=period, max_queueing_time_ms=500)


def _rl(res, count, queue_ms):
    # (max_queueing_time_ms is explicit: left 0 the rule is invalid and nothing queues)
    return abi.sf_flow_rule(resource=res, grade=abi.GRADE_QPS, count=float(count), strategy=0,
                            control_behavior=abi.BEHAVIOR_RATE_LIMITER, warm_up_period_sec=10,
                            max_queueing_time_ms=queue_ms)


def _warm_rl(res, count, queue_ms):
    return abi.sf_flow_rule(resource=res, grade=abi.GRADE_QPS, count=float(count), strategy=0,
                            control_behavior=abi.BEHAVIOR_WARM_UP_RATE_LIMITER, warm_up_period_sec=10,
                            max_queueing_time_ms=queue_ms)


def _thread(res, count):
    return abi.sf_flow_rule(resource=res, grade=abi.GRADE_THREAD, count=float(count), strategy=0, control_behavior=0,
                            warm_up_period_sec=10, max_queueing_time_ms=500)


def _prule(res, count):
    return abi.sf_param_rule(resource=res, grade=abi.GRADE_QPS, param_idx=0, control_behavior=0, count=float(count),
                             max_queueing_time_ms=0, burst_count=0, duration_in_sec=1, item_offset=0, item_count=0)


def merge_exits(res, ts, cnt, ent, ex_ts, args=None):
    """One time-ordered batch from entries (res, ts, cnt; ts non-decreasing)
    and the exits of the entries ``ent`` at ``ex_ts``: an exit follows the
    entries of its millisecond and carries its entry's resource, acquireCount
    and argument."""
    n = len(ts)
    all_ts = np.concatenate([ts, ex_ts])
    isx = np.concatenate([np.zeros(n, bool), np.ones(len(ent), bool)])
    order = np.lexsort((isx, all_ts))
    pos = np.empty(order.size, np.int64)
    pos[order] = np.arange(order.size)
    src = np.concatenate([np.arange(n), ent])[order]
    fl = np.where(isx[order], abi.EV_EXIT | abi.EV_IN, abi.EV_IN).astype(np.uint8)
    eref = np.full(order.size, -1, np.int64)
    eref[pos[n:]] = pos[ent]
    kw = {}
    if args is not None:
        kw = dict(arg_tag=np.full((1, order.size), abi.TAG_LONG, np.uint8),
                  arg_bits=np.asarray(args, np.uint64)[src].reshape(1, -1), n_args=np.ones(order.size, np.uint8))
    return abi.HostBatch(np.asarray(res, np.uint32)[src], all_ts[order], np.asarray(cnt, np.int32)[src], fl,
                         entry_ref=eref, **kw)


def split(full, cuts):
    return [full.subset(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


def oracle_status(so, w):
    """The oracle's verdict status of every event of the workload, batches
    concatenated (the positions of w["full"])."""
    ora = so.OracleEngine(w["cfg"])
    if w.get("flow"):
        ora.load_flow_rules(list(w["flow"]))
    if w.get("param"):
        ora.load_param_rules(list(w["param"]), list(w.get("items", ())))
    outs = [ora.submit(b) for b in w["batches"]]
    ora.close()
    return np.concatenate([o.status for o in outs]), np.concatenate([o.wait_ms for o in outs])


def passed(st):
    return np.isin(st, abi.PASSED)


def blocked(st):
    return np.isin(st, (abi.V_BLOCK_FLOW, abi.V_BLOCK_PARAM))


def is_exit(b):
    return (b.flags & abi.EV_EXIT) != 0


def run_ids(b, sel=None):
    """Run id of every event of one resource's segment (a run: consecutive
    events of one kind, entries or exits), as k_thr_rid numbers them."""
    x = is_exit(b) if sel is None else is_exit(b)[sel]
    return np.concatenate([[0], np.cumsum(x[1:] != x[:-1])])


def exit_of(b):
    """Position of each entry's exit in the batch, -1 without one."""
    xo = np.full(b.n, -1, np.int64)
    ex = np.nonzero(is_exit(b) & (b.entry_ref >= 0))[0]
    xo[b.entry_ref[ex]] = ex
    return xo


def profile_modes(eng):
    """{resource: (events, mode)} of the heavy segments of the last submit."""
    return {int(r): (int(n), int(m)) for r, n, m, _, _ in eng.heavy_profile(cap=1 << 16)}


# ---------------------------------------------------------------- 1. run mode, far runs
def far_runs(count, batches=1, seed=71, duration=6000, per_ms=20):
    """One THREAD resource; every millisecond holds its entries, then its due
    exits, so entry runs and exit runs alternate and an entry's exit lies
    2 rt + 1 runs ahead.  About 5 % of the response times are 4090..4099 ms:
    rt 4094 is the last slot of the RUN_RC counter ring, 4095 the first far
    mark (run_pre in HBM, fenced before the next table step)."""
    rng = np.random.default_rng(seed)
    n = duration * per_ms
    ts = T0 + np.repeat(np.arange(duration, dtype=np.int64), per_ms)
    acq = np.ones(n, np.int32)
    multi = rng.random(n) < 0.10
    acq[multi] = rng.integers(2, 6, int(multi.sum()))
    rt = np.floor(rng.exponential(5.0, n)).astype(np.int64)
    far = rng.random(n) < 0.05
    rt[far] = rng.integers(RUN_FAR // 2 - 5, RUN_FAR // 2 + 5, int(far.sum()))      # 4090..4099
    keep = np.nonzero(ts + rt <= T0 + duration - 1)[0]
    full = merge_exits(np.zeros(n, np.uint32), ts, acq, keep, (ts + rt)[keep])
    cuts = np.linspace(0, full.n, batches + 1).astype(int)
    return dict(cfg=abi.default_config(max_resources=1, max_batch=full.n), flow=[_thread(0, count)],
                batches=split(full, cuts) if batches > 1 else [full], full=full, cuts=cuts, nodes=[0], n_flow=1,
                count=count)


def guard_far_runs(w, st):
    full = w["full"]
    ok = passed(st) & ~is_exit(full)
    assert ok.any() and (blocked(st) & ~is_exit(full)).any(), "passes and blocks"
    for a, b in zip(w["cuts"][:-1], w["cuts"][1:]):
        part = full.subset(int(a), int(b))
        runs = run_ids(part)
        assert part.n >= SF_THR_RUN_AVG * (int(runs[-1]) + 1), "thr_run_mode"
    if len(w["batches"]) == 1:
        runs, xo = run_ids(full), exit_of(full)
        n_runs = int(runs[-1]) + 1
        assert n_runs > RUN_RC, n_runs
        has = ok & (xo >= 0)
        dist = runs[xo[has]] - runs[np.nonzero(has)[0]]
        info = dict(events=full.n, runs=n_runs, passes=int(ok.sum()), far=int((dist >= RUN_FAR).sum()),
                    last_slot=int((dist == RUN_FAR - 2).sum()), first_far=int((dist == RUN_FAR).sum()))
        if w["count"] >= 1500:
            assert info["far"] >= 100 and info["last_slot"] >= 20 and info["first_far"] >= 20, info
        else:
            assert info["far"] >= 1, info
    else:
        # Exits of the later batch whose entry passed in the earlier one: live,
        # and every one of them is counted into run_pre by k_thr_rec, whatever
        # its distance (no batch of this variant has RUN_RC runs, so the ring is
        # never left in-batch).  carried_far only records that the long
        # response times, by their time gap, are among them; it proves no
        # further path.
        k = int(w["cuts"][1])
        ex = np.nonzero(is_exit(full) & (full.entry_ref >= 0) & (np.arange(full.n) >= k))[0]
        carried = ex[(full.entry_ref[ex] < k) & ok[full.entry_ref[ex]]]
        gap = full.ts_ms[carried] - full.ts_ms[full.entry_ref[carried]]
        info = dict(carried=int(carried.size), carried_far=int((gap >= RUN_FAR // 2).sum()))
        # (no more than ``count`` threads are alive at the cut)
        lo_c, lo_f = (100, 20) if w["count"] >= 1500 else (1, 1)
        assert info["carried"] >= lo_c and info["carried_far"] >= lo_f, info
    return info


# ---------------------------------------------------------------- 2. window walk, live-exit ring border
LX_BAND = (LX_SPLIT - 128, LX_SPLIT + 192)              # 130,880 .. 131,200


def lx_ring(n=300_000, seed=72, count=645, copies=2):
    """One THREAD resource whose kinds alternate every two events (E E X X:
    the window walk, never run mode).  A band of entries, ``copies`` for every
    sorted distance of LX_BAND, has its exit that many positions ahead: on both
    sides of thr_mark_exit's split between the LDS ring and the HBM bitmap, at
    every offset of the entry inside its 64-event window.  The other exits
    take the most recent open entry.  The limit leaves the band room to pass
    and then holds the thread count at the cap until the band's exits arrive."""
    rng = np.random.default_rng(seed)
    kind = np.tile(np.array([0, 0, 1, 1], np.int8), n // 4 + 1)[:n]       # 1: exit slot
    ref = np.full(n, -1, np.int64)
    band = np.zeros(n, bool)
    taken = np.zeros(n, bool)
    p = 8000
    for d in np.repeat(np.arange(LX_BAND[0], LX_BAND[1] + 1), copies):
        while taken[p] or taken[p + d]:
            p += 1
        kind[p], kind[p + d] = 0, 1                                        # (the pattern gives way to the band)
        band[p] = taken[p] = taken[p + d] = True
        ref[p + d] = p
        p += 37                                                            # walks the offsets within a window
    assert p + LX_BAND[1] < n
    stack = []
    for i in range(n):
        if taken[i]:
            continue
        if kind[i] == 1 and stack:
            ref[i] = stack.pop()
        else:
            kind[i] = 0                                                    # no open entry: an entry instead
            stack.append(i)
    cnt = np.where(band, 1, rng.integers(1, 6, n)).astype(np.int32)
    ex = np.nonzero(kind == 1)[0]
    cnt[ex] = cnt[ref[ex]]
    ts = T0 + np.arange(n, dtype=np.int64) // 50
    fl = np.where(kind == 1, abi.EV_EXIT | abi.EV_IN, abi.EV_IN).astype(np.uint8)
    full = abi.HostBatch(np.zeros(n, np.uint32), ts, cnt, fl, entry_ref=ref)
    return dict(cfg=abi.default_config(max_resources=1, max_batch=n), flow=[_thread(0, count)], batches=[full],
                full=full, nodes=[0], n_flow=1)


def guard_lx_ring(w, st):
    full = w["full"]
    runs, xo = run_ids(full), exit_of(full)
    assert full.n < SF_THR_RUN_AVG * (int(runs[-1]) + 1), "must stay out of run mode"
    ok = passed(st) & ~is_exit(full) & (xo >= 0)
    dist = (xo - np.arange(full.n))[ok]
    inband = dist[(dist >= LX_BAND[0]) & (dist <= LX_BAND[1])]
    assert inband.size >= 400, inband.size
    missing = np.setdiff1d(np.arange(LX_BAND[0], LX_BAND[1] + 1), inband)
    assert missing.size == 0, f"no passed entry at distances {missing[:8]}"
    # x - q with q the entry's window start: both sides of the split at every window offset
    off = (np.nonzero(ok)[0] % 64)[(dist >= LX_BAND[0]) & (dist <= LX_BAND[1])]
    assert np.unique(off[inband + off < LX_SPLIT]).size >= 32 and np.unique(off[inband + off >= LX_SPLIT]).size >= 32
    nb = int((blocked(st) & ~is_exit(full)).sum())
    assert nb > 1000, nb
    return dict(events=full.n, runs=int(runs[-1]) + 1, band_passes=int(inband.size), blocks=nb)


# ---------------------------------------------------------------- 3. the 64-ary team search
POPS = (1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
SMALL_WIN = 7
WL = 500                                           # bucket window of the default geometry (1000 ms / 2)


def ladder_thresholds(pop):
    return sorted({1, 63, 64, 65, pop - 1, pop, pop + 1})


def search_ladder(kind, seed=73):
    """One resource per (window population, threshold): three half-second
    windows of ``pop`` entries with a window of 7 between them, resources
    interleaved in time, all heavy (heavy_min_events 2).  The end of a bucket
    window and the first failing entry of heavy_qps (team_first_true) then sit
    at 0, 1, at the 64 and 4096 borders of the wavefront search and at the
    window's end.  (Only the first-failure search runs over a range of ``pop``
    entries; the window-end search runs over the rest of the segment, 3 pop +
    14 events at the first window down to pop at the last, and finds its answer
    ``pop`` entries in.)  kind: "qps" (DefaultController, acquireCount 1), "warm"
    (WarmUp with count 3 k: the cold threshold is k), "multi" (acquireCount
    1-3: the tail loop after the first failure, team_next)."""
    rng = np.random.default_rng(seed)
    rules, meta, res_l, ts_l = [], [], [], []
    for pop in POPS:
        for k in ladder_thresholds(pop):
            r = len(meta)
            meta.append((pop, k))
            # (a long warm-up period keeps the threshold near count / coldFactor for the whole batch)
            rules.append(_warm(r, 3 * k, period=WARM_PERIOD) if kind == "warm" else _qps(r, k))
            for wdw in range(5):
                m = pop if wdw % 2 == 0 else SMALL_WIN
                ts_l.append(T0 + WL * wdw + (np.arange(m, dtype=np.int64) * WL) // m)
                res_l.append(np.full(m, r, np.uint32))
    ts, res = np.concatenate(ts_l), np.concatenate(res_l)
    order = np.argsort(ts, kind="stable")
    ts, res = ts[order], res[order]
    cnt = np.ones(ts.size, np.int32) if kind != "multi" else rng.integers(1, 4, ts.size).astype(np.int32)
    full = abi.HostBatch(res, ts, cnt, np.full(ts.size, abi.EV_IN, np.uint8))
    R = len(meta)
    return dict(cfg=abi.default_config(max_resources=R, max_batch=full.n, heavy_min_events=2), flow=rules,
                batches=[full], full=full, nodes=list(range(R)), n_flow=len(rules), meta=meta, kind=kind,
                modes={r: SM_WARM if kind == "warm" else SM_QPS for r in range(R)})


def first_blocks(full, st, r):
    """Index of the first blocked entry in each of the five windows of
    resource r (None: none), and the window's population."""
    sel = np.nonzero(full.res_id == r)[0]
    wdw = (full.ts_ms[sel] - T0) // WL
    out = []
    for k in range(5):
        s = st[sel[wdw == k]]
        b = np.nonzero(blocked(s))[0]
        out.append((int(b[0]) if b.size else None, int(s.size)))
    return out


WARM_PERIOD, COLD_FACTOR = 1000, 3                # the WarmUp ladder's rules (cold_factor: the config default)


def warm_first_blocks(ts, count):
    """WarmUpController replayed on one resource's entries (acquireCount 1) at
    times ``ts`` from T0: the designed index of the first blocked entry in each
    of the five windows (None: none).  The reference's arithmetic step by
    step (WarmUpController.java:113-139 construct, :147-175 canPass, :178-232
    syncToken / coolDownTokens), in the same doubles."""
    import math
    warning = int(WARM_PERIOD * count) // (COLD_FACTOR - 1)
    max_token = warning + int(2 * WARM_PERIOD * count / (1.0 + COLD_FACTOR))
    stored, last_filled = 0, 0
    win_pass = [0] * 5                              # passes per half-second window
    first = [None] * 5
    seen_in = [0] * 5
    for t in ts:
        q = int(t - T0) // WL
        pass_qps = win_pass[q] + (win_pass[q - 1] if q else 0)            # the two buckets of the interval
        sec = q // 2
        prev_qps = sum(win_pass[2 * (sec - 1):2 * sec]) if sec else 0    # the minute bucket of the second before
        cur = int(t) - int(t) % 1000
        if cur > last_filled:                                            # syncToken, once per second
            new = stored
            if stored < warning or (stored > warning and prev_qps < int(count) // COLD_FACTOR):
                new = int(stored + (cur - last_filled) * count / 1000)
            stored = max(min(new, max_token) - prev_qps, 0)
            last_filled = cur
        if stored >= warning:
            # (count 0: slope is inf, the threshold 0 * inf = NaN, and nothing passes)
            if count > 0:
                slope = (COLD_FACTOR - 1.0) / count / (max_token - warning)
                ok = float(pass_qps + 1) <= math.nextafter(1.0 / (float(stored - warning) * slope + 1.0 / count),
                                                           math.inf)
            else:
                ok = False
        else:
            ok = float(pass_qps + 1) <= count
        if ok:
            win_pass[q] += 1
        elif first[q] is None:
            first[q] = seen_in[q]
        seen_in[q] += 1
    return first


def guard_search_ladder(w, st):
    """The oracle's first blocked entry of every window is at the designed
    index: for QPS rules the replay of the rolling two-bucket budget, for
    WarmUp rules the replay of the controller (warm_first_blocks); in the first
    window both have the closed form k (none when k >= pop).  ``seen`` holds
    the OBSERVED (population, index) pairs of the full windows, and every rung
    of the ladder must be among them.  Later WarmUp windows mostly repeat the
    first window's index; the rungs near k = pop drift by a few entries as the
    stored tokens cool, which the replay follows exactly."""
    full, kind = w["full"], w["kind"]
    assert passed(st).any() and blocked(st).any()
    seen = set()
    tail = 0
    for r, (pop, k) in enumerate(w["meta"]):
        fb = first_blocks(full, st, r)
        assert [n for _, n in fb] == [pop, SMALL_WIN, pop, SMALL_WIN, pop]
        sel = np.nonzero(full.res_id == r)[0]
        wdw = (full.ts_ms[sel] - T0) // WL
        if kind == "warm":
            want = warm_first_blocks(full.ts_ms[sel], w["flow"][r].count)
            assert [f for f, _ in fb] == want, (r, pop, k, fb, want)
        else:
            # rolling QPS over the two half-second buckets: a window's budget is
            # the count less what the previous window passed; an entry passes
            # while the acquireCounts passed so far plus its own fit
            prev = 0
            for q in range(5):
                room, used, want = k - prev, 0, None
                for i, c in enumerate(full.count[sel[wdw == q]]):
                    if used + int(c) <= room:
                        used += int(c)
                        tail += want is not None and q % 2 == 0
                    elif want is None:
                        want = i
                assert fb[q][0] == want, (r, pop, k, q, fb, want)
                prev = used
        if kind != "multi":
            assert fb[0][0] == (k if k < pop else None), (r, pop, k, fb)
        for q in (0, 2, 4):
            seen.add((pop, fb[q][0]))
    if kind != "multi":
        for pop in POPS:                          # the first failure at 0 / 1, the 64-borders and the window's end
            for k in ladder_thresholds(pop):
                assert (pop, k if k < pop else None) in seen, (pop, k)
    else:
        assert tail >= 20, tail                   # passes after a window's first failure (team_next's tail)
    return dict(events=full.n, resources=len(w["meta"]), passes=int(passed(st).sum()), blocks=int(blocked(st).sum()),
                tail_passes=int(tail))


RL_LENGTHS = (HS_CH - 1, HS_CH, HS_CH + 1, 2 * HS_CH, 2 * HS_CH + 1)


def rl_chunks(seed=74):
    """RateLimiter segments whose ends sit on the HS_CH chunk edges of
    rl_decide_chunk; maxQueueingTimeMs is set, so entries queue."""
    rng = np.random.default_rng(seed)
    rules, res_l, ts_l = [], [], []
    for r, m in enumerate(RL_LENGTHS):
        rules.append(_rl(r, 400 + 50 * r, 8 + r))
        ts_l.append(T0 + np.sort(rng.integers(0, 4000, m)).astype(np.int64))
        res_l.append(np.full(m, r, np.uint32))
    ts, res = np.concatenate(ts_l), np.concatenate(res_l)
    order = np.argsort(ts, kind="stable")
    cnt = np.where(rng.random(ts.size) < 0.9, 1, rng.integers(2, 4, ts.size)).astype(np.int32)
    full = abi.HostBatch(res[order], ts[order], cnt, np.full(ts.size, abi.EV_IN, np.uint8))
    R = len(RL_LENGTHS)
    return dict(cfg=abi.default_config(max_resources=R, max_batch=full.n, heavy_min_events=2), flow=rules,
                batches=[full], full=full, nodes=list(range(R)), n_flow=R, modes={r: SM_RL for r in range(R)})


def guard_rl_chunks(w, st, wait):
    full = w["full"]
    for r, m in enumerate(RL_LENGTHS):
        sel = full.res_id == r
        assert int(sel.sum()) == m
        assert (wait[sel] > 0).any() and blocked(st[sel]).any() and passed(st[sel]).any(), r
    return dict(events=full.n, waits=int((wait > 0).sum()))


# ---------------------------------------------------------------- 4. batch sizes and key widths
BATCH_SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
KEY_RESOURCES = (1, 2, 256, 257, 65536, 65537)     # key_bits 1, 1, 8, 9, 16, 17: one, two, three sort passes


def sort_digits(R):
    """(passes, digit bits) of rs_sort for R resources."""
    kb = key_bits(R)
    P = (kb + 7) // 8
    return P, (kb + P - 1) // P


def batch_sizes(R, seed=75):
    """One engine fed consecutive time-ordered batches of BATCH_SIZES events
    (the 16-position vector tails, the 4096 tiles and the unrolled 2048 stride
    of the sort phase, one under, on and one over).  Resource ids include 0,
    R - 1 and pairs that differ only in the top digit of the sort key; tight
    QPS and THREAD rules make the verdicts depend on the stable order."""
    rng = np.random.default_rng(seed + R)
    P, D = sort_digits(R)
    top = 1 << ((P - 1) * D)
    ids = sorted({x for x in (0, 1, R - 1, R - 2, top, top + 1, 2 * top + 1, R // 2) if 0 <= x < R})
    thr = [x for i, x in enumerate(ids) if i % 2 == 1 or R == 1]          # THREAD with exits; the rest QPS
    qps = [x for x in ids if x not in thr]
    rules = [(_thread(x, 1) if x in thr else _qps(x, 1 + i % 3)) for i, x in enumerate(ids)]
    total = sum(BATCH_SIZES)
    # Entries come as pairs on one resource in one millisecond, THREAD and QPS
    # resources in turn: a THREAD pair is a pass and a block, its exits follow
    # in the same millisecond (some one or two later, holding the thread), so
    # any 16 consecutive events hold a pass and a block of one resource and
    # most cuts separate an exit from its entry.
    pairs = total // 2 + 1
    pick_t = np.asarray(thr, np.uint32)[rng.integers(0, len(thr), pairs)]
    pick_q = np.asarray(qps or thr, np.uint32)[rng.integers(0, len(qps or thr), pairs)]
    res = np.repeat(np.where(np.arange(pairs) % 2 == 0, pick_t, pick_q), 2)
    n = res.size
    ts = T0 + np.arange(n, dtype=np.int64) // 2
    ent = np.nonzero(np.isin(res, thr))[0]
    rt = np.where((ent % 2 == 0) & (rng.random(ent.size) < 0.15), rng.integers(1, 3, ent.size), 0)
    full = merge_exits(res, ts, np.ones(n, np.int32), ent, ts[ent] + rt)
    full = full.subset(0, total)
    cuts = np.concatenate([[0], np.cumsum(BATCH_SIZES)])
    # An exit whose entry was blocked in an earlier batch carries entry_ref -2,
    # as a caller would send it (-1 would make it live and the rule slack).
    # Which THREAD entries block is replayed here; the guard checks the outcome
    # against the oracle.
    limit = {int(r.resource): r.count for r in rules if r.grade == abi.GRADE_THREAD}
    alive = dict.fromkeys(limit, 0)
    ok = np.zeros(full.n, bool)
    for i in range(full.n):
        r = int(full.res_id[i])
        if r not in limit:
            continue
        if full.flags[i] & abi.EV_EXIT:
            alive[r] -= bool(ok[full.entry_ref[i]])
        elif alive[r] + 1 <= limit[r]:
            ok[i] = True
            alive[r] += 1
    batches = split(full, cuts)
    for b, a in zip(batches, cuts[:-1]):
        ref = full.entry_ref[int(a):int(a) + b.n]
        b.entry_ref[(ref >= 0) & (ref < a) & ~ok[np.clip(ref, 0, None)]] = -2
    return dict(cfg=abi.default_config(max_resources=R, max_batch=max(BATCH_SIZES)), flow=rules,
                batches=batches, full=full, cuts=cuts, nodes=ids, n_flow=len(rules), ids=ids, thread_ok=ok)


def guard_batch_sizes(w, st):
    full = w["full"]
    assert tuple(b.n for b in w["batches"]) == BATCH_SIZES
    ent = ~is_exit(full)
    for a, b in zip(w["cuts"][:-1], w["cuts"][1:]):
        if b - a < 16:
            continue
        sl = slice(int(a), int(b))
        key = (full.res_id[sl].astype(np.int64) << 32) | ((full.ts_ms[sl] - T0) // WL)
        kp = np.unique(key[passed(st[sl]) & ent[sl]])
        kb = np.unique(key[blocked(st[sl]) & ent[sl]])
        assert np.intersect1d(kp, kb).size > 0, f"batch [{a}, {b}): no resource with a pass and a block in one window"
    thr = np.isin(full.res_id, [int(r.resource) for r in w["flow"] if r.grade == abi.GRADE_THREAD]) & ent
    assert np.array_equal(passed(st)[thr], w["thread_ok"][thr]), "the builder's THREAD replay"
    ids = w["ids"]
    R = w["cfg"].max_resources
    assert 0 in ids and R - 1 in ids
    P, D = sort_digits(R)
    if R > 2:
        low = (1 << ((P - 1) * D)) - 1
        assert any(x != y and (x & low) == (y & low) for x in ids for y in ids), "a pair differing in the top digit only"
    return dict(events=full.n, passes=int(passed(st).sum()), blocks=int(blocked(st).sum()))


# ---------------------------------------------------------------- 5. segment placement
BORDERS = (64, 2048, 4096, 8192)
FIRST_LENGTHS = (0, 1, 63, 64, 2047, 4095)
HEAVY_KINDS = ("qps", "warm", "rl", "norule", "thread", "generic", "param")
KIND_MODE = dict(qps=SM_QPS, warm=SM_WARM, rl=SM_RL, norule=SM_NORULE, thread=SM_THREAD, generic=SM_GENERIC,
                 param=SM_PARAM)
PLACE_POINTS = 36                                  # cluster points 2048 j, j = 1..36


def placement_lengths(s, rot=0):
    """[(length, kind)] of the segments in resource order: a first resource of
    s events, then a ladder that puts, at every multiple 2048 j of the tile
    sizes and one position under and over it, in turn the end of a heavy
    segment and the start of a light one, the end of a light segment and the
    start of a heavy one, and the inside of a heavy segment.  (Tiles are
    aligned to multiples of their size, so a position counts for border B by
    its residue mod B.)  Heavy segments take the kinds of HEAVY_KINDS in turn,
    starting at ``rot``; the gaps are filled with light segments of every
    length class."""
    segs = [(s, "first")] if s else []
    pos = s
    fill_cycle = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 300, 511, 512]
    state = dict(fill=0, heavy=rot)

    def light(n):
        nonlocal pos
        segs.append((n, "light"))
        pos += n

    def heavy(n):
        nonlocal pos
        segs.append((n, HEAVY_KINDS[state["heavy"] % len(HEAVY_KINDS)]))
        state["heavy"] += 1
        pos += n

    def fill_to(target):
        while pos < target:
            n = min(fill_cycle[state["fill"] % len(fill_cycle)], target - pos)
            state["fill"] += 1
            light(n)

    for j in range(1, PLACE_POINTS + 1):
        q = 2048 * j + (j // 3) % 3 - 1
        hl = HEAVY_MIN + 1 + 13 * (j % 7)
        t = j % 3
        if t == 0:                                # heavy ends at q, light starts at q
            fill_to(q - hl)
            heavy(hl)
            light(1 + j % SHORT_MAX)
        elif t == 1:                              # light ends at q, heavy starts at q
            fill_to(q - 9)
            light(9)
            heavy(hl)
        else:                                     # heavy straddles the multiple
            fill_to(q - hl // 2)
            heavy(hl)
    return segs


def placement(s, origins=False, rot=0, seed=76):
    rng = np.random.default_rng(seed + s)
    segs = placement_lengths(s, rot)
    lens = np.array([n for n, _ in segs], np.int64)
    n = int(lens.sum())
    R = len(segs)
    # events of all resources shuffled over the batch's time; within a THREAD resource E E X ... pairs
    label = rng.permutation(np.repeat(np.arange(R, dtype=np.int64), lens))
    ts = T0 + np.arange(n, dtype=np.int64) // 16
    flags = np.full(n, abi.EV_IN, np.uint8)
    eref = np.full(n, -1, np.int64)
    cnt = np.where(rng.random(n) < 0.85, 1, rng.integers(2, 4, n)).astype(np.int32)
    flow, param = [], []
    light_kinds = ("qps", "none", "thread", "warm", "rl", "qps2")
    kinds = []
    for r, (_, kind) in enumerate(segs):
        if kind in ("light", "first"):
            kind = light_kinds[r % len(light_kinds)]
        kinds.append(kind)
        c = 1 + r % 5
        if kind == "qps":
            flow.append(_qps(r, c))
        elif kind == "warm":
            flow.append(_warm(r, 3 * c))
        elif kind == "rl":
            flow.append(_rl(r, 20 * c, 30))
        elif kind in ("generic", "qps2"):
            flow += [_qps(r, 2 * c), _qps(r, c)]
        elif kind == "thread":
            flow.append(_thread(r, c))
            sel = np.nonzero(label == r)[0]
            open_ = []
            for i in sel:                         # exits of earlier entries, about every other event
                if open_ and rng.random() < 0.5:
                    e = open_.pop(0)
                    flags[i] |= abi.EV_EXIT
                    eref[i] = e
                    cnt[i] = cnt[e]
                else:
                    open_.append(i)
        elif kind == "param":
            param.append(_prule(r, c))
    args = rng.integers(0, 6, n).astype(np.uint64)
    ex = np.nonzero(eref >= 0)[0]
    args[ex] = args[eref[ex]]
    full = abi.HostBatch(label.astype(np.uint32), ts, cnt, flags, entry_ref=eref,
                         arg_tag=np.full((1, n), abi.TAG_LONG, np.uint8), arg_bits=args.reshape(1, -1),
                         n_args=np.ones(n, np.uint8))
    w = dict(cfg=abi.default_config(max_resources=R, max_batch=n, param_capacity=1 << 14), flow=flow, param=param,
             batches=[full], full=full, nodes=list(range(R)), n_flow=len(flow), segs=segs, kinds=kinds,
             modes={r: KIND_MODE[k] for r, (_, k) in enumerate(segs) if k in KIND_MODE})
    if origins:
        full = trace.with_origins(full, n_origins=4, seed=seed)
        pairs = np.unique(full.res_id.astype(np.uint64) << np.uint64(32) | full.origin.astype(np.uint64))
        on = [(int(p >> np.uint64(32)), int(p & np.uint64(0xffffffff))) for p in pairs]
        w.update(batches=[full], full=full, origin_nodes=on[::5])
        w["cfg"].aux_capacity = max(4096, 2 * len(on))
    return w


def guard_placement(segs):
    """Every residue (-1, 0, +1) of every border is hit by a start and by an
    end, of a light and of a heavy segment; returns the (kind, border) pairs
    of heavy segments with a border strictly inside."""
    start = np.concatenate([[0], np.cumsum([n for n, _ in segs])])
    hit = set()
    straddle = set()
    for (n, kind), a, e in zip(segs, start[:-1], start[1:]):
        cls = "light" if n <= HEAVY_MIN else "heavy"
        if kind == "first":                       # (not part of the ladder: any length)
            continue
        assert (cls == "heavy") == (kind in HEAVY_KINDS)
        for B in BORDERS:
            for d in (-1, 0, 1):
                if a > 1 and (a - d) % B == 0:
                    hit.add((cls, "start", B, d))
                if (e - d) % B == 0:
                    hit.add((cls, "end", B, d))
            if cls == "heavy" and (a // B) != ((e - 1) // B) and a % B and e % B:
                straddle.add((kind, B))
    want = {(c, w_, B, d) for c in ("light", "heavy") for w_ in ("start", "end") for B in BORDERS for d in (-1, 0, 1)}
    assert want <= hit, sorted(want - hit)
    return straddle


# ---------------------------------------------------------------- 6. routing borders
ROUTE_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 511, 512, 513, 514)
ROUTE_KINDS = ("none", "qps", "qps2", "warm", "rl", "warm_rl", "thread", "param")
ROUTE_MODE = dict(none=SM_NORULE, qps=SM_QPS, qps2=SM_GENERIC, warm=SM_WARM, rl=SM_RL, warm_rl=SM_GENERIC,
                  thread=SM_THREAD, param=SM_PARAM)


def routing(seed=77, duration=3000):
    """Every segment length on a routing border of k_classify (SHORT_MAX, the
    light length classes, the default heavy_min, the 32-event SM_PARAM rule)
    for each of eight rule kinds, default heavy_min_events."""
    rng = np.random.default_rng(seed)
    flow, param, res_l, meta = [], [], [], []
    for kind in ROUTE_KINDS:
        for m in ROUTE_LENGTHS:
            r = len(meta)
            meta.append((kind, m))
            res_l.append(np.full(m, r, np.int64))
            c = 1 + r % 4
            if kind == "qps":
                flow.append(_qps(r, c))
            elif kind == "qps2":
                flow += [_qps(r, 2 * c), _qps(r, c)]
            elif kind == "warm":
                flow.append(_warm(r, 3 * c))
            elif kind == "rl":
                flow.append(_rl(r, 25 * c, 30))
            elif kind == "warm_rl":
                flow.append(_warm_rl(r, 25 * c, 30))
            elif kind == "thread":
                flow.append(_thread(r, c))
            elif kind == "param":
                param.append(_prule(r, c))
    label = rng.permutation(np.concatenate(res_l))
    n = label.size
    ts = T0 + (np.arange(n, dtype=np.int64) * duration) // n
    flags = np.full(n, abi.EV_IN, np.uint8)
    eref = np.full(n, -1, np.int64)
    cnt = np.ones(n, np.int32)
    for r, (kind, m) in enumerate(meta):
        if kind != "thread":
            continue
        open_ = []
        for i in np.nonzero(label == r)[0]:
            # (a one-event segment stays an entry; longer ones hold exits)
            if open_ and rng.random() < 0.5:
                flags[i] |= abi.EV_EXIT
                eref[i] = open_.pop(0)
            else:
                open_.append(i)
    args = rng.integers(0, 4, n).astype(np.uint64)
    full = abi.HostBatch(label.astype(np.uint32), ts, cnt, flags, entry_ref=eref,
                         arg_tag=np.full((1, n), abi.TAG_LONG, np.uint8), arg_bits=args.reshape(1, -1),
                         n_args=np.ones(n, np.uint8))
    R = len(meta)
    heavy = {r: ROUTE_MODE[kind] for r, (kind, m) in enumerate(meta)
             if m > HEAVY_MIN or (kind == "param" and m > PARAM_MIN)}
    return dict(cfg=abi.default_config(max_resources=R, max_batch=n, param_capacity=1 << 14), flow=flow, param=param,
                batches=[full], full=full, nodes=list(range(R)), n_flow=len(flow), meta=meta, modes=heavy)


def guard_routing(w, st):
    full = w["full"]
    lens = np.bincount(full.res_id, minlength=len(w["meta"]))
    assert [int(x) for x in lens] == [m for _, m in w["meta"]]
    for B in (1, 2, SHORT_MAX, 16, 32, 64, 128, 256, HEAVY_MIN):           # each border: on it and one over
        assert B in ROUTE_LENGTHS and B + 1 in ROUTE_LENGTHS, B
    assert PARAM_MIN in ROUTE_LENGTHS and PARAM_MIN + 1 in ROUTE_LENGTHS
    for kind in ROUTE_KINDS:
        if kind == "none":
            continue
        sel = np.isin(full.res_id, [r for r, (k, _) in enumerate(w["meta"]) if k == kind])
        assert passed(st[sel]).any() and blocked(st[sel]).any(), kind
    return dict(events=full.n, heavy=len(w["modes"]))


# ---------------------------------------------------------------- 7. classify fallbacks
def acc_overflow(seed=78, R=48, bursts=24, span_ms=1_000_000):
    """48 heavy segments (heavy_min_events 8) of 72 events each in bursts of 3
    per millisecond over 1000 s: together they ask for about 96 k half-second
    windows against acc_cap 65,536, so k_classify sends some of them (which
    ones depends on the order of its atomics) to SM_GENERIC.  The verdicts
    must not depend on that."""
    rng = np.random.default_rng(seed)
    flow, ts_l, res_l = [], [], []
    kinds = ("none", "qps", "warm", "rl")
    for r in range(R):
        kind = kinds[r % 4]
        if kind == "qps":
            flow.append(_qps(r, 2))
        elif kind == "warm":
            flow.append(_warm(r, 6))
        elif kind == "rl":
            flow.append(_rl(r, 1000, 1))
        t = np.sort(rng.integers(0, span_ms, bursts - 2))
        t = np.concatenate([[r], t, [span_ms - 1 - r]])                    # every segment spans the whole time
        ts_l.append(T0 + np.repeat(t, 3).astype(np.int64))
        res_l.append(np.full(3 * bursts, r, np.uint32))
    ts, res = np.concatenate(ts_l), np.concatenate(res_l)
    order = np.argsort(ts, kind="stable")
    full = abi.HostBatch(res[order], ts[order], np.ones(ts.size, np.int32), np.full(ts.size, abi.EV_IN, np.uint8))
    return dict(cfg=abi.default_config(max_resources=R, max_batch=full.n, heavy_min_events=8), flow=flow,
                batches=[full], full=full, nodes=list(range(R)), n_flow=len(flow))


def many_windows(seed=79, n=1200, span_ms=36_000_000):
    """One heavy QPS segment spanning more than 65,536 bucket windows (10 h)."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, span_ms, n // 2))
    t[0], t[-1] = 0, span_ms - 1
    ts = T0 + np.repeat(t, 2).astype(np.int64)
    full = abi.HostBatch(np.zeros(n, np.uint32), ts, np.ones(n, np.int32), np.full(n, abi.EV_IN, np.uint8))
    return dict(cfg=abi.default_config(max_resources=1, max_batch=n), flow=[_qps(0, 1)], batches=[full], full=full,
                nodes=[0], n_flow=1)


def requested_windows(w):
    """Half-second windows the heavy segments of the batch ask k_classify for."""
    full, hm = w["full"], w["cfg"].heavy_min_events or HEAVY_MIN
    total, widest = 0, 0
    for r in np.unique(full.res_id):
        t = full.ts_ms[full.res_id == r]
        if t.size > hm:
            nh = int(t[-1] // WL - t[0] // WL + 1)
            total += nh
            widest = max(widest, nh)
    return total, widest


def guard_fallback(w, st, which):
    total, widest = requested_windows(w)
    cap = acc_cap(w["cfg"].max_batch, w["cfg"].heavy_min_events)
    assert passed(st).any() and blocked(st).any()
    if which == "acc":
        assert cap == 1 << ACC_LO_LOG2 and total > cap and widest <= MAX_WINDOWS, (total, widest, cap)
    else:
        assert widest > MAX_WINDOWS, widest
    return dict(events=w["full"].n, windows=total, widest=widest, acc_cap=cap, passes=int(passed(st).sum()),
                blocks=int(blocked(st).sum()))


# ---------------------------------------------------------------- 8. rules of count 0
def zero_counts(heavy):
    """One resource per controller, every rule with count 0 (a valid rule:
    FlowRuleUtil.isValidRule asks for count >= 0): nothing may pass.  A WarmUp
    rule of count 0 has slope inf and a threshold 0 * inf = NaN, which Java's
    passQps + acquireCount <= warningQps never satisfies; heavy_qps once asked
    "> threshold" instead and passed everything.  heavy: on the window
    algorithms (heavy_min_events 2), else on the light lane walks."""
    m = 40
    flow = [_warm(0, 0), _qps(1, 0), _rl(2, 0, 20), _thread(3, 0)]
    res = np.tile(np.arange(4, dtype=np.uint32), m)
    ts = T0 + np.arange(4 * m, dtype=np.int64) * 30            # 4.8 s: the per-second WarmUp sync runs again
    ent = np.nonzero(res == 3)[0]
    full = merge_exits(res, ts, np.ones(4 * m, np.int32), ent, ts[ent] + 5)
    modes = {0: SM_WARM, 1: SM_QPS, 2: SM_RL, 3: SM_THREAD} if heavy else {}
    return dict(cfg=abi.default_config(max_resources=4, max_batch=full.n, heavy_min_events=2 if heavy else 0),
                flow=flow, batches=[full], full=full, nodes=[0, 1, 2, 3], n_flow=4, modes=modes)


def guard_zero_counts(w, st):
    full = w["full"]
    ent = ~is_exit(full)
    assert blocked(st[ent]).all() and (st[~ent] == abi.V_EXIT_IGNORED).all()
    return dict(events=full.n, blocks=int(ent.sum()))


# ---------------------------------------------------------------- the cases
# name -> (builder, guard(w, status, wait) -> figures); the guard sees the
# batch and the oracle's verdicts only
def _placement_guard(w, st):
    straddle = guard_placement(w["segs"])
    for kind in ("qps", "warm", "rl", "thread", "generic", "param"):
        sel = np.isin(w["full"].res_id, [r for r, k in enumerate(w["kinds"]) if k == kind])
        assert passed(st[sel]).any() and blocked(st[sel]).any(), kind
    return dict(events=w["full"].n, segments=len(w["segs"]), straddle=len(straddle))


CASES = {}
for _c in (30, 1500):
    CASES[f"far_runs_{_c}"] = (lambda c=_c: far_runs(c), lambda w, st, wait: guard_far_runs(w, st))
    CASES[f"far_runs_{_c}_two_batches"] = (lambda c=_c: far_runs(c, batches=2), lambda w, st, wait: guard_far_runs(w, st))
CASES["lx_ring"] = (lx_ring, lambda w, st, wait: guard_lx_ring(w, st))
for _k in ("qps", "warm", "multi"):
    CASES[f"search_{_k}"] = (lambda k=_k: search_ladder(k), lambda w, st, wait: guard_search_ladder(w, st))
CASES["rl_chunks"] = (rl_chunks, guard_rl_chunks)
for _r in KEY_RESOURCES:
    CASES[f"batch_sizes_R{_r}"] = (lambda r=_r: batch_sizes(r), lambda w, st, wait: guard_batch_sizes(w, st))
for _i, _s in enumerate(FIRST_LENGTHS):
    CASES[f"placement_s{_s}"] = (lambda s=_s, i=_i: placement(s, rot=i), lambda w, st, wait: _placement_guard(w, st))
    CASES[f"placement_s{_s}_origins"] = (lambda s=_s, i=_i: placement(s, origins=True, rot=i + 3),
                                           lambda w, st, wait: _placement_guard(w, st))
CASES["routing"] = (routing, lambda w, st, wait: guard_routing(w, st))
CASES["zero_counts_heavy"] = (lambda: zero_counts(True), lambda w, st, wait: guard_zero_counts(w, st))
CASES["zero_counts_light"] = (lambda: zero_counts(False), lambda w, st, wait: guard_zero_counts(w, st))
CASES["acc_overflow"] = (acc_overflow, lambda w, st, wait: guard_fallback(w, st, "acc"))
CASES["many_windows"] = (many_windows, lambda w, st, wait: guard_fallback(w, st, "windows"))


def placement_straddles():
    """(kind, border) pairs with a border inside a heavy segment, over all
    placement cases: every heavy kind straddles every border."""
    got = set()
    for i, s in enumerate(FIRST_LENGTHS):
        got |= guard_placement(placement_lengths(s, i)) | guard_placement(placement_lengths(s, i + 3))
    return got
