"""Workloads that put DegradeSlot events on the internal borders of the breaker
kernels (sentinel_amd/csrc/sf_degrade.hip): the 64|65 switch between the lane
walk (k_dg_walk) and the wave walk (k_dg_wave), the lanes and chunk edges of
the wave walk's bulk prefix, its window-roll runs, its four ways of finding an
exit's entry, the hand-off of breaker state between HBM and registers at a
batch cut, the grid stride and the radix key widths.  Seeded random traffic
reaches any of these only by chance; every builder here is scripted to sit on
one, and comes with a guard that proves it on the CPU from the batch, a model
of the kernels' event placement (paths()) and the transition log of
oracle/degrade.py.

Shared by tests/test_degrade_cases.py (guards, the two oracles against each
other, hand-derived expectations, the registry meta-check) and
tests/test_gpu_degrade_cases.py (the engine against the oracle).

CASES[name] = (build, guard).  build() returns a dict: rules, batches, R, and
per family extras (marks: designed positions, expect: literal verdicts,
twins).  guard(case, an) takes the analysis of analyze(case) and returns the
set of properties it proved (PROPS lists the ones the registry must cover).

Position classes of a transition on the wave walk: the first state-changing
event of a chunk ("stop": a transition, or a probe that a later breaker sent
back) is found by the lane-parallel bulk prefix when it sits at lane >= 1
("bulk"); a stop at lane 0, and every transition after the first stop of its
chunk, is decided by the serial walk ("serial").
"""
import math
import os
import re

import numpy as np

from oracle import degrade as od
from sentinel_amd import abi

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the engine's constants, restated (test_constants_match_the_source)
HEAVY = 64                  # sf_degrade.hip: segments longer than this take the wave walk
MAXC = 4                    # sf_degrade.hip: breakers per resource the wave walk holds
GRID = 2048                 # dg_launch: most waves k_dg_wave is launched with
MAX_BREAKERS = 64           # sentinel_flow.h: SF_MAX_BREAKERS_PER_RESOURCE
MIRROR = dict(HEAVY=HEAVY, MAXC=MAXC, GRID=GRID, MAX_BREAKERS=MAX_BREAKERS)

RT, RATIO, COUNT = abi.DEGRADE_GRADE_RT, abi.DEGRADE_GRADE_EXCEPTION_RATIO, abi.DEGRADE_GRADE_EXCEPTION_COUNT
T0 = 1_000_000              # first timestamp of every case (>= 0)
KIND = {(od.CLOSED, od.OPEN): "trip", (od.OPEN, od.HALF_OPEN): "probe", (od.HALF_OPEN, od.CLOSED): "close",
        (od.HALF_OPEN, od.OPEN): "reopen", (od.OPEN, od.OPEN): "fallback"}
KINDS = ("trip", "probe", "close", "reopen")
ROUTES = ("same", "prev", "old", "cts")
PROPS = ({"walk:wave", "walk:lane"} | {f"route:{r}" for r in ROUTES} | {f"bulk:{k}" for k in KINDS}
         | {f"serial:{k}" for k in KINDS})


def source_constants():
    """The same constants, read from the source text."""
    def one(path, pat):
        with open(os.path.join(_ROOT, path)) as f:
            m = re.findall(pat, f.read())
        assert len(m) == 1, (pat, m)
        return m[0]
    hip = "sentinel_amd/csrc/sf_degrade.hip"
    out = dict(HEAVY=int(one(hip, r"constexpr uint32_t HEAVY = (\d+);")),
               MAXC=int(one(hip, r"constexpr uint32_t MAXC = (\d+);")),
               GRID=int(one(hip, r"const uint32_t waves = min\(d\.n_rres, (\d+)u\);")),
               MAX_BREAKERS=int(one("include/sentinel_flow.h", r"#define SF_MAX_BREAKERS_PER_RESOURCE (\d+)")))
    # the compares the cases are built around
    one(hip, r"(if \(j1 - j0 > HEAVY && c1 - c0 <= MAXC\))")
    one(hip, r"(if \(j0 \+ 64 < j1\) load_rec\(j0 \+ 64,)")
    one(hip, r"(if \(j \+ 128 < j1\) load_rec\(j \+ 128,)")
    one(hip, r"(for \(uint32_t h = blockIdx\.x; h < nh; h \+= gridDim\.x\))")
    return out


# ---------------------------------------------------------------- scripting
def rule(res, grade, count, tw=1, min_req=1, ratio=1.0, interval=1000):
    return abi.degrade_rule(res, grade, count, tw, min_request_amount=min_req, slow_ratio_threshold=ratio,
                            stat_interval_ms=interval)


class Script:
    """Events of many resources, added per resource in time order; assemble()
    merges them by (time, exits after entries, insertion order), which keeps
    each resource's order as long as an entry never follows an exit of its own
    resource within one millisecond (Res steps time to see to that)."""

    def __init__(self):
        self.t, self.x, self.res, self.fl, self.ref, self.cr = [], [], [], [], [], []

    def add(self, res, t, flags, ref=-1, create=0):
        assert t >= 0
        self.t.append(t); self.x.append(1 if flags & abi.EV_EXIT else 0); self.res.append(res)
        self.fl.append(flags); self.ref.append(ref); self.cr.append(create)
        return len(self.t) - 1

    def assemble(self, cuts=(), extra_flags=0):
        """The full batch and the edges of its split at the times ``cuts`` (a
        batch starts at the first event with t >= cut); finish() makes the
        batches.  ``self.pos`` maps add()'s handles to positions in it."""
        t, x = np.array(self.t, np.int64), np.array(self.x, np.int64)
        order = np.lexsort((np.arange(t.size), x, t))
        pos = np.empty(t.size, np.int64)
        pos[order] = np.arange(t.size)
        ref = np.array(self.ref, np.int64)
        cr = np.array(self.cr, np.int64)
        has = ref >= 0
        cr[has] = t[ref[has]]
        ref[has] = pos[ref[has]]
        fl = np.array(self.fl, np.uint8) | np.uint8(extra_flags)
        full = abi.HostBatch(np.array(self.res, np.uint32)[order], t[order], np.ones(t.size, np.int32), fl[order],
                             entry_ref=ref[order], create_ts=cr[order])
        self.pos = pos
        edges = [0] + [int(np.searchsorted(full.ts_ms, c, "left")) for c in cuts] + [full.n]
        return full, edges


def finish(rules, full, edges, R, refs=True, **extra):
    """The case: its batches, cut at ``edges``.  An exit whose entry lies in
    an earlier batch carries entry_ref -1 and create_ts, or -2 when the oracle
    blocked that entry, as a caller would send it (so the oracle's verdicts on
    the whole trace are needed).  refs=False: the later batches carry no
    entry_ref array at all, every exit by create_ts."""
    o = od.DegradeOracle()
    o.load_rules(rules)
    st, _ = o.submit(full.res_id, full.ts_ms, full.flags, full.entry_ref, full.create_ts)
    batches = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        if hi == lo:
            continue
        b = full.subset(lo, hi)
        r = full.entry_ref[lo:hi]
        prior = (r >= 0) & (r < lo)
        dead = prior & np.isin(st[np.clip(r, 0, None)], (od.V_BLOCK_DEGRADE, od.V_BLOCK_OTHER))
        b.entry_ref[dead] = -2
        if not refs:
            ex = (b.flags & abi.EV_EXIT) != 0
            assert not dead.any() and np.all(b.entry_ref[ex] < 0), "refs=False: every exit's entry in an earlier batch"
            b = abi.HostBatch(b.res_id, b.ts_ms, b.count, b.flags, create_ts=b.create_ts)
        batches.append(b)
    return dict(rules=rules, batches=batches, R=R, full=full, **extra)


class Res:
    """One resource's script: every event one millisecond after the last
    unless told otherwise; ``pos`` counts the walked events of the current
    batch (the designed sorted position of the next event)."""

    def __init__(self, S, res, t=T0):
        self.S, self.res, self.t, self.pos = S, res, t, 0

    def at(self, t):
        assert t >= self.t
        self.t = t
        return self

    def cut(self, t):
        """A batch cut at time t: the next event starts a new segment."""
        self.at(t)
        self.pos = 0
        return self

    def entry(self, dt=1, preblocked=False, flags=0):
        self.t += dt
        h = self.S.add(self.res, self.t, flags | (abi.EV_BLOCKED if preblocked else 0))
        self.pos += not preblocked
        return h

    def exit(self, of=None, dt=1, err=False, create=None, ref=None, walked=True, flags=0):
        self.t += dt
        f = abi.EV_EXIT | (abi.EV_ERROR if err else 0) | flags
        if of is not None:
            h = self.S.add(self.res, self.t, f, ref=of)
        else:
            h = self.S.add(self.res, self.t, f, ref=-1 if ref is None else ref,
                           create=self.t if create is None else create)
        self.pos += walked
        return h

    def fill(self, upto, dt=0):
        """Entries (no state change on a CLOSED, an OPEN-before-retry or a
        HALF_OPEN breaker) up to sorted position ``upto``; dt=0 keeps the
        clock, but never puts an entry into the millisecond of an exit."""
        first = True
        out = []
        while self.pos < upto:
            out.append(self.entry(dt=max(dt, 1) if first else dt))
            first = False
        return out


def churn(S, res, n, seed, t=T0, err_p=0.4, dt_max=40, preblock=0):
    """Exactly n walked events of seeded entries and exits (every entry's exit
    follows after a few events if there is room)."""
    rng = np.random.default_rng(seed)
    r = Res(S, res, t)
    open_ = []
    while r.pos < n:
        if open_ and (rng.random() < 0.5 or len(open_) > 6):
            r.exit(of=open_.pop(0), dt=int(rng.integers(1, dt_max)), err=bool(rng.random() < err_p))
        else:
            open_.append(r.entry(dt=int(rng.integers(1, dt_max))))
    for _ in range(preblock):                      # pre-blocked entries and their exits: never walked
        h = r.entry(preblocked=True)
        r.exit(of=h, walked=False)
    return r


# ---------------------------------------------------------------- the path model
def valid_breakers(rules):
    """{resource: [global breaker index]} of the valid rules, in load order."""
    by, k = {}, 0
    for r in rules:
        if od.is_valid_rule(r):
            by.setdefault(int(r["resource"]), []).append(k)
            k += 1
    return by, k


def paths(rules, b):
    """k_dg_keys + the stable sort + k_dg_walk's choice, for one batch:
    {resource: dict(idx=walked events in order, walk='wave'|'lane', nb)}."""
    by, _ = valid_breakers(rules)
    ex = (b.flags & abi.EV_EXIT) != 0
    skip = ~ex & ((b.flags & abi.EV_BLOCKED) != 0)
    if b.entry_ref is not None:
        ref = b.entry_ref
        inb = ex & (ref >= 0)
        tgt = np.clip(ref, 0, b.n - 1)
        skip |= ex & (ref == -2)
        skip |= inb & (ref < np.arange(b.n)) & ((b.flags[tgt] & (abi.EV_BLOCKED | abi.EV_EXIT)) == abi.EV_BLOCKED)
    out = {}
    for r, cbs in by.items():
        idx = np.nonzero((b.res_id == r) & ~skip)[0]
        if idx.size:
            out[r] = dict(idx=idx, nb=len(cbs), walk="wave" if idx.size > HEAVY and len(cbs) <= MAXC else "lane")
    return out


def analyze(case):
    """Runs oracle/degrade.py with its transition log over the case and places
    every logged event on the kernels' paths.  Returns dict(status, rule_idx
    (per batch), states, trans=[dict(kind, res, batch, walk, pos, chunk, lane,
    n, cls, rolled)], routes={(batch, res): {route: [pos]}}, segs={(batch,
    res): (length, walk, nb)}, stops={(batch, res): {chunk: first stop lane}})."""
    rules, batches = case["rules"], case["batches"]
    o = od.DegradeOracle(log=True)
    nbrk = o.load_rules(rules)
    owner = {k: r for r, ks in o.by_res.items() for k in ks}
    outs, base, trans, routes, segs, stops = [], 0, [], {}, {}, {}
    for bi, b in enumerate(batches):
        n0 = len(o.transitions)
        outs.append(o.submit(b.res_id, b.ts_ms, b.flags, b.entry_ref, b.create_ts))
        st = outs[-1][0]
        p = paths(rules, b)
        where = {}
        for r, seg in p.items():
            segs[(bi, r)] = (int(seg["idx"].size), seg["walk"], seg["nb"])
            for q, i in enumerate(seg["idx"]):
                where[int(i)] = q
            if seg["walk"] == "wave":
                rt = routes.setdefault((bi, r), {k: [] for k in ROUTES})
                for q, i in enumerate(seg["idx"]):
                    if not b.flags[i] & abi.EV_EXIT:
                        continue
                    ref = -1 if b.entry_ref is None else int(b.entry_ref[i])
                    if ref < 0:
                        rt["cts"].append(q)
                    else:
                        d = q // 64 - where[ref] // 64
                        rt["same" if d == 0 else "prev" if d == 1 else "old"].append((q, where[ref], int(st[ref])))
        first = {}
        for ev, k, s0, s1, rolled in o.transitions[n0:]:
            i, r = ev - base, owner[k]
            q = where[i]
            if s0 != s1 or not rolled:
                first.setdefault((bi, r), {}).setdefault(q // 64, q % 64)
                first[(bi, r)][q // 64] = min(first[(bi, r)][q // 64], q % 64)
        stops.update(first)
        for ev, k, s0, s1, rolled in o.transitions[n0:]:
            i, r = ev - base, owner[k]
            q = where[i]
            n, walk, _ = segs[(bi, r)]
            kind = "roll" if s0 == s1 and rolled else KIND[(s0, s1)]
            cls = None
            if walk == "wave" and kind != "roll":
                cls = "bulk" if q % 64 >= 1 and first[(bi, r)][q // 64] == q % 64 else "serial"
            trans.append(dict(kind=kind, res=r, breaker=k, batch=bi, walk=walk, pos=q, chunk=q // 64, lane=q % 64, n=n,
                              cls=cls, rolled=bool(rolled), t=int(b.ts_ms[i]), i=i))
        base += b.n
    return dict(status=[s for s, _ in outs], rule_idx=[ri for _, ri in outs], states=[o.state(k) for k in range(nbrk)],
                trans=trans, routes=routes, segs=segs, stops=stops, by_res=dict(o.by_res))


def props_of(an):
    """The registry properties this analysis shows."""
    got = {f"walk:{w}" for _, w, _ in an["segs"].values()}
    for rt in an["routes"].values():
        got |= {f"route:{k}" for k, v in rt.items() if v}
    got |= {f"{t['cls']}:{t['kind']}" for t in an["trans"] if t["cls"] and t["kind"] in KINDS}
    return got


def _tr(an, res, batch=None, kinds=KINDS + ("fallback",)):
    return [t for t in an["trans"] if t["res"] == res and t["kind"] in kinds and (batch is None or t["batch"] == batch)]


# ---------------------------------------------------------------- seg_lengths
SEG_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)


def seg_lengths():
    """One-breaker resources of SEG_LENGTHS walked events (the 64|65 switch of
    k_dg_walk, a tail chunk of 1, the j+64 < j1 and j+128 < j1 prefetch
    conditions on equality and one either side); a 70-event resource with 6
    pre-blocked events (segment 64: lane walk); 65 events under 4 and under 5
    breakers; twins with the same traffic under 4 breakers and under the same 4
    plus an inert fifth (wave walk against lane walk directly)."""
    S, rules, want = Script(), [], {}
    for r, n in enumerate(SEG_LENGTHS):
        rules.append(rule(r, COUNT, 1, interval=300))
        churn(S, r, n, seed=100 + r)
        want[r] = (n, "wave" if n > HEAVY else "lane", 1)
    r = len(SEG_LENGTHS)
    rules.append(rule(r, COUNT, 1, interval=300))
    churn(S, r, 64, seed=120, preblock=3)
    want[r] = (64, "lane", 1)
    four = [(RT, 12.0, dict(ratio=0.4, interval=200)), (RATIO, 0.3, dict(min_req=2)), (COUNT, 2.0, dict(interval=500)),
            (RT, 25.0, dict(ratio=0.2, min_req=3))]
    for nb in (4, 5):
        r += 1
        rules += [rule(r, g, c, **kw) for g, c, kw in (four + [(COUNT, 1.0, {})])[:nb]]
        churn(S, r, 65, seed=130 + nb)
        want[r] = (65, "wave" if nb <= MAXC else "lane", nb)
    a, b = r + 1, r + 2
    for x in (a, b):
        rules += [rule(x, g, c, **kw) for g, c, kw in four]
        churn(S, x, 200, seed=140)
    rules.append(rule(b, COUNT, 1e9))                          # inert: no trace has 1e9 errors
    want[a], want[b] = (200, "wave", 4), (200, "lane", 5)
    full, edges = S.assemble()
    return finish(rules, full, edges, b + 1, want=want, twins=[(a, b, 4)])


def guard_seg_lengths(c, an):
    for r, w in c["want"].items():
        assert an["segs"][(0, r)] == w, (r, an["segs"][(0, r)], w)
    full = c["full"]
    assert int((full.res_id == len(SEG_LENGTHS)).sum()) == 70
    for a, b, _ in c["twins"]:
        ia, ib = np.nonzero(full.res_id == a)[0], np.nonzero(full.res_id == b)[0]
        assert np.array_equal(full.ts_ms[ia], full.ts_ms[ib]) and np.array_equal(full.flags[ia], full.flags[ib])
        assert np.array_equal(an["status"][0][ia], an["status"][0][ib])
        assert {t["kind"] for t in _tr(an, a)} >= set(KINDS) - {"reopen"}, "the twins' breakers move"
    st = an["status"][0]
    assert (st == od.V_BLOCK_DEGRADE).sum() > 20 and (st == od.V_EXIT_IGNORED).sum() > 5
    return props_of(an)


# ---------------------------------------------------------------- first_change_lane
FC_LANES = (0, 1, 62, 63)
FC_LEN = 192                                                   # three full chunks: first, middle, tail
CUT1 = T0 + 100_000                                            # second batch of the two-batch cases


def first_change_lane():
    """One resource per (kind of change, chunk, lane): the second batch's
    segment has three chunks and exactly one state change, at that lane of
    that chunk; the other two chunks change nothing (cut == cnt).  The state
    the change starts from is set up in the first batch (lane walk)."""
    S, rules, marks = Script(), [], {}
    r = 0
    for kind in KINDS:
        for chunk in range(3):
            for lane in FC_LANES:
                rules.append(rule(r, COUNT, 0))
                x = Res(S, r)
                if kind != "trip":                             # OPEN; the retry time falls behind the cut
                    x.at(CUT1 - (500 if kind == "probe" else 1500))
                e0 = x.entry()                                 # passes (CLOSED)
                if kind != "trip":
                    x.exit(of=e0, err=True)                    # -> OPEN, retry 1000 ms on
                    retry = x.t + 1000
                    if kind != "probe":
                        e0 = x.at(retry).entry(dt=0)           # the probe -> HALF_OPEN
                P = chunk * 64 + lane
                x.cut(CUT1).fill(P)
                if kind == "probe":
                    assert x.t < retry
                    x.at(max(x.t, CUT1 + 2000)).entry(dt=0 if P else 1)
                else:
                    x.exit(of=e0, err=kind != "close")
                x.fill(FC_LEN, dt=0)
                marks[r] = (kind, chunk, lane)
                r += 1
    full, edges = S.assemble(cuts=[CUT1])
    return finish(rules, full, edges, r, marks=marks)


def guard_first_change_lane(c, an):
    seen = set()
    for r, (kind, chunk, lane) in c["marks"].items():
        assert an["segs"][(1, r)] == (FC_LEN, "wave", 1), (r, an["segs"][(1, r)])
        tr = _tr(an, r, batch=1)
        assert [(t["kind"], t["chunk"], t["lane"]) for t in tr] == [(kind, chunk, lane)], (r, tr)
        assert an["stops"][(1, r)] == {chunk: lane}
        assert tr[0]["cls"] == ("serial" if lane == 0 else "bulk")
        seen.add((kind, chunk, lane))
    assert seen == {(k, ch, ln) for k in KINDS for ch in range(3) for ln in FC_LANES}
    return props_of(an)


# ---------------------------------------------------------------- window_rolls
WR_L = 100                                                     # stat_interval_ms of the roll cases
WR_N = 128                                                     # entries first, then their exits: chunks 2 and 3
# note -> (window edges, exits with an error, count): exit k (sorted position WR_N + k) lies in window
# sum(k >= e for e in edges); the exit before an edge at ws + L - 1, the one after it at the next
# ws.  The breaker trips at the (count + 1)th error of one window.
ROLLS = {
    # a boundary between lanes a | a + 1: errors on both sides that only trip if the counts do not restart
    "roll 0|1": ([1], [0, 1, 2], 1.0),
    "roll 31|32": ([32], [0, 31, 32, 33, 34], 2.0),
    "roll 62|63": ([63], [0, 62, 63, 64, 65], 2.0),
    "roll 63|next chunk's 0": ([64], [62, 63, 64, 65, 70], 2.0),
    "three windows": ([21, 41], [0, 20, 21, 40, 41, 42, 43], 2.0),
    "one window": ([], [10, 20, 30], 2.0),
    # the first run of the next chunk needs the two errors counted in the previous chunk
    "carry from the previous chunk": ([], [10, 20, 69], 2.0),
    # a later run must not take them: window A (all of chunk 2, ten lanes of chunk 3) holds two
    # errors, window B trips at its own third ...
    "later run": ([74], [0, 1, 74, 90, 91], 2.0),
    # ... and 74 clean requests of window A must not dilute window B's ratio: its first request,
    # an error, is 1/1 > 0.5 (with A's counts 1/75)
    "later run, ratio": ([74], [74], 0.5),
}


def window_rolls():
    """Exits of one-breaker resources around stat_interval_ms boundaries
    (ROLLS); two errors before a batch cut and the third after it in the same
    window; a window that only an entry, or only an ignored exit, enters; two
    breakers of intervals 200 and 1000 on one resource."""
    S, rules, marks = Script(), [], {}
    r = 0
    base = T0 + 1000
    for note, (edges, errs, count) in ROLLS.items():
        rules.append(rule(r, RATIO if count < 1 else COUNT, count, interval=WR_L, tw=50))
        x = Res(S, r, T0 + 500)
        ent = x.fill(WR_N)
        for k in range(WR_N):
            w = sum(k >= e for e in edges)
            last = w < len(edges) and k == edges[w] - 1
            x.at(base + w * WR_L + (WR_L - 1 if last else 0)).exit(of=ent[k], dt=0, err=k in errs)
        marks[r] = dict(note=note, edges=edges, errs=errs, count=count)
        r += 1
    rules.append(rule(r, COUNT, 2.0, interval=1_000_000, tw=50))
    x = Res(S, r)
    ent = x.fill(70)
    x.exit(of=ent[0], err=True)
    x.exit(of=ent[1], err=True)
    x.cut(CUT1).fill(3)
    for k in range(2, 70):
        x.exit(of=ent[k], err=k == 6)
    marks[r] = dict(note="carry from the previous batch")
    r += 1
    # the bucket keeps the old window's counts until a counted exit arrives
    # (LeapArray.currentWindow runs in onRequestComplete only)
    rules.append(rule(r, COUNT, 5.0, interval=WR_L))
    x = Res(S, r)
    ent = x.fill(70)
    x.exit(of=ent[0], err=True)
    ws = x.t - x.t % WR_L
    x.at(ws + 3 * WR_L).entry()
    marks[r] = dict(note="entry only", ws=ws, counts=(1, 1))
    r += 1
    rules += [rule(r, COUNT, 0.0, tw=50), rule(r, COUNT, 100.0, interval=WR_L)]
    x = Res(S, r)
    ent = x.fill(70)
    x.exit(of=ent[0], err=True)                                # breaker 0 opens; breaker 1 counts 1 / 1
    ws = x.t - x.t % WR_L
    blocked = x.entry()
    x.at(ws + 3 * WR_L).exit(of=blocked)                       # ignored: breaker 1's window does not roll
    marks[r] = dict(note="ignored exit only", ws=ws, counts=(1, 1))
    r += 1
    rules += [rule(r, COUNT, 2.0, interval=200), rule(r, RATIO, 0.5, interval=1000, min_req=4)]
    churn(S, r, 300, seed=210, dt_max=30)
    marks[r] = dict(note="intervals 200 and 1000")
    r += 1
    full, edges = S.assemble(cuts=[CUT1])
    return finish(rules, full, edges, r, marks=marks)


def guard_window_rolls(c, an):
    notes = set()
    b0 = c["batches"][0]
    for r, m in c["marks"].items():
        notes.add(m["note"])
        rolls = [t for t in an["trans"] if t["res"] == r and t["rolled"]]
        trips = _tr(an, r, kinds=("trip",))
        if "edges" in m:
            assert an["segs"][(0, r)] == (2 * WR_N, "wave", 1)
            assert sorted({t["pos"] for t in rolls}) == [WR_N] + [WR_N + e for e in m["edges"]], (r, m, rolls)
            idx = paths(c["rules"], b0)[r]["idx"]
            for e in m["edges"]:                               # events at ws + L - 1 and ws + L
                t = b0.ts_ms[idx[WR_N + e]]
                assert t % WR_L == 0 and b0.ts_ms[idx[WR_N + e - 1]] == t - 1, (r, m)
            w_of = lambda k: sum(k >= e for e in m["edges"])                      # noqa: E731
            assert len(trips) == 1, (r, m, trips)
            k_trip = trips[0]["pos"] - WR_N
            in_w = [e for e in m["errs"] if w_of(e) == w_of(k_trip) and e <= k_trip]
            assert len(in_w) == int(m["count"]) + 1 and in_w[-1] == k_trip == m["errs"][-1], (r, m, k_trip)
            if m["note"].startswith("later run"):              # window A's counts come from the chunk before
                assert w_of(k_trip) == 1 and trips[0]["chunk"] == 3 and m["edges"][0] % 64 > 0
                assert all(e < 64 for e in m["errs"] if w_of(e) == 0)
                first_b = [t for t in an["trans"] if t["res"] == r and t["rolled"]][-1]
                assert (first_b["chunk"], first_b["lane"]) == (3, m["edges"][0] - 64)
            if m["note"] == "carry from the previous chunk":
                assert (trips[0]["chunk"], trips[0]["cls"]) == (3, "bulk") and max(m["errs"][:-1]) < 64
            if m["note"] == "roll 63|next chunk's 0":
                assert rolls[-1]["lane"] == 0 and rolls[-1]["chunk"] == 3
        elif m["note"] == "carry from the previous batch":
            assert an["segs"][(1, r)][1] == "wave" and len(trips) == 1
            assert (trips[0]["batch"], trips[0]["chunk"], trips[0]["cls"]) == (1, 0, "bulk")
        elif "ws" in m:
            s = an["states"][an["by_res"][r][-1]]
            assert (s["window_start"], s["hit_count"], s["total_count"]) == (m["ws"],) + m["counts"], (r, s)
            last = c["full"].ts_ms[c["full"].res_id == r][-1]
            assert last - last % WR_L > m["ws"], "the last event lies in a later window"
            assert an["segs"][(0, r)][1] == "wave"
        else:
            assert an["segs"][(0, r)] == (300, "wave", 2) and len(trips) >= 2
    assert notes == set(ROLLS) | {"carry from the previous batch", "entry only", "ignored exit only",
                                  "intervals 200 and 1000"}
    return props_of(an)


# ---------------------------------------------------------------- thresholds
BELOW_THIRD = math.nextafter(0.3333333333333333, 0.0)
NAN = float("nan")
# name -> (rules of the resource, requests [(rt ms, error)], tripped?).  The
# last column is derived by hand from the reference and written as a literal:
#   ExceptionCircuitBreaker.java:106-108  totalCount < minRequestAmount returns
#   ExceptionCircuitBreaker.java:110-118  ratio = errCount * 1.0d / totalCount; trips on curCount > threshold
#   ResponseTimeCircuitBreaker.java:52    maxAllowedRt = Math.round(count); :78 slow when rt > maxAllowedRt
#   ResponseTimeCircuitBreaker.java:116-129  ratio > max trips; ratio == max trips only when max == 1.0
#   DegradeRuleManager.java:183-204       isValidRule: count >= 0 and 0 <= slowRatioThreshold <= 1 are false for NaN
THRESHOLDS = {
    "min_req_exact": ([(COUNT, 0.0, dict(min_req=3))], [(0, True)] * 3, True),
    "min_req_one_under": ([(COUNT, 0.0, dict(min_req=3))], [(0, True)] * 2, False),
    "ratio_half_equal": ([(RATIO, 0.5, dict(min_req=2))], [(0, True), (0, False)], False),
    "rt_ratio_one_all_slow": ([(RT, 10.0, dict(ratio=1.0, min_req=2))], [(11, False)] * 2, True),
    "exc_ratio_one_all_errors": ([(RATIO, 1.0, dict(min_req=1))], [(0, True)] * 6, False),
    "third_equal": ([(RATIO, 0.3333333333333333, dict(min_req=3))], [(0, True), (0, False), (0, False)], False),
    "third_next_below": ([(RATIO, BELOW_THIRD, dict(min_req=3))], [(0, True), (0, False), (0, False)], True),
    "count_equal": ([(COUNT, 2.0, {})], [(0, True)] * 2, False),
    "count_plus_one": ([(COUNT, 2.0, {})], [(0, True)] * 3, True),
    "count_fraction_two": ([(COUNT, 2.5, {})], [(0, True)] * 2, False),
    "count_fraction_three": ([(COUNT, 2.5, {})], [(0, True)] * 3, True),
    "rt_equal_round": ([(RT, 10.4, dict(ratio=0.5))], [(10, False)], False),
    "rt_round_plus_one": ([(RT, 10.4, dict(ratio=0.5))], [(11, False)], True),
    "rt_round_half_up": ([(RT, 10.5, dict(ratio=0.5))], [(11, False)], False),
    "rt_tiny_count_zero": ([(RT, 0.49999999999999994, dict(ratio=0.5))], [(0, False)], False),
    "rt_tiny_count_one": ([(RT, 0.49999999999999994, dict(ratio=0.5))], [(1, False)], True),
    "rt_ratio_zero_none_slow": ([(RT, 10.0, dict(ratio=0.0))], [(10, False)] * 3, False),
    "rt_ratio_zero_one_slow": ([(RT, 10.0, dict(ratio=0.0))], [(10, False), (10, False), (11, False)], True),
    # the two NaN rules are dropped: the third rule is breaker 0 of its resource
    "nan_rules_dropped": ([(COUNT, NAN, {}), (RT, 10.0, dict(ratio=NAN)), (COUNT, 0.0, {})], [(0, True)], True),
}
TH_LEAD = 70                                                   # leading entries of the wave-walk copy


def thresholds():
    """Every THRESHOLDS scenario twice: on a short segment (lane walk) and
    behind 70 passed entries (wave walk; the requests' exits sit in the second
    chunk at lanes >= 6, so a trip is found by the bulk prefix).  After the
    requests one more entry shows whether the breaker tripped."""
    S, rules, marks = Script(), [], {}
    r = 0
    for name, (rs, reqs, tripped) in THRESHOLDS.items():
        for lead in (0, TH_LEAD):
            rules += [rule(r, g, cnt, tw=50, **kw) for g, cnt, kw in rs]
            x = Res(S, r)
            x.fill(lead)
            x.at(T0 + 200)
            ents = [x.entry(dt=0) for _ in reqs]
            t0 = x.t
            for e, (rt, err) in sorted(zip(ents, reqs), key=lambda p: p[1][0]):
                x.at(t0 + max(rt, 0)).exit(of=e, dt=0, err=err)
            probe = x.entry()
            marks[r] = (name, lead, probe)
            r += 1
    full, edges = S.assemble()
    c = finish(rules, full, edges, r, marks=marks)
    c["probe"] = {res: int(S.pos[p]) for res, (_, _, p) in marks.items()}
    return c


def threshold_verdicts(c, status, rule_idx):
    """{(name, lead): tripped} from a run's verdicts; a block must name breaker 0."""
    out = {}
    for res, (name, lead, _) in c["marks"].items():
        i = c["probe"][res]
        assert status[i] in (od.V_PASS, od.V_BLOCK_DEGRADE)
        out[(name, lead)] = bool(status[i] == od.V_BLOCK_DEGRADE)
        if out[(name, lead)]:
            assert rule_idx[i] == 0, (name, rule_idx[i])
    return out


def threshold_expect():
    return {(name, lead): v[2] for name, v in THRESHOLDS.items() for lead in (0, TH_LEAD)}


def guard_thresholds(c, an):
    assert threshold_verdicts(c, an["status"][0], an["rule_idx"][0]) == threshold_expect()
    for res, (name, lead, _) in c["marks"].items():
        n, walk, nb = an["segs"][(0, res)]
        assert walk == ("wave" if lead else "lane") and nb == 1, (name, lead, n, walk, nb)
        for t in _tr(an, res):
            assert t["kind"] == "trip" and (not lead or t["cls"] == "bulk"), (name, t)
    _, n = valid_breakers(c["rules"])
    assert n == len(c["rules"]) - 4, "two NaN rules dropped on each of two resources"
    return props_of(an)


# ---------------------------------------------------------------- retry_and_probe
def _trip(x):
    """entry + error exit on an exception-count-0 breaker: OPEN, returns the exit's time."""
    x.exit(of=x.entry(), err=True)
    return x.t


def retry_and_probe():
    """Entries one millisecond before and at next_retry with the probe at
    chosen lanes, the probe's exit at growing distances (clean and a hit),
    probes that a later breaker sends back (2, 4 and 64 breakers)."""
    S, rules, marks = Script(), [], {}
    r = 0
    # the probe at next_retry (the entry one millisecond earlier is blocked), at lanes 0, 17, 63
    # of the second chunk; its exit in the same chunk, the next, two later, or the next batch;
    # clean (close, later counts from 0) or a hit (re-open, next_retry = exit t + recovery)
    for lane in (0, 17, 63):
        for where in ("same", "next", "two", "batch"):
            if lane == 63 and where == "same":
                continue
            for hit in (False, True):
                rules.append(rule(r, COUNT, 0))
                x = Res(S, r)
                t_open = _trip(x)
                x.fill(64 + lane - 1)
                x.at(t_open + 999).entry(dt=0)                 # next_retry - 1: blocked
                p = x.at(t_open + 1000).entry(dt=0)            # next_retry: probes
                ppos = x.pos - 1
                if where == "batch":
                    x.fill(140)
                    x.cut(CUT1).fill(3)
                else:
                    x.fill({"same": ppos + 1, "next": 128 + 5, "two": 192 + 5}[where])
                x.exit(of=p, err=hit)
                t_x = x.t
                if hit:
                    x.at(t_x + 999).entry(dt=0)
                    x.at(t_x + 1000).entry(dt=0)
                else:
                    e = x.entry()
                    x.exit(of=e, err=True)                     # counts from 0: the first error trips again
                marks[r] = dict(kind="probe", lane=lane, where=where, hit=hit, probe=p, retry=t_open + 1000,
                                retry2=t_x + 1000)
                r += 1
    # probe fallback with 2 and 4 breakers, each position in turn the first non-CLOSED one
    for nb in (2, 4):
        for first in range(nb - 1):
            for blk in sorted({first + 1, nb - 1}):
                for lead in (0, 70):
                    rs = [rule(r, RT, 1e9, tw=1) for _ in range(nb)]             # never slow: stays CLOSED
                    rs[first] = rule(r, COUNT, 0, tw=1)
                    rs[blk] = rule(r, COUNT, 0, tw=5)
                    rules += rs
                    x = Res(S, r)
                    x.fill(lead)
                    t_open = _trip(x)
                    a = x.at(t_open + 1000).entry(dt=0)        # `first` probes, `blk` blocks: falls back
                    b = x.entry()                              # probes again
                    b2 = x.at(t_open + 4999).entry(dt=0)       # and again, one millisecond before `blk` lets go
                    d = x.at(t_open + 5000).entry(dt=0)        # both probe: passes
                    x.exit(of=d)                               # both close
                    marks[r] = dict(kind="fallback", nb=nb, first=first, blk=blk, lead=lead, blocked=[a, b, b2],
                                    passed=d, retry=t_open + 1000)
                    r += 1
    # 64 breakers (lane walk): 0..62 OPEN with their retry reached, 63 blocks
    rules += [rule(r, COUNT, 0, tw=1 if k < MAX_BREAKERS - 1 else 5) for k in range(MAX_BREAKERS)]
    x = Res(S, r)
    t_open = _trip(x)
    a = x.at(t_open + 1000).entry(dt=0)
    d = x.at(t_open + 5000).entry(dt=0)
    x.exit(of=d, err=True)                                     # all 64 re-open
    marks[r] = dict(kind="wide", blocked=[a], passed=d)
    r += 1
    full, edges = S.assemble(cuts=[CUT1])
    c = finish(rules, full, edges, r, marks=marks)
    c["pos"] = S.pos
    return c


def guard_retry_and_probe(c, an):
    full, pos = c["full"], c["pos"]
    st = np.concatenate(an["status"])
    ri = np.concatenate(an["rule_idx"])
    for r, m in c["marks"].items():
        if m["kind"] == "probe":
            i = int(pos[m["probe"]])
            assert full.ts_ms[i] == m["retry"] and st[i] == od.V_PASS, (r, m)
            prev = np.nonzero((full.res_id == r) & (np.arange(full.n) < i))[0][-1]
            assert full.ts_ms[prev] == m["retry"] - 1 and st[prev] == od.V_BLOCK_DEGRADE, (r, m)
            tr = _tr(an, r)
            p = [t for t in tr if t["kind"] == "probe"][0]
            assert (p["chunk"], p["lane"], p["walk"]) == (1, m["lane"], "wave"), (r, m, p)
            nxt = tr[tr.index(p) + 1]
            assert nxt["kind"] == ("reopen" if m["hit"] else "close")
            want = dict(same=(0, 1), next=(0, 2), two=(0, 3), batch=(1, 0))[m["where"]]
            assert (nxt["batch"], nxt["chunk"]) == want, (r, m, nxt)
            if m["hit"]:
                sel = np.nonzero((full.res_id == r) & (full.ts_ms >= m["retry2"] - 1))[0]
                assert [int(x) for x in st[sel[-2:]]] == [od.V_BLOCK_DEGRADE, od.V_PASS], (r, m)
                assert list(full.ts_ms[sel[-2:]]) == [m["retry2"] - 1, m["retry2"]]
            else:
                assert tr[-1]["kind"] == "trip" and tr[-1]["pos"] > nxt["pos"] or tr[-1]["batch"] > nxt["batch"]
        else:
            ks = an["by_res"][r]
            for h in m["blocked"]:
                i = int(pos[h])
                want = m["blk"] if m["kind"] == "fallback" else MAX_BREAKERS - 1
                assert st[i] == od.V_BLOCK_DEGRADE and ri[i] == want, (r, m, st[i], ri[i])
            assert st[int(pos[m["passed"]])] == od.V_PASS
            fb = [t for t in an["trans"] if t["res"] == r and t["kind"] == "fallback"]
            if m["kind"] == "fallback":
                assert [t["breaker"] for t in fb] == [ks[m["first"]]] * 3, (r, m, fb)
                assert an["segs"][(0, r)][1] == ("wave" if m["lead"] else "lane")
            else:
                assert len(ks) == MAX_BREAKERS and sorted(t["breaker"] for t in fb) == ks[:-1]
                assert an["segs"][(0, r)][1] == "lane"
    fbs = {(m["nb"], m["first"]) for m in c["marks"].values() if m["kind"] == "fallback"}
    assert fbs == {(2, 0), (4, 0), (4, 1), (4, 2)}
    return props_of(an)


# ---------------------------------------------------------------- ignored_exits
IGN_PLACES = ("same_before_cut", "same_after_cut", "same_serial", "prev_bit0", "prev_bit63", "two_back", "ten_back")
# (entry lane in chunk 1, the entry is refused?): the entry's neighbours in the mask have the other verdict
IGN_NEIGHBOURS = {"probe_bit0": (0, False), "probe_bit63": (63, False), "refused_bit0_before_probe": (0, True),
                  "refused_bit63_after_trip": (63, True)}


def ignored_exits(refs=True):
    """The exit of an entry the breaker blocked, and of one it passed, with
    that entry in each position of IGN_PLACES relative to the exit; an exit by
    create_ts (entry_ref -1), an exit with entry_ref -2.  refs=False: the
    second batch carries no entry_ref array at all, every exit by create_ts."""
    S, rules, marks = Script(), [], {}
    r = 0
    if not refs:
        for k in range(3):
            rules.append(rule(r, COUNT, 1, interval=200))
            x = Res(S, r)
            ent = x.fill(80 if k else 20)
            x.cut(CUT1)
            for j, e in enumerate(ent):
                x.exit(of=e, err=j % 3 == k)
            marks[r] = dict(kind="cts")
            r += 1
        full, edges = S.assemble(cuts=[CUT1])
        return finish(rules, full, edges, r, refs=False, marks=marks)
    for blocked in (True, False):
        for place in IGN_PLACES:
            if place == "same_serial" and not blocked:
                continue
            rules.append(rule(r, COUNT, 0))
            x = Res(S, r)
            x.at(CUT1 - 500)
            e0 = x.entry()
            e1 = x.entry()
            if blocked:
                x.exit(of=e0, err=True)                        # OPEN from the first batch on, retry behind the cut
            t_open = x.t
            x.cut(CUT1)
            chunks = 12 if place == "ten_back" else 4
            pe, px = {"same_before_cut": (70, 80), "same_after_cut": (70, 90), "same_serial": (87, 95),
                      "prev_bit0": (64, 130), "prev_bit63": (127, 128), "two_back": (70, 64 * 3 + 9),
                      "ten_back": (70, 64 * 11 + 9)}[place]
            if place == "same_serial":
                x.fill(85)
                x.at(CUT1 + 5000).entry(dt=0)                  # the stop: a probe (retry long reached)
                x.fill(pe, dt=0)
                e = x.entry(dt=0)                              # refused by the HALF_OPEN breaker, after the cut
            else:
                x.fill(pe)
                e = x.entry(dt=0)
                if place == "same_after_cut":
                    x.fill(85, dt=0)
                    if blocked:
                        x.at(CUT1 + 5000).entry(dt=0)          # the stop: a probe
                    else:
                        x.exit(of=e1, err=True)                # the stop: a trip
            x.fill(px, dt=0)
            h = x.exit(of=e, err=True)
            x.fill(chunks * 64, dt=0)
            marks[r] = dict(kind="place", blocked=blocked, place=place, pe=pe, px=px, exit=h, t_open=t_open)
            r += 1
    # one bit of the previous chunk's mask that differs from its neighbours
    for place, (lane, blocked) in IGN_NEIGHBOURS.items():
        rules.append(rule(r, COUNT, 0))
        x = Res(S, r)
        x.at(CUT1 - 500)
        e0 = x.entry()
        if place != "refused_bit63_after_trip":
            x.exit(of=e0, err=True)                            # OPEN, retry behind the cut
        x.cut(CUT1)
        if place == "refused_bit63_after_trip":
            x.fill(64 + 62)                                    # passed
            x.exit(of=e0, err=True)                            # lane 62: trips
            e = x.entry()                                      # lane 63: refused
        elif place == "refused_bit0_before_probe":
            x.fill(64)
            e = x.entry(dt=0)                                  # lane 0: refused, one millisecond early
            x.at(CUT1 + 5000).entry(dt=0)                      # lane 1: probes
        else:
            x.fill(64 + lane)                                  # refused
            e = x.at(CUT1 + 5000).entry(dt=0)                  # the probe: the one passed entry of the chunk
        pe = x.pos - 1 if place != "refused_bit0_before_probe" else 64
        x.fill(128 + 7, dt=0)
        h = x.exit(of=e)
        x.fill(192, dt=0)
        marks[r] = dict(kind="neighbour", blocked=blocked, place=place, pe=pe, px=128 + 7, exit=h)
        r += 1
    # entry_ref -1 with create_ts and entry_ref -2, on a wave segment
    rules.append(rule(r, RT, 10.0, ratio=0.5, tw=50))
    x = Res(S, r)
    x.fill(70)
    a = x.exit(create=x.t - 10, ref=-1)                        # rt 11: slow -> trips
    b = x.exit(ref=-2, walked=False)
    marks[r] = dict(kind="minus", cts=a, dead=b)
    r += 1
    full, edges = S.assemble(cuts=[CUT1])
    c = finish(rules, full, edges, r, marks=marks)
    c["pos"] = S.pos
    return c


def guard_ignored_exits(c, an):
    st = np.concatenate(an["status"])
    seen = set()
    for r, m in c["marks"].items():
        if m["kind"] == "cts":
            assert c["batches"][1].entry_ref is None and c["batches"][1].create_ts is not None
            assert an["routes"].get((1, r), {}).get("cts") or an["segs"][(1, r)][1] == "lane"
            seen.add(an["segs"][(1, r)][1])
            continue
        if m["kind"] == "minus":
            ia, ib = int(c["pos"][m["cts"]]), int(c["pos"][m["dead"]])
            assert st[ia] == od.V_EXIT and st[ib] == od.V_EXIT_IGNORED
            assert [t["kind"] for t in _tr(an, r)] == ["trip"] and an["routes"][(0, r)]["cts"] == [70]
            continue
        i = int(c["pos"][m["exit"]])
        assert st[i] == (od.V_EXIT_IGNORED if m["blocked"] else od.V_EXIT), (r, m, st[i])
        assert an["segs"][(1, r)][1] == "wave"
        if m["kind"] == "neighbour":
            hit = [x for x in an["routes"][(1, r)]["prev"] if x[0] == m["px"]]
            assert hit and hit[0][1] == m["pe"] == 64 + IGN_NEIGHBOURS[m["place"]][0], (r, m, hit)
            b1 = c["batches"][1]
            idx = paths(c["rules"], b1)[r]["idx"]
            refused = an["status"][1][idx[64:128]] == od.V_BLOCK_DEGRADE
            k = m["pe"] - 64
            assert refused[k] == m["blocked"] and refused[(k + 1) % 64] != refused[k], (r, m)
            assert k == 0 or refused[k - 1] != refused[k] or m["place"] == "refused_bit63_after_trip"
            seen.add(m["place"])
            continue
        route = {"same": "same", "prev": "prev", "two_": "old", "ten_": "old"}[m["place"][:4]]
        hit = [x for x in an["routes"][(1, r)][route] if x[0] == m["px"]]
        assert hit and hit[0][1] == m["pe"], (r, m, an["routes"][(1, r)])
        assert (hit[0][2] == od.V_BLOCK_DEGRADE) == m["blocked"]
        cut = an["stops"].get((1, r), {}).get(m["px"] // 64)
        if m["place"] == "same_before_cut":
            assert cut is None or cut >= m["px"] % 64
        if m["place"] in ("same_after_cut", "same_serial"):
            assert cut is not None and cut < m["px"] % 64
            assert (cut < m["pe"] % 64) == (m["place"] == "same_serial")
        if m["place"] == "prev_bit0":
            assert m["pe"] % 64 == 0
        if m["place"] == "prev_bit63":
            assert m["pe"] % 64 == 63
        if m["place"] == "ten_back":
            assert m["px"] // 64 - m["pe"] // 64 == 10
        seen.add((m["blocked"], m["place"]))
    if any(m["kind"] == "place" for m in c["marks"].values()):
        want = {(b, p) for b in (True, False) for p in IGN_PLACES if b or p != "same_serial"}
        assert seen == want | set(IGN_NEIGHBOURS)
    else:
        assert seen == {"wave", "lane"}
    return props_of(an)


# ---------------------------------------------------------------- batch_cuts
def batch_cuts():
    """A cut while OPEN, while HALF_OPEN (the probe in flight across it) and
    in the middle of a window with counts; each once with the wave walk before
    the cut and the lane walk after it, and once the other way round."""
    S, rules, marks = Script(), [], {}
    r = 0
    for what in ("open", "half_open", "mid_window"):
        for wave_first in (True, False):
            n1, n2 = (100, 20) if wave_first else (20, 100)
            rules.append(rule(r, COUNT, 0 if what != "mid_window" else 2, interval=1_000_000))
            x = Res(S, r)
            if what == "mid_window":
                ent = x.fill(n1 - 2)
                x.exit(of=ent[0], err=True)
                x.exit(of=ent[1], err=True)
                x.cut(CUT1).fill(n2 - 10, dt=0)
                x.exit(of=ent[2], err=True)                    # the third error of the window: trips
                x.fill(n2, dt=0)
            else:
                e = x.fill(n1 - 12)[0]
                x.exit(of=e, err=True)
                t_open = x.t
                x.fill(n1 - 1 - (what == "half_open"))
                if what == "half_open":
                    p = x.at(t_open + 1000).entry(dt=0)
                    x.entry()
                    x.cut(CUT1).fill(n2 - 10, dt=0)
                    x.exit(of=p)                               # closes
                else:
                    x.entry()
                    x.cut(CUT1).fill(n2 - 10, dt=0)            # retry long reached: the first entry probes
                x.fill(n2)
            marks[r] = dict(what=what, walks=("wave", "lane") if wave_first else ("lane", "wave"), n=(n1, n2))
            r += 1
    full, edges = S.assemble(cuts=[CUT1])
    return finish(rules, full, edges, r, marks=marks)


def guard_batch_cuts(c, an):
    o = od.DegradeOracle()
    o.load_rules(c["rules"])
    b = c["batches"][0]
    o.submit(b.res_id, b.ts_ms, b.flags, b.entry_ref, b.create_ts)
    for r, m in c["marks"].items():
        assert (an["segs"][(0, r)][:2], an["segs"][(1, r)][:2]) == tuple(zip(m["n"], m["walks"])), (r, m)
        s = o.state(an["by_res"][r][0])
        if m["what"] == "mid_window":
            assert (s["state"], s["hit_count"], s["total_count"]) == (od.CLOSED, 2, 2)
            assert [t["kind"] for t in _tr(an, r, batch=1)] == ["trip"]
        else:
            assert s["state"] == (od.OPEN if m["what"] == "open" else od.HALF_OPEN), (r, m, s)
            assert [t["kind"] for t in _tr(an, r, batch=1)][:1] == ["probe" if m["what"] == "open" else "close"]
    return props_of(an)


# ---------------------------------------------------------------- many_segments
def many_segments(n_res=GRID + 3, per=65):
    """GRID + 3 one-breaker resources of 65 walked events each (k_dg_wave's
    grid-stride loop runs a second time for three waves), with events of
    resources without a breaker in between."""
    pairs = per // 2
    res = np.repeat(np.arange(n_res, dtype=np.int64), pairs)
    k = np.tile(np.arange(pairs, dtype=np.int64), n_res)
    t_en = T0 + k * 40 + res % 7
    err = (k + res) % 5 < 2
    last = np.arange(n_res, dtype=np.int64)                    # the 65th event: an entry
    free = n_res + np.arange(7000, dtype=np.int64) % 5         # resources n_res .. n_res + 4: no breaker
    ts = np.concatenate([t_en, t_en + 3, T0 + pairs * 40 + last % 7, T0 + (np.arange(7000) * pairs * 40) // 7000])
    isx = np.concatenate([np.zeros(res.size), np.ones(res.size), np.zeros(n_res), np.zeros(7000)]).astype(np.int64)
    rs = np.concatenate([res, res, last, free])
    fl = np.concatenate([np.zeros(res.size), np.where(err, abi.EV_EXIT | abi.EV_ERROR, abi.EV_EXIT),
                         np.zeros(n_res), np.zeros(7000)]).astype(np.uint8)
    order = np.lexsort((np.arange(ts.size), isx, ts))
    pos = np.empty(ts.size, np.int64)
    pos[order] = np.arange(ts.size)
    ref = np.full(ts.size, -1, np.int64)
    ref[res.size:2 * res.size] = pos[:res.size]
    full = abi.HostBatch(rs[order].astype(np.uint32), ts[order], np.ones(ts.size, np.int32), fl[order],
                         entry_ref=ref[order], create_ts=np.zeros(ts.size, np.int64))
    rules = [rule(r, COUNT, float(r % 3), interval=500) for r in range(n_res)]
    return dict(rules=rules, batches=[full], R=n_res + 5, full=full)


def guard_many_segments(c, an):
    segs = an["segs"]
    assert len(segs) == GRID + 3 and all(v == (65, "wave", 1) for v in segs.values())
    assert 130_000 < c["full"].n < 150_000
    free = c["full"].res_id >= GRID + 3
    assert 5000 < free.sum() and (np.diff(np.nonzero(free)[0]) > 1).any()
    st = an["status"][0]
    assert (st == od.V_BLOCK_DEGRADE).sum() > 1000 and (st == od.V_EXIT_IGNORED).sum() > 1000
    late = {t["res"] for t in an["trans"] if t["res"] >= GRID}
    assert late == {GRID, GRID + 1, GRID + 2}, "the second trip of the grid-stride loop changes state"
    return props_of(an)


KEY_COUNTS = (1, 2, 255, 256)                                  # key_bits of n_rres + 1 keys: 1, 2, 8, 9


def key_widths(n):
    """n breaker resources (dense ids 0 .. n-1, the "no breaker" key n: the
    radix key-width borders of the loader's key_bits) between resources
    without a breaker; a wave segment on the first and on the last dense id."""
    S, rules = Script(), []
    ids = [2 * k + 1 for k in range(n)]                        # odd resources carry a breaker
    for j, r in enumerate(ids):
        rules.append(rule(r, COUNT, 1, interval=300))
        churn(S, r, 70 if j in (0, n - 1) else 6 + j % 5, seed=300 + j)
        churn(S, r - 1, 3, seed=900 + j)
    full, edges = S.assemble()
    return finish(rules, full, edges, 2 * n, ids=ids)


def guard_key_widths(c, an):
    n = len(c["ids"])
    assert n in KEY_COUNTS and len({r for _, r in an["segs"]}) == n
    assert an["segs"][(0, c["ids"][0])][1] == "wave" and an["segs"][(0, c["ids"][-1])][1] == "wave"
    assert (c["full"].res_id % 2 == 0).sum() == 3 * n
    return props_of(an)


# ---------------------------------------------------------------- the registry
CASES = {
    "seg_lengths": (seg_lengths, guard_seg_lengths),
    "first_change_lane": (first_change_lane, guard_first_change_lane),
    "window_rolls": (window_rolls, guard_window_rolls),
    "thresholds": (thresholds, guard_thresholds),
    "retry_and_probe": (retry_and_probe, guard_retry_and_probe),
    "ignored_exits": (ignored_exits, guard_ignored_exits),
    "ignored_exits_no_refs": (lambda: ignored_exits(refs=False), guard_ignored_exits),
    "batch_cuts": (batch_cuts, guard_batch_cuts),
    "many_segments": (many_segments, guard_many_segments),
}
for _n in KEY_COUNTS:
    CASES[f"key_widths_{_n}"] = (lambda n=_n: key_widths(n), guard_key_widths)


# ---------------------------------------------------------------- section 0: recovery time
# time_window_s -> recoveryTimeoutMs, Java int arithmetic (AbstractCircuitBreaker.java:36,54)
RECOVERY_MS = {2147483: 2147483000, 2147484: -2147483296, 4294967: -296, 4294968: 704, 2147483647: -1000}
REC_TRIP = T0 + 7                                              # the trip's exit time


def recovery():
    """One exception-count-0 breaker per time window of RECOVERY_MS: a trip at
    REC_TRIP, then an entry one millisecond later, one at REC_TRIP + 703 and one
    at REC_TRIP + 704; the literal expectations are recovery_expect()."""
    S, rules = Script(), []
    for r, tw in enumerate(RECOVERY_MS):
        rules.append(rule(r, COUNT, 0, tw=tw))
        x = Res(S, r, REC_TRIP - 2)
        x.exit(of=x.entry(), err=True)
        assert x.t == REC_TRIP
        x.entry()
        x.at(REC_TRIP + 703).entry(dt=0)
        x.at(REC_TRIP + 704).entry(dt=0)
    full, edges = S.assemble()
    return finish(rules, full, edges, len(RECOVERY_MS))


def recovery_expect():
    """{resource: (next_retry_ms after the trip, verdicts of the three later
    entries)}, by hand: a negative recovery puts next_retry before the trip, so
    the next entry probes (HALF_OPEN) and the two after it are refused; 704
    refuses until REC_TRIP + 704; 2147483000 refuses all three."""
    P, B = od.V_PASS, od.V_BLOCK_DEGRADE
    want = {2147483: (REC_TRIP + 2147483000, [B, B, B]), 2147484: (REC_TRIP - 2147483296, [P, B, B]),
            4294967: (REC_TRIP - 296, [P, B, B]), 4294968: (REC_TRIP + 704, [B, B, P]),
            2147483647: (REC_TRIP - 1000, [P, B, B])}
    return {r: want[tw] for r, tw in enumerate(RECOVERY_MS)}


def recovery_observed(c, status, read_breaker):
    """The same shape from a run: the entries' verdicts, and next_retry_ms read
    back (it still holds the trip's value: no later event re-opens)."""
    out = {}
    for r in range(len(RECOVERY_MS)):
        sel = np.nonzero((c["full"].res_id == r) & (c["full"].ts_ms > REC_TRIP))[0]
        out[r] = (int(read_breaker(r)), [int(x) for x in status[sel]])
    return out
