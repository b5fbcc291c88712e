"""Workloads that put ParamFlow traffic on the borders of ParamFlowChecker
(passDefaultLocalCheck :139-219, passThrottleLocalCheck :222-273), of the value
identity, of the wavefront-by-value walk's 64-event groups and of the exact
table, and emit each of them in the routing contexts that change only which of
the engine's three restatements decides it:

  lane     <= 32 events of the resource per batch (the stream cut into more
           batches): decide_segment, one lane
  wave     one batch, > 32 events, ParamFlow-only, no exits, no collections:
           SM_PARAM, heavy_param / param_run_rule by value
  generic  the same batch with a never-blocking FlowRule on the resource:
           SM_GENERIC, decide_segment by a wavefront's leader
  xflow    the resource in a RELATE group with a never-blocking rule: the
           second copy of the loop in sf_xflow.h

(heavy_min_events is 32 in every case, so a longer segment is always heavy.)

A case is a list of scenarios: one resource, its rules and hot items, and
occurrences (time, value, acquireCount, expectation).  The expectation is the
DESIGNED outcome on its border ("P" pass, "B" block, an int: pass with that
wait, ("B", wait): blocked after that wait); the guards compare it with the
ORACLE's verdicts, so a case that drifts off its border fails its guard
whatever the engine does.  Every case ends with a tail batch: for each
touched value of a default rule TAIL entries of acquireCount 1 at the last
timestamp, which makes the (rule, value) slot visible in verdicts (the engine
has no reader for it); guard_tail ties their passes to OracleEngine.read_param.

Shared by tests/test_param_cases.py (host build, guards, drift test) and
tests/test_gpu_param_cases.py (the engine, routing, table and thread guards).
"""
import os
import re

import numpy as np

from sentinel_amd import abi, trace

T0 = trace.T0
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sentinel_amd", "csrc")
CONTEXTS = ("lane", "wave", "generic", "xflow")
PARAM_MIN = 32                       # k_classify: a longer ParamFlow-only segment is SM_PARAM
SM_GENERIC, SM_PARAM = 1, 7
TAIL = 8
NEVER = 1e9                          # count of the never-blocking flow rules
L, I, S = abi.TAG_LONG, abi.TAG_INT, abi.TAG_STRING
FILL = 0x7F00_0000_0000              # filler values: distinct, never a scenario's value
HOUR = 3_600_000
BLOCKED = "blocked"                  # occurrence flagged SF_EV_BLOCKED by the caller


def D(count, burst=0, dur=1, items=(), idx=0):
    return dict(behavior=0, count=count, burst=burst, dur=dur, queue=0, items=list(items), idx=idx)


def Th(count, queue, dur=1, items=(), idx=0):
    return dict(behavior=2, count=count, burst=0, dur=dur, queue=queue, items=list(items), idx=idx)


class Scn:
    """One resource: rules (load order), occurrences (t, value, acq, expect, nargs)."""

    def __init__(self, name, rules, occ=(), pad=PARAM_MIN + 8):
        self.name, self.rules, self.occ, self.pad = name, list(rules), [], pad
        for o in occ:
            self.add(*o)

    def add(self, t, value, acq=1, expect=None, nargs=1):
        self.occ.append((int(t), value, int(acq), expect, int(nargs)))
        return self


def one(name, rules, value, seq, **kw):
    """Scenario of one value: seq = [(t, acq, expect)]."""
    return Scn(name, rules, [(t, value, a, e) for t, a, e in seq], **kw)


# ---------------------------------------------------------------- emit
def build(name, scns, capacity=1 << 12, tail=True):
    """The logical case: events of all scenarios merged in time order (stable:
    a scenario's occurrences keep their order), fillers of distinct values in
    front of a scenario shorter than its pad."""
    rows = []                                       # (t, seq, res, tag, bits, acq, nargs, flags, expect)
    for r, s in enumerate(scns):
        # epochs: occurrences more than an hour apart go to different batches (batch_cuts), each padded
        occ, start = [], 0
        for k in range(1, len(s.occ) + 1):
            if k == len(s.occ) or s.occ[k][0] - s.occ[k - 1][0] > HOUR:
                ep = s.occ[start:k]
                occ += [(ep[0][0], (L, FILL + (r << 16) + len(occ) + j), 1, None, 1)
                        for j in range(max(0, s.pad - len(ep)))] + ep
                start = k
        for k, (t, v, acq, ex, na) in enumerate(occ):
            fl = abi.EV_IN
            if ex == BLOCKED:
                fl |= abi.EV_BLOCKED
            tag, bits = (abi.TAG_NULL, 0) if v is None else v
            rows.append((t, len(rows), r, tag, bits, acq, na, fl, ex))
    rows.sort(key=lambda x: (x[0], x[1]))
    return dict(name=name, scns=scns, rows=rows, capacity=capacity, tail=tail)


def _batch(rows):
    n = len(rows)
    return abi.HostBatch(np.array([x[2] for x in rows], np.uint32), np.array([T0 + x[0] for x in rows], np.int64),
                         np.array([x[5] for x in rows], np.int32), np.array([x[7] for x in rows], np.uint8),
                         arg_tag=np.array([x[3] for x in rows], np.uint8).reshape(1, n),
                         arg_bits=np.array([x[4] for x in rows], np.uint64).reshape(1, n),
                         n_args=np.array([x[6] for x in rows], np.uint8))


def batch_cuts(rows, lane):
    """Cuts at every gap of more than an hour (a segment that spans more than
    65,536 bucket windows is never SM_PARAM) and, for the lane context, greedy
    cuts that leave every resource at most PARAM_MIN events per batch."""
    cuts, seen = [0], {}
    for k, x in enumerate(rows):
        if (lane and seen.get(x[2], 0) == PARAM_MIN) or (k and x[0] - rows[k - 1][0] > HOUR):
            cuts.append(k)
            seen = {}
        seen[x[2]] = seen.get(x[2], 0) + 1
    return cuts + [len(rows)]


def tail_rows(case):
    """TAIL entries of acquireCount 1 per touched (resource, value) at the last timestamp."""
    rows = case["rows"]
    t_last = max(x[0] for x in rows)
    seen, out = set(), []
    for x in rows:
        key = (x[2], x[3], x[4])
        if x[3] == abi.TAG_NULL or x[4] >= FILL and x[4] < FILL << 1 or key in seen or x[6] == 0:
            continue
        seen.add(key)
        out += [(t_last, 0, x[2], x[3], x[4], 1, 1, abi.EV_IN, None)] * TAIL
    return out


def emit(case, ctx):
    """The workload of one context (for workloads.run).  w["main"]: how many of
    its batches hold the case itself (the tail batch follows)."""
    scns, rows = case["scns"], case["rows"]
    R = len(scns)
    prules, items = [], []
    for r, s in enumerate(scns):
        for d in s.rules:
            off = len(items)
            items += [abi.sf_hot_item(tag=t, count=c, bits=b) for (t, b), c in d["items"]]
            prules.append(abi.sf_param_rule(resource=r, grade=abi.GRADE_QPS, param_idx=d["idx"],
                                            control_behavior=d["behavior"], count=float(d["count"]),
                                            max_queueing_time_ms=d["queue"], burst_count=d["burst"],
                                            duration_in_sec=d["dur"], item_offset=off, item_count=len(d["items"])))
    flow = []
    if ctx == "generic":
        flow = [abi.sf_flow_rule(resource=r, grade=abi.GRADE_QPS, count=NEVER, strategy=0, control_behavior=0,
                                 warm_up_period_sec=10, max_queueing_time_ms=500) for r in range(R)]
    elif ctx == "xflow":
        flow = [abi.sf_flow_rule(resource=r, grade=abi.GRADE_QPS, count=NEVER, strategy=abi.STRATEGY_RELATE,
                                 ref_resource=R, control_behavior=0, warm_up_period_sec=10, max_queueing_time_ms=500)
                for r in range(R)]
    cuts = batch_cuts(rows, ctx == "lane")
    batches = [_batch(rows[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    main = len(batches)
    tr = tail_rows(case) if case["tail"] else []
    if tr:
        batches.append(_batch(tr))
    mode = {"wave": SM_PARAM, "generic": SM_GENERIC}.get(ctx)
    modes = []                                      # per main batch: {resource: (events, mode)} of its heavy segments
    for b in batches[:main]:
        lens = np.bincount(b.res_id, minlength=R)
        modes.append({r: (int(lens[r]), mode) for r in range(R) if mode and lens[r] > PARAM_MIN and scns[r].rules})
    cfg = abi.default_config(max_resources=R + (ctx == "xflow"), max_batch=max(b.n for b in batches),
                             heavy_min_events=PARAM_MIN, param_capacity=case["capacity"])
    return dict(cfg=cfg, flow=flow, param=prules, items=items, batches=batches, nodes=list(range(R)), n_flow=len(flow),
                main=main, modes=modes, ctx=ctx, touched=sorted({(x[2], x[3], x[4]) for x in rows if x[3] != abi.TAG_NULL
                                                                 and x[6] > 0}))


# ---------------------------------------------------------------- guards
def oracle_run(so, w, upto=None):
    """The oracle over the workload's batches (the first ``upto`` events of
    the first batch only, when given): (engine, status, wait, rule)."""
    ora = so.OracleEngine(w["cfg"])
    if w["flow"]:
        ora.load_flow_rules(list(w["flow"]))
    ora.load_param_rules(list(w["param"]), list(w["items"]))
    bs = w["batches"] if upto is None else ([w["batches"][0].subset(0, upto)] if upto else [])
    outs = [ora.submit(b) for b in bs]
    cat = lambda f: np.concatenate([f(o) for o in outs]) if outs else np.zeros(0)  # noqa: E731
    return ora, cat(lambda o: o.status), cat(lambda o: o.wait_ms), cat(lambda o: o.rule_idx)


def expect_of(ex):
    """(status, wait) designed for an occurrence; None: not pinned."""
    if ex is None:
        return None
    if ex == BLOCKED:
        return abi.V_BLOCK_OTHER, 0
    if ex == "P":
        return abi.V_PASS, 0
    if ex == "B":
        return abi.V_BLOCK_PARAM, 0
    if isinstance(ex, tuple):
        return abi.V_BLOCK_PARAM, ex[1]
    return (abi.V_PASS_WAIT, ex) if ex > 0 else (abi.V_PASS, 0)


def guard_expect(case, st, wait):
    """Every pinned occurrence has the designed verdict in the oracle: the
    case sits on its borders, each decided the designed way."""
    pinned = 0
    for k, x in enumerate(case["rows"]):
        want = expect_of(x[8])
        if want is None:
            continue
        got = (int(st[k]), int(wait[k]))
        assert got == want, (case["name"], case["scns"][x[2]].name, x[:7], got, want)
        pinned += 1
    return pinned


def rule_index(case, r, k):
    return sum(len(s.rules) for s in case["scns"][:r]) + k


def guard_tail(so, case, w):
    """The tail entries the oracle passes per (resource, value) equal the
    tokens read_param reported before the tail, for resources with one default
    rule and no refill due (else the tail is compared for parity only)."""
    ora = so.OracleEngine(w["cfg"])
    ora.load_param_rules(list(w["param"]), list(w["items"]))
    for b in w["batches"][:-1]:
        ora.submit(b)
    tb = w["batches"][-1]
    t_last = int(tb.ts_ms[0])
    want = {}
    for r, tag, bits in {(int(a), int(b), int(c)) for a, b, c in zip(tb.res_id, tb.arg_tag[0], tb.arg_bits[0])}:
        rules = case["scns"][r].rules
        if len(rules) != 1 or rules[0]["behavior"] != 0:
            continue
        present, last_add, tokens = ora.read_param(rule_index(case, r, 0), (tag, bits))
        if present and tokens is not None and t_last - last_add <= rules[0]["dur"] * 1000:
            want[(r, tag, bits)] = min(max(tokens, 0), TAIL)
    out = ora.submit(tb)
    ora.close()
    for (r, tag, bits), n in want.items():
        sel = (tb.res_id == r) & (tb.arg_tag[0] == tag) & (tb.arg_bits[0] == np.uint64(bits))
        got = int(np.isin(out.status[sel], abi.PASSED).sum())
        assert got == n, (case["name"], r, tag, bits, got, n)
    return len(want)


def state_before(so, case, r, k_rule, value, row):
    """read_param of (rule, value) in a fresh oracle fed the rows before ``row``."""
    w = emit(case, "wave")
    ora, *_ = oracle_run(so, w, upto=row)
    got = ora.read_param(rule_index(case, r, k_rule), value)
    ora.close()
    return got


def guard_refill_border(so, case):
    """Scenarios named refill_d<dur>: their value meets the no-refill
    occurrence with now - lastAdd == duration * 1000 and the refill one
    millisecond later (read_param before each)."""
    hit = 0
    for r, s in enumerate(case["scns"]):
        if not s.name.startswith("refill_d"):
            continue
        dur = s.rules[0]["dur"]
        rows = [(k, x) for k, x in enumerate(case["rows"]) if x[2] == r and x[4] < FILL]
        (ka, xa), (kb, xb) = rows[-2], rows[-1]
        for k, x, gap in ((ka, xa, dur * 1000), (kb, xb, dur * 1000 + 1)):
            present, last_add, tokens = state_before(so, case, r, 0, (x[3], x[4]), k)
            assert present and T0 + x[0] - last_add == gap and tokens == 0, (s.name, x, last_add, tokens)
        hit += 1
    return hit


# ---------------------------------------------------------------- a. token bucket
V = (L, 77)
WEEKS = 14 * 24 * 3600 * 1000
BIG = float(2 ** 40)


def family_a():
    hot = lambda v, c: [(v, c)]  # noqa: E731
    s = [
        one("refill_d1", [D(3)], V, [(0, 1, "P"), (0, 1, "P"), (0, 1, "P"), (1000, 1, "B"), (1001, 1, "P")]),
        one("refill_d3", [D(3, dur=3)], V, [(0, 3, "P"), (3000, 1, "B"), (3001, 1, "P")]),
        # toAdd = passTime * 3 / (dur * 1000): 3 at 1333 / 3999 (newQps 0 + 3 - 4 = -1), 4 at 1334 / 4000
        # (rest + toAdd == maxCount, newQps 0)
        one("toadd_d1", [D(3, burst=1)], V, [(0, 4, "P"), (1333, 4, "B"), (1334, 4, "P"), (1334, 1, "B")]),
        one("toadd_d3", [D(3, burst=1, dur=3)], V, [(0, 4, "P"), (3999, 4, "B"), (4000, 4, "P"), (4000, 1, "B")]),
        # rest 1 + toAdd 4 == maxCount + 1: newQps = maxCount - acquireCount
        one("over_max", [D(3, burst=1)], V, [(0, 3, "P"), (1334, 4, "P"), (1334, 1, "B")]),
        one("acq_max", [D(2, burst=3)], V, [(0, 6, "B"), (0, 5, "P"), (0, 1, "B"), (1001, 6, "B"), (1001, 5, "B"),
                                            (1001, 2, "P"), (1001, 1, "B")]),
        # the packed word's count escape (1..255 inline, else the caller's array through the permutation)
        one("acq_255", [D(1, items=hot(V, 1000))], V,
            [(0, 255, "P"), (0, 256, "P"), (0, 256, "P"), (0, 255, "B"), (0, 256, "B"), (0, 233, "P"), (0, 1, "B")]),
        one("count_half", [D(0.5)], V, [(0, 1, "B"), (1500, 1, "B")]),
        one("count_1_9", [D(1.9)], V, [(0, 1, "P"), (0, 1, "B"), (1001, 1, "P")]),
        one("count_1e19", [D(1e19)], V, [(0, 1, "P"), (0, 255, "P"), (5, 2 ** 31 - 1, "P")]),
        # Long.MAX_VALUE + burst wraps negative: acquireCount > maxCount always
        one("count_1e19_burst", [D(1e19, burst=1)], V, [(0, 1, "B"), (1500, 1, "B")]),
        one("hot_zero", [D(5, items=hot(V, 0))], V, [(0, 1, "B"), (1200, 1, "B")]),
        one("hot_negative", [D(5, burst=3, items=hot(V, -2))], V, [(0, 1, "P"), (0, 1, "B"), (0, 2, "B")]),
        # the same bits under another tag are another value: the rule's count holds
        one("hot_other_tag", [D(2, items=hot((I, 77), 0))], V, [(0, 1, "P"), (0, 1, "P"), (0, 1, "B")]),
        one("hot_first_wins", [D(9, items=[(V, 1), (V, 5)])], V, [(0, 1, "P"), (0, 1, "B")]),
    ]
    return build("a_bucket", s)


def family_a_wmul():
    """passTime * tokenCount past 2^63 (count 2^40, gaps of weeks): Java's long
    multiply wraps, and toAdd is whatever the wrapped product gives."""
    s = [one("wmul", [D(BIG)], V, [(0, 1, "P"), (WEEKS, 1, None), (WEEKS + 1, 3, None), (2 * WEEKS, 1, None)]),
         one("wmul_burst", [D(BIG - 1, burst=7, dur=3)], V, [(0, 8, "P"), (WEEKS + 77, 2, None), (3 * WEEKS, 9, None)])]
    return build("a_wmul", s)


def family_a_invalid_counts():
    """count NaN and -1 (ParamFlowRuleUtil.isValidRule would refuse them; the
    engine decides what it is given: (long) NaN is 0, -1 + burst 2 is 1)."""
    s = [one("count_nan", [D(float("nan"))], V, [(0, 1, "B"), (1500, 1, "B")]),
         one("count_neg", [D(-1.0, burst=2)], V, [(0, 1, "P"), (0, 1, "B"), (0, 2, "B")])]
    return build("a_invalid_counts", s)


def guard_a(so, case, st, wait):
    assert guard_refill_border(so, case) == 2
    return {}


def guard_a_wmul(so, case, st, wait):
    for x in case["scns"]:
        assert x.occ[1][0] * int(x.rules[0]["count"]) >= 2 ** 63
    return {}


# ---------------------------------------------------------------- b. throttle
def family_b():
    eight = [(k // 8, 1) for k in range(40)]         # 40 entries of one value, eight per millisecond
    s = [
        # cost round(0.5) = 1: waits 1 .. 9 pass; expected - now == maxQueueingTimeMs blocks
        one("half_cost", [Th(2000, 10)], V, [(0, 1, "P")] + [(0, 1, k) for k in range(1, 10)] + [(0, 1, "B")] * 2
            + [(1, 1, 9), (1, 1, "B")]),
        one("cost_333", [Th(3, 500)], V, [(0, 1, "P"), (0, 1, 333), (0, 1, "B"), (167, 1, 499), (167, 1, "B")]),
        one("cost_0", [Th(1e15, 5)], V, [(0, 1, "P")] * 6 + [(3, 255, "P")]),
        one("queue_0", [Th(10, 0)], V, [(0, 1, "P"), (50, 1, "B"), (99, 1, "B"), (100, 1, "P"), (100, 1, "B")]),
        one("hot_negative", [Th(10, 0, items=[(V, -5)])], V, [(0, 1, "P")] * 5 + [(7, 3, "P")]),
        one("two_throttles", [Th(10, 500), Th(5, 500)], V,
            [(0, 1, "P"), (0, 1, 300), (0, 1, 600), (0, 1, ("B", 300)), (50, 1, ("B", 350)), (150, 1, 800)]),
        # a throttle rule with a positive wait, then a default rule that blocks: the thread has
        # slept in passThrottleLocalCheck before the next rule refuses it
        one("throttle_first", [Th(10, 500), D(2)], V,
            [(t, a, e) for (t, a), e in zip(eight, ["P", 100, ("B", 200), ("B", 300), ("B", 400), "B", "B", "B"]
                                            + [None] * 32)]),
        one("default_first", [D(2), Th(10, 500)], V,
            [(t, a, e) for (t, a), e in zip(eight, ["P", 100] + ["B"] * 38)]),
    ]
    return build("b_throttle", s)


def guard_b(so, case, st, wait):
    rows = case["rows"]
    r = [k for k, s in enumerate(case["scns"]) if s.name == "throttle_first"][0]
    sel = np.array([x[2] == r and x[4] < FILL for x in rows])
    n = len(rows)
    late = (st[:n][sel] == abi.V_BLOCK_PARAM) & (wait[:n][sel] > 0)
    assert late.sum() >= 3, "blocked entries with an accumulated wait"
    return dict(blocked_after_wait=int(late.sum()))


# ---------------------------------------------------------------- c. value identity
def family_c():
    lo, hi32, top = (L, 5), (L, 5 | 1 << 32), (L, 5 | 1 << 63)
    vals = [lo, hi32, top, (L, 0), (L, 2 ** 64 - 1), (I, 9), (L, 9), (S, 9), (L, 4), (L, 6)]

    def ident(name):
        s = Scn(name, [D(2)], pad=0)
        for rep, ex in enumerate(("P", "P", "B")):
            for v in vals:
                s.add(rep, v, 1, ex)
            s.add(rep, None, 1, "P")                         # a null value skips every rule
            s.add(rep, lo, 1, "P", nargs=0)                  # n_args <= paramIdx: no value
        return s
    # (each round is 12 events: the three rounds of a value sit in one 64-event group)
    return build("c_identity", [ident("first"), ident("neighbour"),
                                one("two_rules", [D(3), D(2)], lo, [(0, 1, "P"), (0, 1, "P"), (0, 1, "B"), (0, 1, "B")]),
                                ident("last_id")])


def guard_c(so, case, st, wait):
    rows = case["rows"]
    bits = {x[4] for x in rows if x[2] == 0}
    assert {5, 5 | 1 << 32, 5 | 1 << 63, 0, 2 ** 64 - 1} <= bits
    assert {x[3] for x in rows if x[4] == 9} == {I, L, S}
    return {}


def no_arg_slots():
    """A batch without argument arrays (arg_slots 0) on a param resource: every entry passes."""
    n = PARAM_MIN + 8
    b = abi.HostBatch(np.zeros(n, np.uint32), T0 + np.arange(n, dtype=np.int64) // 8, np.ones(n, np.int32),
                      np.full(n, abi.EV_IN, np.uint8))
    pr = [abi.sf_param_rule(resource=0, grade=abi.GRADE_QPS, param_idx=0, control_behavior=0, count=1.0,
                            max_queueing_time_ms=0, burst_count=0, duration_in_sec=1, item_offset=0, item_count=0)]
    return dict(cfg=abi.default_config(max_resources=1, max_batch=n, heavy_min_events=PARAM_MIN, param_capacity=1 << 12),
                flow=[], param=pr, items=[], batches=[b], nodes=[0], n_flow=0, main=1, modes={0: (n, SM_PARAM)},
                ctx="wave", touched=[])


# ---------------------------------------------------------------- d. wave-group borders
GROUP_LENGTHS = (64, 65, 63, 127, 33, 128, 129)     # starts 0, 64, 129, 192, 319, 352, 480
HOT = (L, 3)


def family_d(seed=91):
    """Segments of 33 .. 129 events starting at sorted positions 0, 1 and 63
    mod 64 (the fourth and fifth share a passbits word), three rules on the
    index (default, throttle, default with a hot item: the blocking rule
    differs by occurrence), six values over 2.5 s (refills in later groups than
    the first sight), caller-blocked and null-valued entries interleaved; then
    64 distinct values in one group, 64 copies of one value whose bucket empties
    in mid-group, a segment of caller-blocked entries only, and a value first
    seen in one group and refilled in the next."""
    rng = np.random.default_rng(seed)
    scns = []
    for n in GROUP_LENGTHS:
        s = Scn(f"len{n}", [D(4), Th(50, 30), D(2, burst=1, items=[(HOT, 6)])], pad=0)
        ts = np.sort(rng.integers(0, 2500, n))
        for t in ts:
            u = rng.random()
            v = None if u < 0.1 else (L, int(rng.integers(1, 7)))
            s.add(t, v, int(rng.integers(1, 3)), BLOCKED if 0.1 <= u < 0.2 else None)
        scns.append(s)
    scns.append(Scn("distinct64", [D(1)], [(k // 32, (L, 1000 + k), 1, "P") for k in range(64)], pad=0))
    scns.append(Scn("copies64", [D(40)], [(0, V, 1, "P" if k < 40 else "B") for k in range(64)], pad=0))
    scns.append(Scn("all_blocked", [D(1)], [(k // 8, V, 1, BLOCKED) for k in range(PARAM_MIN + 8)], pad=0))
    # first sight in the first group, the refill (event 65) in the second
    scns.append(Scn("late_refill", [D(2)], [(0, V, 1, "P"), (0, V, 1, "P"), (0, V, 1, "B")]
                    + [(1, (L, 2000 + k), 1, "P") for k in range(62)] + [(1001, V, 1, "P"), (1001, V, 2, "B")], pad=0))
    return build("d_groups", scns)


def guard_d(so, case, st, wait):
    rows = case["rows"]
    lens = np.bincount([x[2] for x in rows])
    by_name = {s.name: int(lens[r]) for r, s in enumerate(case["scns"])}
    assert tuple(int(x) for x in lens[:len(GROUP_LENGTHS)]) == GROUP_LENGTHS
    assert by_name["distinct64"] == 64 and by_name["copies64"] == 64 and by_name["late_refill"] == 67
    late = [x for x in rows if case["scns"][x[2]].name == "late_refill"]
    assert late[65][:5] == (1001, late[65][1], late[65][2], L, 77), "the refill sits in the second 64-event group"
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    assert {0, 1, 63} <= {int(x) % 64 for x in starts[:len(GROUP_LENGTHS)]}
    assert any(a // 64 == (a - 1) // 64 for a in starts[1:len(GROUP_LENGTHS)]), "two segments in one passbits word"
    assert {n % 64 for n in GROUP_LENGTHS} >= {0, 1, 63} and 65 in GROUP_LENGTHS     # a tail group of one lane
    ora, _, _, rule = oracle_run(so, emit(case, "wave"))
    ora.close()
    res = np.array([x[2] for x in rows])
    first = res < len(GROUP_LENGTHS)
    blk = st[:len(rows)] == abi.V_BLOCK_PARAM
    assert {int(x) for x in np.unique(rule[:len(rows)][first & blk])} == {0, 1, 2}, "each rule blocks somewhere"
    assert (st[:len(rows)][first] == abi.V_PASS_WAIT).any() and (st[:len(rows)][first] == abi.V_BLOCK_OTHER).any()
    return dict(starts=[int(x) % 64 for x in starts])


# ---------------------------------------------------------------- e. handover between walks
HAND = ("lane", "wave", "exit", "coll", "wave")
HAND_MODES = (None, SM_PARAM, SM_GENERIC, SM_GENERIC, SM_PARAM)


def handover():
    """One resource (default rule 30 / s, then a throttle) over five batches,
    400 ms apart, each decided by another walk: lane (20 events), wave (48),
    generic by an exit in the segment (the exits of the second batch's first
    entries: the thread counts the wave walk added at once come off one at a
    time), generic by a collection argument, wave.  Three values recur."""
    vals = [(L, 1), (L, 2), (S, 1)]
    coll = [(L, 1), (L, 2)]
    batches = []
    for k, kind in enumerate(HAND):
        n = 20 if kind == "lane" else 48
        t = T0 + 400 * k + np.arange(n, dtype=np.int64) // 4
        values = [[vals[i % 3] for i in range(n)]]
        if kind == "coll":
            values[0][7] = coll
        fl = np.full(n, abi.EV_IN, np.uint8)
        eref = np.full(n, -1, np.int64)
        cts = np.zeros(n, np.int64)
        if kind == "exit":
            # the first nine events of this batch are exits of entries of the batch before
            # (entry_ref -1: alive, created then), carrying their entry's argument
            fl[:9] |= abi.EV_EXIT
            cts[:9] = T0 + 400 * (k - 1) + np.arange(9) // 4
        at, ab, off, et, eb = abi.HostBatch.collections(1, n, values)
        batches.append(abi.HostBatch(np.zeros(n, np.uint32), t, np.ones(n, np.int32), fl, entry_ref=eref, create_ts=cts,
                                     arg_tag=at, arg_bits=ab, n_args=np.ones(n, np.uint8),
                                     **(dict(elem_off=off, elem_tag=et, elem_bits=eb) if kind == "coll" else {})))
    pr = [abi.sf_param_rule(resource=0, grade=abi.GRADE_QPS, param_idx=0, control_behavior=0, count=30.0,
                            max_queueing_time_ms=0, burst_count=0, duration_in_sec=1, item_offset=0, item_count=0),
          abi.sf_param_rule(resource=0, grade=abi.GRADE_QPS, param_idx=0, control_behavior=2, count=400.0,
                            max_queueing_time_ms=20, burst_count=0, duration_in_sec=1, item_offset=0, item_count=0)]
    return dict(cfg=abi.default_config(max_resources=1, max_batch=48, heavy_min_events=PARAM_MIN, param_capacity=1 << 12),
                flow=[], param=pr, items=[], batches=batches, nodes=[0], n_flow=0, main=len(batches), ctx="handover",
                modes=None, touched=[(0, t, b) for t, b in vals])


def guard_handover(so, w):
    ora, st, wait, _ = oracle_run(so, w)
    th = [ora.param_thread(0, 0, v[1:]) for v in w["touched"]]
    ora.close()
    assert (st == abi.V_EXIT).sum() == 9 and (st == abi.V_BLOCK_PARAM).any() and (st == abi.V_PASS_WAIT).any()
    n0 = w["batches"][0].n
    assert np.isin(st[n0:n0 + 48], abi.PASSED).sum() > 9, "the wave batch passes more than the exits take off"
    return dict(threads=th)


# ---------------------------------------------------------------- f. table borders
def growth():
    """param_capacity 16 and five batches of 40 events with new keys each: the
    table is rebuilt before most batches; a bucket drained half-way (value 1,
    count 5, three tokens taken in the first batch, the rest in the last) and
    a throttle timestamp (rule 1) must survive the rebuilds."""
    batches = []
    for k in range(5):
        n = 40
        bits = np.array([1 if i in (0, 1, 2) else 100 + 40 * k + i for i in range(n)], np.uint64)
        if k in (1, 2, 3):
            bits[:3] = 100 + 40 * k + np.arange(3)
        batches.append(abi.HostBatch(np.zeros(n, np.uint32), np.full(n, T0 + 10 * k, np.int64), np.ones(n, np.int32),
                                     np.full(n, abi.EV_IN, np.uint8), arg_tag=np.full((1, n), L, np.uint8),
                                     arg_bits=bits.reshape(1, n), n_args=np.ones(n, np.uint8)))
    pr = [abi.sf_param_rule(resource=0, grade=abi.GRADE_QPS, param_idx=0, control_behavior=0, count=5.0,
                            max_queueing_time_ms=0, burst_count=0, duration_in_sec=1, item_offset=0, item_count=0),
          abi.sf_param_rule(resource=0, grade=abi.GRADE_QPS, param_idx=0, control_behavior=2, count=100.0,
                            max_queueing_time_ms=100, burst_count=0, duration_in_sec=1, item_offset=0, item_count=0)]
    return dict(cfg=abi.default_config(max_resources=1, max_batch=40, heavy_min_events=PARAM_MIN, param_capacity=16),
                host_capacity=1 << 12, flow=[], param=pr, items=[], batches=batches, nodes=[0], n_flow=0, main=5,
                ctx="wave", modes={0: (40, SM_PARAM)}, touched=[(0, L, 1)])


def guard_growth(so, w):
    ora, st, wait, _ = oracle_run(so, w)
    ora.close()
    last = st[-40:]
    # bucket 5 - 3 = 2 left; the throttle's latestPassedTime T0 + 20, cost 10, now T0 + 40
    assert list(last[:3]) == [abi.V_PASS, abi.V_PASS_WAIT, abi.V_BLOCK_PARAM], last[:3]
    assert list(wait[-40:][:3]) == [0, 10, 0], wait[-40:][:3]
    return {}


MIX = np.uint64(0x9e3779b97f4a7c15)
PK_RULE = 1
WRAP_CAP, WRAP_LAST, WRAP_VALUES = 1 << 12, 4, 48


def pkey_hi(res, kind, idx, tag):
    """sf_decide.h pkey_hi, restated."""
    return ((res + 1) << 32) | (kind << 24) | ((idx & 0xffff) << 8) | (tag & 0xff)


def table_hash(hi, lo):
    """ParamTable::hash, restated on trace.mix64 (uint64 arrays)."""
    with np.errstate(over="ignore"):
        return trace.mix64(np.uint64(hi) ^ trace.mix64(np.asarray(lo, np.uint64) + MIX))


def wrap_values():
    """The first WRAP_VALUES longs whose (rule 0, value) key of resource 0 has
    its home in the last WRAP_LAST slots of a WRAP_CAP table."""
    cand = np.arange(1, 200_000, dtype=np.uint64)
    home = table_hash(pkey_hi(0, PK_RULE, 0, L), cand) & np.uint64(WRAP_CAP - 1)
    vals = cand[home >= WRAP_CAP - WRAP_LAST][:WRAP_VALUES]
    assert vals.size == WRAP_VALUES
    return vals


def table_wrap():
    """48 values homed in the last four slots, all in one 64-event group of
    an SM_PARAM segment: the lanes' CAS inserts collide and the chain wraps to
    slot 0; a second batch finds every one of them again."""
    vals = wrap_values()
    n = 64
    bits = np.concatenate([vals, vals[:n - vals.size]])
    mk = lambda t: abi.HostBatch(np.zeros(n, np.uint32), np.full(n, t, np.int64), np.ones(n, np.int32),  # noqa: E731
                                 np.full(n, abi.EV_IN, np.uint8), arg_tag=np.full((1, n), L, np.uint8),
                                 arg_bits=bits.reshape(1, n), n_args=np.ones(n, np.uint8))
    pr = [abi.sf_param_rule(resource=0, grade=abi.GRADE_QPS, param_idx=0, control_behavior=0, count=3.0,
                            max_queueing_time_ms=0, burst_count=0, duration_in_sec=1, item_offset=0, item_count=0)]
    return dict(cfg=abi.default_config(max_resources=1, max_batch=n, heavy_min_events=PARAM_MIN, param_capacity=WRAP_CAP),
                flow=[], param=pr, items=[], batches=[mk(T0), mk(T0 + 5)], nodes=[0], n_flow=0, main=2, ctx="wave",
                modes={0: (n, SM_PARAM)}, touched=[(0, L, int(v)) for v in vals[:4]],
                # the cluster's last key lies at least this far from its home; rule and thread keys
                min_probe=WRAP_VALUES - WRAP_LAST, used=2 * WRAP_VALUES)


def guard_table_wrap(so, w):
    ora, st, wait, _ = oracle_run(so, w)
    ora.close()
    # 16 values occur twice per batch: tokens 3 -> second batch blocks their last occurrence
    assert (st[:64] == abi.V_PASS).all() and (st[64:] == abi.V_BLOCK_PARAM).sum() == 16
    return {}


def source_lines():
    """The hash, key packing and probing lines the wrap case restates, read
    from sf_decide.h / sf_internal.h as text: a retune fails the drift test."""
    def text(name):
        with open(os.path.join(_CSRC, name)) as f:
            return f.read()
    dec, internal, kern = text("sf_decide.h"), text("sf_internal.h"), text("sf_segs.hip")

    def one_(src, pat):
        m = re.findall(pat, src)
        assert len(m) == 1, (pat, m)
        return m[0]
    one_(dec, r"(SF_HD static uint64_t hash\(uint64_t hi, uint64_t lo\) \{ return mix64\(hi \^ mix64\(lo \+ "
              r"0x9e3779b97f4a7c15ULL\)\); \})")
    one_(dec, r"(return \(\(uint64_t\)\(res \+ 1u\) << 32\) \| \(kind << 24\) \| \(\(uint64_t\)\(idx & 0xffff\) << 8\) \| "
              r"\(tag & 0xff\);)")
    one_(dec, r"(x \^= x >> 33; x \*= 0xff51afd7ed558ccdULL; x \^= x >> 33;\n\s*x \*= 0xc4ceb9fe1a85ec53ULL; x \^= x >> 33; "
              r"return x;)")
    assert len(re.findall(r"i = \(i \+ 1\) & mask;", dec)) == 2             # find and insert probe linearly, wrapping
    return dict(PK_RULE=int(one_(internal, r"constexpr uint64_t PK_RULE = (\d+), PK_THREAD = \d+;")),
                PARAM_MIN=int(one_(kern, r"if \(light && hi - lo > (\d+) && \(st\.rdesc\[res\]\.flags & RD_PRULE\)")))


# ---------------------------------------------------------------- g. param_inert
def inert(seed=97):
    """A QPS SystemRule (150 / s) over 1.4 s of entries on a resource whose
    first rule blocks some of them for certain -- a hot item of 0 (value 1),
    acquireCount 40 > maxCount 3, an empty bucket with no refill due (values 2
    to 4) -- which the planner treats as inert (sf_system.h param_inert); most
    other entries bring a fresh value and pass.  From 111 passes on the
    SystemRule refuses the entries of acquireCount 40, from 150 on every
    entry, until the first half-second bucket leaves the window at 1000 ms.
    Value 9's bucket is emptied at 0 ms and met again at exactly 1000 ms (no
    refill due: inert) and at 1001 ms (a refill is due: not inert)."""
    rng = np.random.default_rng(seed)

    def traffic(n, t0, t1, base):
        u = rng.random(n)
        bits = np.where(u < 0.6, base + np.arange(n), np.where(u < 0.75, 1, rng.integers(2, 5, n))).astype(np.uint64)
        cnt = np.where(rng.random(n) < 0.1, 40, 1).astype(np.int32)
        return np.sort(rng.integers(t0, t1, n)), bits, cnt
    parts = [(np.zeros(3, np.int64), np.full(3, 9, np.uint64), np.ones(3, np.int32)), traffic(600, 1, 1000, 1000),
             (np.array([1000, 1000, 1001, 1001]), np.array([9, 2, 9, 2], np.uint64), np.ones(4, np.int32)),
             traffic(200, 1002, 1400, 5000)]
    t = np.concatenate([p[0] for p in parts]).astype(np.int64)
    bits = np.concatenate([p[1] for p in parts]).astype(np.uint64)
    cnt = np.concatenate([p[2] for p in parts]).astype(np.int32)
    m = t.size
    b = abi.HostBatch(np.zeros(m, np.uint32), T0 + t, cnt, np.full(m, abi.EV_IN, np.uint8),
                      arg_tag=np.full((1, m), L, np.uint8), arg_bits=bits.reshape(1, m), n_args=np.ones(m, np.uint8))
    pr = [abi.sf_param_rule(resource=0, grade=abi.GRADE_QPS, param_idx=0, control_behavior=0, count=2.0,
                            max_queueing_time_ms=0, burst_count=1, duration_in_sec=1, item_offset=0, item_count=1)]
    items = [abi.sf_hot_item(tag=L, count=0, bits=1)]
    sysr = [abi.sf_system_rule(highest_system_load=-1, highest_cpu_usage=-1, qps=150.0, avg_rt=-1, max_thread=-1)]
    return dict(cfg=abi.default_config(max_resources=1, max_batch=m, heavy_min_events=PARAM_MIN, param_capacity=1 << 12),
                flow=[], param=pr, items=items, batches=[b], nodes=[0], n_flow=0, main=1, ctx="system", modes=None,
                touched=[(0, L, 9)], system=sysr, status=(0.0, 0.0), edge=603)


def guard_inert(so, w):
    ora = so.OracleEngine(w["cfg"])
    ora.set_system_status(*w["status"])
    ora.load_system_rules(list(w["system"]))
    ora.load_param_rules(list(w["param"]), list(w["items"]))
    st = ora.submit(w["batches"][0]).status
    ora.close()
    b = w["batches"][0]
    sysb = np.nonzero(st == abi.V_BLOCK_SYSTEM)[0]
    prm = np.zeros(b.n, bool)
    prm[sysb[0]:sysb[-1]] = True
    prm &= st == abi.V_BLOCK_PARAM
    assert sysb.size > 100 and prm.sum() > 10, "ParamFlow blocks between the SystemRule's blocks"
    bits = b.arg_bits[0]
    assert (prm & (bits == 1)).any() and (prm & (bits >= 2) & (bits <= 4) & (b.count == 1)).any()
    assert ((st == abi.V_BLOCK_PARAM) & (b.count == 40)).any() and ((st == abi.V_BLOCK_SYSTEM) & (b.count == 40)).any()
    assert np.isin(st[sysb[0]:sysb[-1]], abi.PASSED).any(), "passes between the SystemRule's blocks"
    e = w["edge"]
    assert [int(x) for x in b.ts_ms[e:e + 4] - T0] == [1000, 1000, 1001, 1001] and list(bits[e:e + 4]) == [9, 2, 9, 2]
    # no refill due at passTime == 1000 (inert), due at 1001; value 2's bucket (first seen after 1 ms) stays empty
    assert [int(x) for x in st[e:e + 4]] == [abi.V_BLOCK_PARAM, abi.V_BLOCK_PARAM, abi.V_PASS, abi.V_BLOCK_PARAM]
    return dict(system=int(sysb.size), param_inside=int(prm.sum()))


# ---------------------------------------------------------------- the cases
# name -> (builder of the logical case, guard(so, case, status, wait)); emitted in CONTEXTS
CASES = {
    "a_bucket": (family_a, guard_a),
    "a_invalid_counts": (family_a_invalid_counts, lambda so, case, st, wait: {}),
    "a_wmul": (family_a_wmul, guard_a_wmul),
    "b_throttle": (family_b, guard_b),
    "c_identity": (family_c, guard_c),
    "d_groups": (family_d, guard_d),
}
# name -> (builder of the workload, guard(so, w)): one routing of their own
SINGLE = {
    "no_arg_slots": (no_arg_slots, lambda so, w: {}),
    "handover": (handover, guard_handover),
    "growth": (growth, guard_growth),
    "table_wrap": (table_wrap, guard_table_wrap),
}
# the same, under a SystemRule (the host build has no planner: GPU only)
SYSTEM = {"inert": (inert, guard_inert)}
