"""Token-server scripts that sit on the hand-built borders of sf_request_tokens:
the 64-ary window search, the first-fail search and the strided scatter of
k_ns_limit, the namespace table next to NS_NONE, the ClusterMetric ring at
every geometry and gap, tryOccupyNext, the config factors, the per-value
columns (a full table, one slot claimed by thousands of lanes, every tag), the
serial route of Collection params, and degenerate calls.  Random traffic
(tests/test_gpu_token.py) reaches these only by chance.

A case is a Script: loads and calls in order.  play() runs it on any engine
(FlowEngine or OracleEngine) and records, per call, every request's status,
remaining and wait_ms, and cluster_sum of all 7 events of every flow rule at
the call's last timestamp, at last + I - 1 and at last + I.  cluster_sum rolls
the window like a request, so it is a call with a time of its own: a read
whose time lies after the next call's first request is left out (time never
runs backwards inside a script), and both engines are always read alike.

Hidden state (limiter buckets, value columns) has no read-out: every script
follows its main call with probe calls whose decisions depend on that state,
and its guard proves, from the ORACLE's answers alone, that the probe
separates two outcomes.

Shared by tests/test_token_wire_cases.py (CPU: guards and the constant-drift
check) and tests/test_gpu_token_wire_cases.py (the engine against the oracle).
"""
import os
import re

import numpy as np

from sentinel_amd import abi, trace

T0 = trace.T0
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sentinel_amd", "csrc")

# ---- the engine's constants, restated (test_token_constants_match_the_source) ----
LIM_S, LIM_WL, LIM_INTERVAL = 10, 100, 1000     # sf_token.h: RequestLimiter's UnaryLeapArray
CL_MAXS = 16                                    # sf_token.h: largest sample_count (array bound)
TD_T = 64                                       # sf_token.hip: segments per workgroup of k_tok_decide
NS_NONE = 0xFF                                  # sf_token.hip: namespace key of an unlimited request
PT_MAX_PROBE = 4096                             # sf_decide.h: probe reach of the value table
CP_MIN_SLOTS = 1024                             # sf_host_cluster.cpp tok_rebuild: smallest value table
NS_MAX = 255                                    # sf_host_cluster.cpp sf_load_namespaces
SEARCH_FAN = 64                                 # k_ns_limit: `e - a > 64`, step = (e - a + 63) / 64

MIRROR = dict(LIM=(LIM_S, LIM_WL, LIM_INTERVAL), CL_MAXS=CL_MAXS, TD_T=TD_T, NS_NONE=NS_NONE,
              PT_MAX_PROBE=PT_MAX_PROBE, CP_MIN_SLOTS=CP_MIN_SLOTS, NS_MAX=NS_MAX, SEARCH_FAN=SEARCH_FAN)


def source_constants(csrc=_CSRC):
    """The same constants, read from the source text."""
    def text(name):
        with open(os.path.join(csrc, name)) as f:
            return f.read()

    def one(src, pat):
        m = re.findall(pat, src)
        assert len(m) == 1, (pat, m)
        return m[0]
    tok_h, tok, dec, eng = text("sf_token.h"), text("sf_token.hip"), text("sf_decide.h"), text("sf_host_cluster.cpp")
    out = {}
    out["LIM"] = tuple(int(x) for x in one(
        tok_h, r"constexpr int LIM_S = (\d+), LIM_WL = (\d+), LIM_INTERVAL = (\d+);"))
    out["CL_MAXS"] = int(one(tok_h, r"constexpr int CL_MAXS = (\d+);"))
    out["TD_T"] = int(one(tok, r"constexpr int TD_T = (\d+);"))
    out["NS_NONE"] = int(one(tok, r"constexpr uint8_t NS_NONE = (0x[0-9a-f]+);"), 16)
    out["PT_MAX_PROBE"] = int(one(dec, r"constexpr uint64_t PT_MAX_PROBE = (\d+);"))
    a, b = one(eng, r"uint64_t pc = (\d+);\s*while \(pc < std::max<uint64_t>\(e->cfg\.param_capacity, (\d+)\)\) pc <<= 1;")
    assert a == b
    out["CP_MIN_SLOTS"] = int(a)
    out["NS_MAX"] = int(one(eng, r"if \(n > (\d+)\) return fail\(SF_ERR_UNSUPPORTED, \"at most 255 namespaces\"\);"))
    fan = one(tok, r"while \(e - a > (\d+)\) \{")
    f1, f2 = one(tok, r"const uint32_t step = \(e - a \+ (\d+)\) / (\d+);")
    assert int(f1) + 1 == int(f2) == int(fan)
    out["SEARCH_FAN"] = int(fan)
    # the compares and the probe reach the cases are built around
    one(tok, r"(const uint64_t reach = ts\.cp_mask < PT_MAX_PROBE \? ts\.cp_mask : PT_MAX_PROBE;)")
    one(tok, r"(if \(\(double\)wadd\(sum, \(int64_t\)mid\) / 1\.0 \+ 1 <= qps\) klo = mid \+ 1;)")
    one(tok, r"(for \(uint32_t j = p \+ K \+ \(uint32_t\)lane; j < bnd; j \+= 64\))")
    return out


OK, BLOCKED, WAIT, NO_RULE = abi.TOKEN_OK, abi.TOKEN_BLOCKED, abi.TOKEN_SHOULD_WAIT, abi.TOKEN_NO_RULE_EXISTS
BAD, TOO_MANY = abi.TOKEN_BAD_REQUEST, abi.TOKEN_TOO_MANY_REQUEST
GLOBAL, AVG_LOCAL = abi.THRESHOLD_GLOBAL, abi.THRESHOLD_AVG_LOCAL
CE_PASS, CE_BLOCK, CE_PASS_REQUEST, CE_BLOCK_REQUEST, CE_OCCUPIED_PASS, CE_OCCUPIED_BLOCK, CE_WAITING = range(7)
INT_MAX = 2 ** 31 - 1
WIRE_TAGS = (abi.TAG_INT, abi.TAG_LONG, abi.TAG_BYTE, abi.TAG_DOUBLE, abi.TAG_FLOAT, abi.TAG_SHORT, abi.TAG_BOOL,
             abi.TAG_STRING)
HUGE = 1e9          # a flow threshold that passes everything


def frule(fid, count, S=10, I=1000, tt=GLOBAL, ns=1):
    return abi.sf_cluster_flow_rule(flow_id=fid, count=float(count), threshold_type=tt, namespace_id=ns,
                                    sample_count=S, window_interval_ms=I)


def prule(fid, count, S=10, I=1000, tt=GLOBAL, ns=1, off=0, cnt=0):
    return abi.sf_cluster_param_rule(flow_id=fid, count=float(count), threshold_type=tt, namespace_id=ns,
                                     sample_count=S, window_interval_ms=I, item_offset=off, item_count=cnt)


def nsp(nid, connected=1, qps=-1.0):
    return abi.sf_namespace(namespace_id=nid, connected_count=connected, max_allowed_qps=float(qps))


def item(tag, bits, count):
    return abi.sf_hot_item(tag=tag, count=count, bits=bits)


def L(v):
    return (abi.TAG_LONG, v)


NULL = (abi.TAG_NULL, 0)


def align(t, I):
    """First multiple of I at or after t (bucket 0 of a LeapArray of interval I starts there)."""
    return (t + I - 1) // I * I


class Script:
    """Loads and calls in order; marks name the requests a guard reads."""

    def __init__(self, name, max_batch=4096, **cfg):
        self.name = name
        self.cfg = dict(max_resources=4, max_batch=max_batch, param_capacity=1 << 12, **cfg)
        self.steps = []
        self.marks = {}
        self.guard = None
        self.n_calls = 0
        self.read_ahead = True      # False: only the last call is followed by the reads at last + I - 1 and last + I
        self._cur = []

    def config(self):
        return abi.default_config(**self.cfg)

    def ns(self, *ns):
        self.steps.append(("ns", list(ns)))

    def rules(self, flow=(), param=(), items=()):
        self.steps.append(("rules", list(flow), list(param), list(items)))

    def req(self, t, fid, n=1, count=1, prio=False, vals=None, param=None, mark=None):
        """n equal requests at time t; vals: None for requestToken, a list of (tag, bits) for requestParamToken."""
        is_param = vals is not None if param is None else param
        fl = (abi.TOK_PRIORITIZED if prio else 0) | (abi.TOK_PARAM if is_param else 0)
        for _ in range(n):
            self._cur.append((int(t), int(fid), int(count), fl, vals, mark))

    def call(self, off=None, plain=False):
        """The requests gathered so far, stably sorted by time, as one call.  Values go through
        param_off when a request has another number of values than one (or off=True);
        plain=True passes no value arrays at all."""
        cur = sorted(self._cur, key=lambda r: r[0])
        self._cur = []
        n = len(cur)
        assert n
        vals = [r[4] if r[4] is not None else [] for r in cur]
        is_param = [bool(r[3] & abi.TOK_PARAM) for r in cur]
        use_off = off if off is not None else any(p and len(v) != 1 for p, v in zip(is_param, vals))
        arr = lambda k, dt: np.array([r[k] for r in cur], dt)
        if plain:
            tag = bits = po = None
        elif use_off:
            po = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.uint32)
            tag = np.array([t for v in vals for t, _ in v], np.uint8)
            bits = np.array([x for v in vals for _, x in v], np.uint64)
        else:
            po = None
            tag = np.array([v[0][0] if v else abi.TAG_NULL for v in vals], np.uint8)
            bits = np.array([v[0][1] if v else 0 for v in vals], np.uint64)
        b = abi.HostTokenBatch(arr(1, np.int64), arr(2, np.int32), arr(3, np.uint8), arr(0, np.int64),
                               param_tag=tag, param_bits=bits, param_off=po)
        k = self.n_calls
        self.n_calls += 1
        self.steps.append(("call", b))
        for i, r in enumerate(cur):
            if r[5] is not None:
                self.marks.setdefault(r[5], (k, []))[1].append(i)
        return k

    def big_req(self, ts, fid, mark=None):
        """One call of len(ts) plain requestToken calls of one flow id at the (sorted) times ts."""
        assert not self._cur
        ts = np.asarray(ts, np.int64)
        n = ts.size
        b = abi.HostTokenBatch(np.full(n, fid, np.int64), np.ones(n, np.int32), np.zeros(n, np.uint8), ts)
        k = self.n_calls
        self.n_calls += 1
        self.steps.append(("call", b))
        return k

    def calls(self):
        return [s[1] for s in self.steps if s[0] == "call"]


class CallResult:
    def __init__(self, r, sums):
        self.status, self.remaining, self.wait_ms, self.sums = r.status, r.remaining, r.wait_ms, sums


def play(eng, sc):
    """Run the script on one engine -> [CallResult].  sums: {(flow_id, t): (7 event sums)}."""
    out = []
    flow = []
    first_ts = [int(s[1].ts_ms[0]) if s[0] == "call" else None for s in sc.steps]
    for k, step in enumerate(sc.steps):
        if step[0] == "ns":
            eng.load_namespaces(step[1])
        elif step[0] == "rules":
            eng.load_cluster_rules(step[1], step[2], step[3])
            flow = []
            for f in step[1]:
                if f.flow_id > 0 and f.flow_id not in [x.flow_id for x in flow]:
                    flow.append(f)
        else:
            b = step[1]
            r = eng.request_tokens(b)
            last = int(b.ts_ms[-1])
            nxt = next((t for t in first_ts[k + 1:] if t is not None), None)
            sums = {}
            for dt in ("last", "I-1", "I"):
                for f in flow:
                    I = f.window_interval_ms
                    t = last + {"last": 0, "I-1": I - 1, "I": I}[dt]
                    if nxt is not None and (t > nxt or (dt != "last" and not sc.read_ahead)):
                        continue
                    sums[(f.flow_id, t)] = tuple(int(eng.cluster_sum(f.flow_id, ev, t)) for ev in range(7))
            out.append(CallResult(r, sums))
    return out


def compare(sc, got, want):
    """Every request of every call and every sum: engine == oracle."""
    assert len(got) == len(want) == sc.n_calls
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.nonzero((g.status != w.status) | (g.remaining != w.remaining) | (g.wait_ms != w.wait_ms))[0]
        if bad.size:
            i = int(bad[0])
            b = sc.calls()[k]
            raise AssertionError(
                f"{sc.name} call {k}: {bad.size} of {b.n} results differ; first at {i} (flow {b.flow_id[i]}, t "
                f"{b.ts_ms[i] - T0}): engine=({g.status[i]},{g.remaining[i]},{g.wait_ms[i]}) "
                f"oracle=({w.status[i]},{w.remaining[i]},{w.wait_ms[i]})")
        assert g.sums.keys() == w.sums.keys()
        for key in w.sums:
            assert g.sums[key] == w.sums[key], f"{sc.name} call {k}: cluster_sum{key}: engine {g.sums[key]} oracle {w.sums[key]}"


def check_times(sc):
    last = -1
    for b in sc.calls():
        assert np.all(np.diff(b.ts_ms) >= 0) and int(b.ts_ms[0]) >= last, sc.name
        last = int(b.ts_ms[-1])


def st(sc, R, mark):
    k, idx = sc.marks[mark]
    return [int(x) for x in R[k].status[idx]]


def count(sc, R, mark, what=OK):
    return st(sc, R, mark).count(what)


# ---------------------------------------------------------------- 1. ns_search
SEARCH_R = (1, 2, 63, 64, 65, 66, 128, 129, 4095, 4096, 4097, 4160, 4161, 8191, 262144, 262145)


def search_nw(R):
    step = -(-R // SEARCH_FAN)
    if R >= 262144:
        c = {1, step, R - 1, R}
    else:
        c = {1, 2, step - 1, step, step + 1, 63, 64, 65, R - step, R - 2, R - 1, R}
    return sorted(x for x in c if 1 <= x <= R)


def ns_search(R):
    """One limited namespace with exactly R requests in the call, the first nw in window W (the
    last of them on W+99), the rest on W+100.  max_qps = nw + 3: the whole first window and three
    requests of the second pass whether or not the window end is placed right; the limiter then
    holds (nw, 3).  The probe at W+1000 reads the second bucket (nw + 4 requests, nw pass; a
    window end off by one gives nw + 1 or nw - 1), the one at W+1100 the bucket of the first probe."""
    sc = Script(f"ns_search[{R}]", max_batch=max(R, 4096))
    sc.rules([frule(1, HUGE)])
    W = T0
    subs = []
    for nw in search_nw(R):
        sc.ns(nsp(1, 1, nw + 3))                    # (a load starts the limiter empty)
        ts = np.full(R, W + 100, np.int64)
        ts[:nw] = W + 99
        ts[0] = W if nw > 1 else W + 99
        k = sc.big_req(ts, 1)
        sc.req(W + 1000, 1, nw + 4)
        sc.call()
        sc.req(W + 1100, 1, nw + 4)
        sc.call()
        subs.append((nw, k))
        W += 5000

    def guard(R_):
        for nw, k in subs:
            main, p1, p2 = R_[k], R_[k + 1], R_[k + 2]
            second = min(3, R - nw)
            assert (main.status[:nw] == OK).all() and (main.status[nw:nw + second] == OK).all()
            assert (main.status[nw + second:] == TOO_MANY).all()
            n1 = int((p1.status == OK).sum())
            assert n1 == nw + 3 - second and 0 < n1 < nw + 4, (nw, n1)
            assert (p1.status[n1:] == TOO_MANY).all()
            n2 = int((p2.status == OK).sum())
            assert n2 == second and n2 < nw + 4, (nw, n2)       # (no second window: nothing is left)
        return f"R={R}: window ends {[nw for nw, _ in subs]}"
    sc.guard = guard
    return sc


# ---------------------------------------------------------------- 2. ns_first_fail
FF_QPS = (0, 0.5, 1, 1.5, 63, 64, 64.999, 65, 129, 130, 131)     # nw - 1, nw, nw + 1 for nw = 130
FF_TAIL = (0, 1, 63, 64, 65, 129)                                # nw - K: requests past the first failing one


def ns_first_fail():
    """One namespace per max_qps, one flow rule each.  A carried-in sum (1 or 3 requests, those
    that fit, at W+50) then a window at W+100 of nw = K + d requests, K = floor(qps) - carry the
    passes left: the first failing request is K and d requests take the strided scatter.  The
    probe at W+1000 (bucket W is the current one and restarts) passes floor(qps) - K = carry."""
    sc = Script("ns_first_fail")
    qs = FF_QPS
    sc.ns(*[nsp(10 + i, 1, q) for i, q in enumerate(qs)])
    sc.rules([frule(100 + i, HUGE, ns=10 + i) for i in range(len(qs))])
    W = T0
    subs = []
    for d in FF_TAIL:
        for carry in (1, 3):
            for i, q in enumerate(qs):
                c = min(carry, int(q))
                K = int(q) - c
                sc.req(W + 50, 100 + i, c, mark=("carry", d, carry, i))
                sc.req(W + 100 + (i % 3), 100 + i, K + d, mark=("win", d, carry, i))
                subs.append((d, carry, i, c, K))
            sc.call()
            for i, q in enumerate(qs):
                sc.req(W + 1000, 100 + i, int(q) + 1, mark=("p1", d, carry, i))
            sc.call()
            for i, q in enumerate(qs):
                sc.req(W + 1100, 100 + i, int(q) + 1, mark=("p2", d, carry, i))
            sc.call()
            W += 5000

    def guard(R):
        for d, carry, i, c, K in subs:
            if c:
                assert st(sc, R, ("carry", d, carry, i)) == [OK] * c
            if K + d:
                assert st(sc, R, ("win", d, carry, i)) == [OK] * K + [TOO_MANY] * d
            n = int(qs[i]) + 1
            p1 = st(sc, R, ("p1", d, carry, i))
            assert p1 == [OK] * c + [TOO_MANY] * (n - c)
            assert st(sc, R, ("p2", d, carry, i)) == [OK] * (n - 1 - c) + [TOO_MANY] * (1 + c)
            if qs[i] >= 1:                       # (under 1 nothing can ever pass: no probe separates)
                assert 0 < p1.count(OK) < n
        return f"{len(subs)} windows"
    sc.guard = guard
    return sc


# ---------------------------------------------------------------- 3. ns_table
def _table_traffic(sc, W, fids, n_each=5):
    """Interleaved requests of the flow ids, n_each per id and millisecond pair, then two probes."""
    for rep in range(n_each):
        for f in fids:
            sc.req(W + 2 * rep, f, 1, mark=("main", f))
    sc.call()
    for f in fids:
        sc.req(W + 1000, f, 4, mark=("p1", f))
    sc.call()
    for f in fids:
        sc.req(W + 1100, f, 4, mark=("p2", f))
    sc.call()


def ns_table_mixed(rules_first=False):
    """Three limited namespaces (qps 2, 3, 0), one unlimited, one rule of a namespace that is not
    loaded (connected 0: AVG_LOCAL threshold 0), and a limited namespace without a request."""
    sc = Script("ns_table_mixed" + ("_rules_first" if rules_first else ""))
    ns = [nsp(7, 2, 2), nsp(3, 1, 3), nsp(900, 1, 0), nsp(5, 4, -1), nsp(6, 1, 1)]
    flow = [frule(1, HUGE, ns=7), frule(2, HUGE, ns=3), frule(3, HUGE, ns=900), frule(4, 1, tt=AVG_LOCAL, ns=5),
            frule(5, 1, tt=AVG_LOCAL, ns=4242), frule(6, 2, ns=4242), frule(7, HUGE, ns=7)]
    if rules_first:
        sc.rules(flow)
        sc.ns(*ns)
    else:
        sc.ns(*ns)
        sc.rules(flow)
    fids = [1, 2, 3, 4, 5, 6, 7]
    _table_traffic(sc, T0, fids)

    def guard(R):
        main = {f: st(sc, R, ("main", f)) for f in fids}
        # namespace 7 is shared by flow ids 1 and 7: qps 2 admits the first two requests in time order
        assert main[1].count(OK) + main[7].count(OK) == 2 and main[1].count(TOO_MANY) + main[7].count(TOO_MANY) == 8
        assert main[2] == [OK] * 3 + [TOO_MANY] * 2 and main[3] == [TOO_MANY] * 5
        assert main[4] == [OK] * 4 + [BLOCKED] and main[5] == [BLOCKED] * 5 and main[6] == [OK] * 2 + [BLOCKED] * 3
        p1 = {f: st(sc, R, ("p1", f)) for f in fids}
        assert p1[2] == [OK] * 3 + [TOO_MANY]           # bucket W restarted: the limiter is empty again
        assert p1[4] == [OK] * 4 and p1[6] == [OK, OK, BLOCKED, BLOCKED]   # so has the ClusterMetric's bucket 0
        p2 = {f: st(sc, R, ("p2", f)) for f in fids}
        assert p2[2] == [TOO_MANY] * 4 and p2[4] == [BLOCKED] * 4 and p2[6] == [BLOCKED] * 4
        return "5 namespaces"
    sc.guard = guard
    return sc


def ns_table_255():
    """255 namespaces, all limited: index 254 is NS_NONE - 1."""
    sc = Script("ns_table_255")
    sc.ns(*[nsp(1000 + i, 1, 1 + i % 3) for i in range(NS_MAX)])
    idx = (0, 1, 253, 254)
    sc.rules([frule(1 + i, HUGE, ns=1000 + i) for i in idx])
    fids = [1 + i for i in idx]
    _table_traffic(sc, T0, fids)

    def guard(R):
        for i in idx:
            q = 1 + i % 3
            assert st(sc, R, ("main", 1 + i)) == [OK] * q + [TOO_MANY] * (5 - q)
            assert st(sc, R, ("p1", 1 + i)) == [OK] * q + [TOO_MANY] * (4 - q)
            assert st(sc, R, ("p2", 1 + i)) == [TOO_MANY] * 4
        return "indices 0, 1, 253, 254"
    sc.guard = guard
    return sc


def ns_table_none():
    """No namespace loaded (no 8-bit sort, no limiter kernel): connected is 0 for every rule."""
    sc = Script("ns_table_none")
    sc.rules([frule(1, 3, ns=1), frule(2, 3, tt=AVG_LOCAL, ns=1)])
    _table_traffic(sc, T0, [1, 2])

    def guard(R):
        assert st(sc, R, ("main", 1)) == [OK] * 3 + [BLOCKED] * 2 and st(sc, R, ("main", 2)) == [BLOCKED] * 5
        assert st(sc, R, ("p1", 1)) == [OK] * 3 + [BLOCKED] and st(sc, R, ("p2", 1)) == [BLOCKED] * 4
        return "no namespaces"
    sc.guard = guard
    return sc


# ---------------------------------------------------------------- 4. metric_ring / 7. param_columns
GEOMS = ((1, 1000), (2, 1000), (3, 999), (10, 1000), (16, 1600), (16, 16), (16, 16000))
PARAM_GEOMS = ((1, 1000), (4, 1000), (10, 1000), (16, 1600))


def ring_times(S, I):
    wl = I // S
    return sorted({0, wl - 1, wl, I - wl, I - 1, I, I + wl - 1, I + wl, 3 * I})


def fit(count, I):
    """Requests of acquireCount 1 an empty window takes: the k-th passes iff count - k / (I/1000) - 1 >= 0."""
    k = 0
    while count - k / (I / 1000.0) - 1 >= 0:
        k += 1
    return k


def _ring(name, S, I, split, param):
    """Bursts on every edge of the ring: on W, on both sides of the first window's end, of the
    interval's last window and of the interval's end, one window later, and after everything has
    expired.  Each burst is what an empty window takes plus 2 (for I = 1000: count + 2), on a rule
    that a single burst fills (id 1) and on one nine bursts do not fill (id 2), so every burst's
    number of passes is the sum over the ring at that instant."""
    sc = Script(f"{name}[{S}-{I}-{'split' if split else 'one'}]")
    c = 200 if I < 100 else 3
    n = fit(c, I) + 2
    wide = fit(9 * c, I) // 2 + 1
    sc.ns(nsp(1, 1))
    rules = [frule, prule][param]
    sc.rules(**{("param" if param else "flow"): [rules(1, c, S, I), rules(2, 9 * c, S, I)]})
    W = align(T0, I)
    v = [L(7)] if param else None
    times = ring_times(S, I)
    for dt in times:
        sc.req(W + dt, 1, n, vals=v, mark=("tight", dt))
        sc.req(W + dt, 2, wide, vals=v, mark=("wide", dt))
        if split:
            sc.call()
    if not split:
        sc.call()

    def guard(R):
        tight = {dt: st(sc, R, ("tight", dt)) for dt in times}
        for dt in times:
            assert tight[dt][-1] == BLOCKED and sorted(tight[dt]) == tight[dt]       # OK ... then BLOCKED
        assert tight[0].count(OK) == n - 2 and tight[times[-1]].count(OK) == n - 2
        assert tight[I].count(OK) > 0                      # bucket 0 restarted one interval later
        w = [count(sc, R, ("wide", dt)) for dt in times]
        assert 0 < sum(w) < wide * len(times) and w[0] == wide
        return f"passes per burst {[tight[dt].count(OK) for dt in times]} / {w}"
    sc.guard = guard
    return sc


def metric_ring(S, I, split):
    return _ring("metric_ring", S, I, split, False)


def param_columns_ring(S, I, split):
    return _ring("param_columns_ring", S, I, split, True)


def param_columns_values():
    """One column per (rule, tag, bits): the same bits under every tag, under two rules, bits 0 and
    2^64 - 1, the stateless null, hot items (exact match, a null item, duplicates, none), GLOBAL and
    AVG_LOCAL thresholds, and the prioritized flag (ignored on requestParamToken)."""
    sc = Script("param_columns_values")
    sc.ns(nsp(1, 3))
    items = [item(abi.TAG_LONG, 7, 1), item(abi.TAG_NULL, 0, 1), item(abi.TAG_LONG, 9, 5), item(abi.TAG_LONG, 9, 1),
             item(abi.TAG_INT, 11, 0)]
    sc.rules(param=[prule(1, 3), prule(2, 2, tt=AVG_LOCAL), prule(3, 3, off=0, cnt=5), prule(4, 3, off=0, cnt=0)],
             items=items)
    W = T0
    for tag in WIRE_TAGS:
        sc.req(W, 1, 5, vals=[(tag, 7)], mark=("tag", tag))
    sc.req(W, 1, 5, vals=[NULL], mark="null")
    sc.req(W, 2, 8, vals=[L(7)], mark="avg_local")
    for bits in (0, 2 ** 64 - 1):
        sc.req(W, 1, 5, vals=[L(bits)], prio=True, mark=("bits", bits))
    sc.req(W, 3, 3, vals=[L(7)], mark="hot_exact")            # item (LONG, 7) -> 1
    sc.req(W, 3, 5, vals=[(abi.TAG_INT, 7)], mark="hot_other_tag")   # no item: rule count 3
    sc.req(W, 3, 2, vals=[NULL], mark="hot_null_1")
    sc.req(W, 3, 2, count=2, vals=[NULL], mark="hot_null_2")
    sc.req(W, 3, 7, vals=[L(9)], mark="hot_dup")              # the first (LONG, 9) item: 5
    sc.req(W, 3, 2, vals=[(abi.TAG_INT, 11)], mark="hot_zero")
    sc.req(W, 4, 5, vals=[L(7)], mark="no_items")
    sc.call()
    for tag in WIRE_TAGS:                                     # probe: one more of each next window
        sc.req(W + 100, 1, 1, vals=[(tag, 7)], mark=("tag2", tag))
    sc.req(W + 1000, 1, 4, vals=[L(7)], mark="restart")
    sc.call()

    def guard(R):
        for tag in WIRE_TAGS:
            assert st(sc, R, ("tag", tag)) == [OK] * 3 + [BLOCKED] * 2 and st(sc, R, ("tag2", tag)) == [BLOCKED]
        k, idx = sc.marks["null"]
        assert st(sc, R, "null") == [OK] * 5 and list(R[k].remaining[idx]) == [2] * 5
        assert st(sc, R, "avg_local") == [OK] * 6 + [BLOCKED] * 2
        for bits in (0, 2 ** 64 - 1):
            assert st(sc, R, ("bits", bits)) == [OK] * 3 + [BLOCKED] * 2
        assert st(sc, R, "hot_exact") == [OK, BLOCKED, BLOCKED] and st(sc, R, "hot_other_tag") == [OK] * 3 + [BLOCKED] * 2
        assert st(sc, R, "hot_null_1") == [OK, OK] and st(sc, R, "hot_null_2") == [BLOCKED, BLOCKED]
        assert st(sc, R, "hot_dup") == [OK] * 5 + [BLOCKED] * 2 and st(sc, R, "hot_zero") == [BLOCKED] * 2
        assert st(sc, R, "no_items") == [OK] * 3 + [BLOCKED] * 2
        assert st(sc, R, "restart") == [OK] * 3 + [BLOCKED]
        assert (R[0].wait_ms == 0).all()
        return "8 tags, null, hot items"
    sc.guard = guard
    return sc


# ---------------------------------------------------------------- 5. occupy
def occupy_base():
    """GLOBAL count 2, S=2, I=1000: the script of ClusterMetric.tryOccupyNext, one call per instant."""
    sc = Script("occupy_base")
    sc.ns(nsp(1, 1))
    sc.rules([frule(1, 2, 2, 1000)])
    W = T0
    sc.req(W, 1, 3, mark="a")
    sc.call()
    sc.req(W + 500, 1, 1, mark="b")
    sc.req(W + 500, 1, 2, prio=True, mark="b")
    sc.call()
    sc.req(W + 1000, 1, 2, mark="c")
    sc.call()
    sc.req(W + 1500, 1, 1, mark="c2")
    sc.call()

    def guard(R):
        got = st(sc, R, "a") + st(sc, R, "b") + st(sc, R, "c") + st(sc, R, "c2")
        assert got == [OK, OK, BLOCKED, BLOCKED, WAIT, WAIT, BLOCKED, BLOCKED, BLOCKED], got
        assert list(R[1].wait_ms) == [0, 500, 500]
        assert R[1].sums[(1, W + 500)][CE_OCCUPIED_PASS] == 0 and R[2].sums[(1, W + 1000)][CE_OCCUPIED_PASS] == 2
        return "OK OK B | B W W | B B | B"
    sc.guard = guard
    return sc


def occupy_geometry(S, gap=None):
    """The same on S buckets: the occupy sits in the interval's last window (the head bucket is the
    one with the passes), a third prioritized request is one too many (OCCUPIED_BLOCK); then the
    next request one window later (the head bucket restarts: transfer), or after `gap`."""
    I = 1600 if S == 16 else 1000          # (S divides I)
    wl = I // S
    sc = Script(f"occupy_geometry[{S}-{gap}]")
    sc.read_ahead = False
    sc.ns(nsp(1, 1))
    sc.rules([frule(1, 2, S, I)])
    W = align(T0, I)
    t1 = W + I - wl + wl // 2
    t2 = W + I if gap is None else t1 + gap
    sc.req(W, 1, 3, mark="a")
    sc.call()
    sc.req(t1, 1, 1, mark="b_plain")
    sc.req(t1, 1, 3, prio=True, mark="b_prio")
    sc.call()
    sc.req(t2, 1, 2, mark="c")
    sc.call()

    def guard(R):
        assert st(sc, R, "a") == [OK, OK, BLOCKED] and st(sc, R, "b_plain") == [BLOCKED]
        assert st(sc, R, "b_prio") == [WAIT, WAIT, BLOCKED]
        k, idx = sc.marks["b_prio"]
        assert list(R[k].wait_ms[idx]) == [1000 // S, 1000 // S, 0]
        assert R[1].sums[(1, t1)][CE_OCCUPIED_PASS] == 0 and R[1].sums[(1, t1)][CE_WAITING] == 2
        assert R[1].sums[(1, t1)][CE_OCCUPIED_BLOCK] == 1
        # the two occupied passes arrive with the first bucket restarted after them, and fill the rule
        assert R[2].sums[(1, t2)][CE_OCCUPIED_PASS] == 2 and R[2].sums[(1, t2)][CE_PASS] == 2
        assert st(sc, R, "c") == [BLOCKED] * 2
        return f"wait {1000 // S}"
    sc.guard = guard
    return sc


def occupy_new_buckets():
    """S=10, everything in the ring's first turn: passes in bucket 1 (W+100), the occupy at W+1000
    in bucket 0 (created there: a new empty bucket, no transfer), requests at W+1200 in bucket 2
    (created there: no transfer, so they pass beside the pending occupy); the transfer happens at
    W+2000, where bucket 0 is the first one to restart."""
    sc = Script("occupy_new_buckets")
    sc.ns(nsp(1, 1))
    sc.rules([frule(1, 2, 10, 1000)])
    W = T0
    sc.req(W + 100, 1, 3, mark="a")
    sc.call()
    sc.req(W + 1000, 1, 1, mark="b")
    sc.req(W + 1000, 1, 2, prio=True, mark="b")
    sc.call()
    sc.req(W + 1200, 1, 3, mark="c")
    sc.call()
    sc.req(W + 2000, 1, 1, mark="d")
    sc.call()

    def guard(R):
        assert st(sc, R, "a") == [OK, OK, BLOCKED] and st(sc, R, "b") == [BLOCKED, WAIT, WAIT]
        assert st(sc, R, "c") == [OK, OK, BLOCKED] and st(sc, R, "d") == [BLOCKED]
        occ = [R[k].sums[(1, t)][CE_OCCUPIED_PASS] for k, t in enumerate((W + 100, W + 1000, W + 1200, W + 2000))]
        assert occ == [0, 0, 0, 2], occ
        return "transfer in call 3"
    sc.guard = guard
    return sc


def occupy_ratio(ratio):
    """max_occupy_ratio: WAITING on ratio * threshold still occupies, one above does not (for ratio 1
    canOccupy's own limit, threshold - 1 + 1 occupied, comes first)."""
    sc = Script(f"occupy_ratio[{ratio}]", max_occupy_ratio=ratio)
    sc.ns(nsp(1, 1))
    sc.rules([frule(1, 4, 2, 1000)])
    W = T0
    sc.req(W, 1, 5, mark="a")
    sc.req(W + 500, 1, 6, prio=True, mark="b")
    sc.call()
    sc.req(W + 1000, 1, 5, mark="c")
    sc.call()
    waits = {0: 1, 0.5: 3, 1: 4}[ratio]

    def guard(R):
        assert st(sc, R, "a") == [OK] * 4 + [BLOCKED]
        assert st(sc, R, "b") == [WAIT] * waits + [BLOCKED] * (6 - waits)
        assert st(sc, R, "c") == [OK] * (4 - waits) + [BLOCKED] * (1 + waits)
        return f"{waits} occupied"
    sc.guard = guard
    return sc


def exceed(factor):
    """exceed_count scales the threshold: the request that brings next to exactly 0 passes with
    remaining 0, the one after it is blocked."""
    sc = Script(f"exceed[{factor}]", exceed_count=factor)
    sc.ns(nsp(1, 2))
    sc.rules([frule(1, 4), frule(2, 2, tt=AVG_LOCAL), frule(3, 3)])
    thr = int(4 * factor)
    W = T0
    sc.req(W, 1, thr + 2, mark="g")
    sc.req(W, 2, thr + 2, mark="l")
    sc.req(W, 3, 4, count=2, mark="odd")          # 3 * factor: 1.5, 4.5, 6 against 2, 4, 6, 8
    sc.call()
    sc.req(W + 1000, 1, thr + 2, mark="g2")
    sc.call()

    def guard(R):
        for m in ("g", "l"):
            k, idx = sc.marks[m]
            assert st(sc, R, m) == [OK] * thr + [BLOCKED] * 2
            assert list(R[k].remaining[idx]) == list(range(thr - 1, -1, -1)) + [0, 0]
        odd = int(3 * factor) // 2
        assert st(sc, R, "odd") == [OK] * odd + [BLOCKED] * (4 - odd) and 0 <= odd < 4
        assert st(sc, R, "g2") == [OK] * thr + [BLOCKED] * 2
        return f"threshold {thr}"
    sc.guard = guard
    return sc


# ---------------------------------------------------------------- 6. numeric
NUM_COUNTS = (0.0, -1.0, 0.5, 10.5, 1e12, float("inf"), float("nan"))
BIG_IDS = (1, 2 ** 31, 2 ** 32 + 1, 2 ** 63 - 1)


def numeric():
    sc = Script("numeric")
    sc.ns(nsp(1, 3))
    flow = [frule(100 + i, c) for i, c in enumerate(NUM_COUNTS)] + \
           [frule(200 + i, c, tt=AVG_LOCAL) for i, c in enumerate(NUM_COUNTS)] + \
           [frule(x, 2) for x in BIG_IDS] + [frule(50, 1), frule(50, 100), frule(60, 2)]
    param = [prule(300 + i, c) for i, c in enumerate(NUM_COUNTS)] + [prule(x, 1) for x in BIG_IDS] + [prule(70, 2)]
    sc.rules(flow, param)
    W = T0
    for i in range(len(NUM_COUNTS)):
        for base in (100, 200):
            sc.req(W, base + i, 2, mark=("f", base + i))
            sc.req(W + 1, base + i, 1, prio=True, mark=("f", base + i))
            sc.req(W + 2, base + i, 1, count=INT_MAX, mark=("fmax", base + i))
        sc.req(W, 300 + i, 2, vals=[L(1)], mark=("p", 300 + i))
        sc.req(W + 2, 300 + i, 1, count=INT_MAX, vals=[L(1)], mark=("pmax", 300 + i))
    for x in BIG_IDS:
        sc.req(W, x, 3, mark=("id", x))
        sc.req(W, x, 2, vals=[L(5)], mark=("pid", x))
    sc.req(W, 306, 1, vals=[NULL], mark="nan_null")
    sc.req(W, 50, 3, mark="dup")
    sc.req(W, 60, 1, vals=[L(1)], mark="flow_as_param")
    sc.req(W, 70, 1, mark="param_as_flow")
    sc.call()

    def guard(R):
        r0 = R[0]
        want = {0: [BLOCKED] * 3, 1: [BLOCKED] * 3, 2: [BLOCKED] * 3, 3: [OK] * 3, 4: [OK] * 3, 5: [OK] * 3, 6: [BLOCKED] * 3}
        for i in range(len(NUM_COUNTS)):
            assert st(sc, R, ("f", 100 + i)) == want[i], (i, st(sc, R, ("f", 100 + i)))
            # ClusterParamFlowChecker blocks on nextRemaining < 0 (a NaN passes, remaining (int) NaN = 0),
            # ClusterFlowChecker passes on nextRemaining >= 0 (a NaN is blocked)
            assert st(sc, R, ("p", 300 + i)) == (want[i][:2] if i != 6 else [OK, OK])
        assert st(sc, R, ("f", 202)) == [OK, BLOCKED, BLOCKED]          # 0.5 * 3 connected
        k, idx = sc.marks[("f", 103)]
        assert list(r0.remaining[idx]) == [9, 8, 7]                       # 10.5 - k - 1, truncated
        for i in (4, 5):
            k, idx = sc.marks[("f", 100 + i)]
            assert list(r0.remaining[idx]) == [INT_MAX] * 3
        assert st(sc, R, ("fmax", 104)) == [OK] and st(sc, R, ("fmax", 103)) == [BLOCKED]
        assert st(sc, R, ("pmax", 304)) == [OK] and st(sc, R, ("fmax", 106)) == [BLOCKED]
        k, idx = sc.marks[("p", 306)]
        assert st(sc, R, ("pmax", 306)) == [OK] and list(r0.remaining[idx]) == [0, 0]
        assert st(sc, R, "nan_null") == [OK]
        for x in BIG_IDS:
            assert st(sc, R, ("id", x)) == [OK, OK, BLOCKED] and st(sc, R, ("pid", x)) == [OK, BLOCKED]
        assert st(sc, R, "dup") == [OK, BLOCKED, BLOCKED]
        assert st(sc, R, "flow_as_param") == [NO_RULE] and st(sc, R, "param_as_flow") == [NO_RULE]
        return "counts, ids, acquireCount"
    sc.guard = guard
    return sc


def connected_reload():
    """load_namespaces between two calls changes connected_count: the ClusterMetric is kept (only 2
    of the new threshold's 6 are left) and the limiter starts empty (5 pass it again)."""
    sc = Script("connected_reload")
    sc.ns(nsp(1, 2, 5))
    sc.rules([frule(1, 2, tt=AVG_LOCAL)], [prule(2, 2, tt=AVG_LOCAL)])
    W = T0
    sc.req(W, 1, 7, mark="a")
    sc.call()
    sc.ns(nsp(1, 3, 5))
    sc.req(W + 10, 1, 7, mark="b")
    sc.call()

    def guard(R):
        assert st(sc, R, "a") == [OK] * 4 + [BLOCKED] + [TOO_MANY] * 2
        assert st(sc, R, "b") == [OK] * 2 + [BLOCKED] * 3 + [TOO_MANY] * 2
        return "metric kept, limiter reset"
    sc.guard = guard
    return sc


# ---------------------------------------------------------------- 8. param_table
def param_table():
    """param_capacity 1 gives the smallest table, CP_MIN_SLOTS slots (probe reach: all of them)."""
    sc = Script("param_table", max_batch=8192)
    sc.cfg["param_capacity"] = 1
    sc.ns(nsp(1, 1))
    rules = dict(param=[prule(1, 3)])
    sc.rules(**rules)
    W = T0
    vals = [(i * 0x9E3779B97F4A7C15 + 12345) % 2 ** 64 for i in range(CP_MIN_SLOTS)]
    for i, v in enumerate(vals):                      # every slot claimed in one call
        sc.req(W, 1, count=1 + i % 2, vals=[L(v)], mark="fill")
    sc.call()
    for i, v in enumerate(vals):                      # found again in the full table; odd ones were taken twice
        sc.req(W + 1, 1, count=2, vals=[L(v)], mark=("again", i % 2))
    sc.call()
    sc.rules(**rules)                                 # a reload empties the table
    sc.req(W + 2, 1, 4096, vals=[L(77)], mark="one")  # one new slot claimed by 4096 lanes
    sc.call()
    sc.rules(**rules)
    for i in range(4096):
        sc.req(W + 3, 1, 1, vals=[L(1000 + i % 64)], mark=("rr", i % 64))
    sc.call()

    def guard(R):
        assert st(sc, R, "fill") == [OK] * CP_MIN_SLOTS
        assert st(sc, R, ("again", 0)) == [OK] * (CP_MIN_SLOTS // 2)
        assert st(sc, R, ("again", 1)) == [BLOCKED] * (CP_MIN_SLOTS // 2)
        assert st(sc, R, "one") == [OK] * 3 + [BLOCKED] * 4093
        for v in range(64):
            assert st(sc, R, ("rr", v)) == [OK] * 3 + [BLOCKED] * 61
        return f"{CP_MIN_SLOTS} slots"
    sc.guard = guard
    return sc


def param_table_overflow():
    """(first call, second call): the second needs slot number CP_MIN_SLOTS + 1 -> SF_ERR_CAPACITY."""
    sc = Script("param_table_overflow")
    sc.cfg["param_capacity"] = 1
    sc.ns(nsp(1, 1))
    sc.rules(param=[prule(1, 3)])
    for i in range(CP_MIN_SLOTS):
        sc.req(T0, 1, 1, vals=[L(i + 1)])
    sc.call()
    sc.req(T0 + 1, 1, 1, vals=[L(CP_MIN_SLOTS + 1)])
    sc.call()
    return sc


# ---------------------------------------------------------------- 9. param_serial
def param_serial():
    """A rule is decided per value in the odd calls (every request has one value, passed through
    param_off) and by one lane in time order in the even ones (a request with several values),
    over the same columns."""
    sc = Script("param_serial")
    sc.ns(nsp(1, 1))
    sc.rules(param=[prule(1, 3), prule(2, 3)])
    a, b, c, d, e, f, g, h = (L(x) for x in range(1, 9))
    W = T0
    sc.req(W + 50, 1, 2, vals=[a], mark="a_first")
    sc.req(W + 50, 2, 1, vals=[a], mark="r2")
    sc.call(off=True)                                   # per value
    t = W + 110
    sc.req(t, 1, 1, vals=[a, b], mark="ab")             # a: 3, b: 1
    sc.req(t + 1, 1, 1, vals=[c, a], mark="ca")         # a has no room: blocked, c not added
    sc.req(t + 2, 1, 1, vals=[a, c], mark="ac")         # the first value stops the check
    sc.req(t + 3, 1, 1, vals=[b, b], mark="bb")         # both see 1: b: 3
    sc.req(t + 4, 1, 1, vals=[NULL, d], mark="nd")      # d: 1
    sc.req(t + 5, 1, 1, vals=[NULL, NULL], mark="nn")
    sc.req(t + 6, 1, 1, vals=[d, e, f, g, h], mark="five")   # d: 2, e to h: 1
    sc.req(t + 7, 1, 1, vals=[], mark="empty")
    sc.req(t + 8, 1, 1, vals=[e], mark="single_in_serial")   # e: 2
    sc.req(t + 9, 2, 1, vals=[a], mark="r2b")           # rule 2 stays per value in this call
    sc.call()
    t = W + 130
    for x, v in enumerate((a, b, c, d, e, f, g, h)):    # per value again: 4 of each
        sc.req(t, 1, 4, vals=[v], mark=("probe", x))
    sc.req(t, 2, 3, vals=[a], mark="r2c")
    sc.call(off=True)
    t = W + 1060                                        # serial again: bucket 0 restarts, a's first two have left
    sc.req(t, 1, 1, vals=[a, b], mark="late")
    sc.req(t, 1, 1, vals=[a, a, a], mark="late3")
    sc.call()
    sc.req(W + 1065, 1, 3, vals=[a], mark="late_probe")
    sc.call(off=True)

    def guard(R):
        assert st(sc, R, "a_first") == [OK, OK]
        k, _ = sc.marks["ab"]
        r = R[k]
        assert (r.remaining == -1).sum() >= 3
        assert st(sc, R, "ab") == [OK] and st(sc, R, "ca") == [BLOCKED] and st(sc, R, "ac") == [BLOCKED]
        assert st(sc, R, "bb") == [OK] and st(sc, R, "nd") == [OK] and st(sc, R, "nn") == [OK]
        assert st(sc, R, "five") == [OK] and st(sc, R, "empty") == [BAD]
        assert st(sc, R, "single_in_serial") == [OK]
        left = [count(sc, R, ("probe", x)) for x in range(8)]
        assert left == [0, 0, 3, 1, 1, 2, 2, 2], left      # c was never added: all 3 are left
        assert st(sc, R, "r2") + st(sc, R, "r2b") + st(sc, R, "r2c") == [OK, OK, OK, BLOCKED, BLOCKED]
        # at W+1060 a holds the serial call's 1 and b its 3 (bucket 1 is still inside): [a, b] is
        # blocked on b, [a, a, a] passes (each check sees 1) and adds 3
        assert st(sc, R, "late") == [BLOCKED] and st(sc, R, "late3") == [OK]
        assert st(sc, R, "late_probe") == [BLOCKED] * 3
        return f"left per value {left}"
    sc.guard = guard
    return sc


# ---------------------------------------------------------------- 10. degenerate
def degenerate_single():
    """Calls of one request, one per status."""
    sc = Script("degenerate_single", max_batch=1)
    sc.ns(nsp(1, 1, 2), nsp(2, 1))
    sc.rules([frule(1, 1, 2, 1000, ns=2), frule(2, HUGE, ns=1)], [prule(3, 1, ns=2)])
    W = T0
    seq = [(W, 1, {}), (W + 1, 1, {}), (W + 500, 1, dict(prio=True)), (W + 501, 99, {}), (W + 502, 0, {}),
           (W + 503, 2, {}), (W + 504, 2, {}), (W + 505, 2, {}), (W + 506, 3, dict(vals=[L(1)])),
           (W + 507, 3, dict(vals=[L(1)])), (W + 508, 3, dict(vals=[], param=True)), (W + 509, 1, dict(count=0))]
    for i, (t, fid, kw) in enumerate(seq):
        sc.req(t, fid, **kw)
        if i == 10:
            sc.call(plain=True)                      # requestParamToken with params == null
        else:
            sc.call()

    def guard(R):
        got = [int(r.status[0]) for r in R]
        assert got == [OK, BLOCKED, WAIT, NO_RULE, BAD, OK, OK, TOO_MANY, OK, BLOCKED, BAD, BAD], got
        assert R[2].wait_ms[0] == 500
        return "six statuses"
    sc.guard = guard
    return sc


def degenerate_uniform():
    """Calls whose requests all end before the checker (n_seg stays 0), and a single valid request
    at the first and at the last index."""
    sc = Script("degenerate_uniform")
    sc.ns(nsp(1, 1, 0), nsp(2, 1))
    sc.rules([frule(1, HUGE, ns=1), frule(2, 2, ns=2)])
    W = T0
    sc.req(W, -3, 3, mark="bad")
    sc.req(W, 2, 2, count=0, mark="bad")
    sc.call()
    sc.req(W + 1, 77, 5, mark="norule")
    sc.call()
    sc.req(W + 2, 1, 5, mark="toomany")
    sc.call()
    sc.req(W + 3, 2, 1, mark="first")
    sc.req(W + 4, 0, 4, mark="first")
    sc.call()
    sc.req(W + 5, 0, 4, mark="last")
    sc.req(W + 6, 2, 1, mark="last")
    sc.call()
    sc.req(W + 7, 2, 2, mark="probe")
    sc.call()

    def guard(R):
        assert st(sc, R, "bad") == [BAD] * 5 and st(sc, R, "norule") == [NO_RULE] * 5
        assert st(sc, R, "toomany") == [TOO_MANY] * 5
        assert st(sc, R, "first") == [OK] + [BAD] * 4 and st(sc, R, "last") == [BAD] * 4 + [OK]
        assert st(sc, R, "probe") == [BLOCKED, BLOCKED]
        return "uniform calls"
    sc.guard = guard
    return sc


SEG_COUNTS = (63, 64, 65, 129)
SEG_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)


def degenerate_ids():
    """One flow id per request around the TD_T segments of one workgroup (even ids take 1, odd ids
    2; the probe call asks each again)."""
    sc = Script("degenerate_ids")
    sc.read_ahead = False                    # (129 rules: 903 reads per call as it is)
    sc.ns(nsp(1, 1))
    sc.rules([frule(1000 + i, 1 + i % 2) for i in range(max(SEG_COUNTS))])
    W = T0
    for n in SEG_COUNTS:
        for i in range(n):
            sc.req(W + i % 7, 1000 + i, 1, mark=("ids", n))
        sc.call()
        for i in range(n):
            sc.req(W + 10, 1000 + i, 1, mark=("ids2", n, i % 2))
        sc.call()
        W += 3000

    def guard(R):
        for n in SEG_COUNTS:
            assert st(sc, R, ("ids", n)) == [OK] * n
            assert st(sc, R, ("ids2", n, 0)) == [BLOCKED] * ((n + 1) // 2) and st(sc, R, ("ids2", n, 1)) == [OK] * (n // 2)
        return "one segment per request"
    sc.guard = guard
    return sc


def degenerate_segments():
    """One segment of n requests."""
    sc = Script("degenerate_segments", max_batch=4200)
    sc.ns(nsp(1, 1))
    sc.rules([frule(1, 30)])
    W = T0
    for n in SEG_LENGTHS:
        sc.req(W, 1, n, mark=("seg", n))
        sc.call()
        W += 3000

    def guard(R):
        for n in SEG_LENGTHS:
            assert st(sc, R, ("seg", n)) == [OK] * min(n, 30) + [BLOCKED] * max(n - 30, 0)
        return "one segment"
    sc.guard = guard
    return sc


def degenerate_reload():
    """load_cluster_rules again: new ClusterMetric objects and empty value columns."""
    sc = Script("degenerate_reload")
    sc.ns(nsp(1, 1))
    rules = ([frule(1, 2)], [prule(2, 2)])
    sc.rules(*rules)
    W = T0
    for k in range(2):
        sc.req(W + k, 1, 3, mark=("f", k))
        sc.req(W + k, 2, 3, vals=[L(5)], mark=("p", k))
        sc.call()
        if k == 0:
            sc.rules(*rules)
    sc.req(W + 2, 1, 1, mark="f_probe")
    sc.req(W + 2, 2, 1, vals=[L(5)], mark="p_probe")
    sc.call()

    def guard(R):
        for k in range(2):                     # (kept state would block all of the second call)
            assert st(sc, R, ("f", k)) == [OK, OK, BLOCKED] and st(sc, R, ("p", k)) == [OK, OK, BLOCKED]
        assert st(sc, R, "f_probe") == [BLOCKED] and st(sc, R, "p_probe") == [BLOCKED]
        return "reload"
    sc.guard = guard
    return sc


def _cases():
    c = {}

    def add(make, *args):
        name = make.__name__ + ("[" + "-".join(str(a) for a in args) + "]" if args else "")
        c[name] = (lambda: make(*args))
    for R in SEARCH_R:
        add(ns_search, R)
    add(ns_first_fail)
    add(ns_table_mixed, False)
    add(ns_table_mixed, True)
    add(ns_table_255)
    add(ns_table_none)
    for S, I in GEOMS:
        for split in (False, True):
            add(metric_ring, S, I, split)
    add(occupy_base)
    for S in (1, 2, 10, 16):
        add(occupy_geometry, S)
    for gap in (1500, 3000):
        add(occupy_geometry, 2, gap)
    add(occupy_new_buckets)
    for ratio in (0, 0.5, 1):
        add(occupy_ratio, ratio)
    for x in (0.5, 1.5, 2):
        add(exceed, x)
    add(numeric)
    add(connected_reload)
    for S, I in PARAM_GEOMS:
        for split in (False, True):
            add(param_columns_ring, S, I, split)
    add(param_columns_values)
    add(param_table)
    add(param_serial)
    add(degenerate_single)
    add(degenerate_uniform)
    add(degenerate_ids)
    add(degenerate_segments)
    add(degenerate_reload)
    return c


CASES = _cases()
