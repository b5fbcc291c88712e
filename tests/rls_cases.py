"""TEST-ONLY workloads of the Envoy rate-limit service path (sf_request_rls),
shared by tests/test_rls_model.py (the guards, on the model alone) and
tests/test_gpu_rls.py (the engine against the model).

A case is a rule table and a list of calls on one engine:
  ("rls", requests)        one sf_request_rls of (domain, descriptors, hits, ts) tuples
  ("tok", HostTokenBatch)  one sf_request_tokens
  ("load", flow rules)     sf_load_cluster_rules between two calls

Sizes follow the constants of sentinel_amd/csrc/sf_rls.h:
  RLS_WAVE_MIN  read from the header's text: the border between the lane and
                the wave route; the wave-border cases are built around it
  CHUNK = 64    RLS_CHUNK, one wavefront: chunk positions 0 / 31 / 63 / 64 and
                the lengths 63 / 64 / 65 are its first, middle and last lane
                and the first lane of the next chunk
  BLOCK = 256   RLS_T, the workgroup of the per-request / per-descriptor
                kernels: the mixed case's calls (thousands of requests) span
                many workgroups, the string case (< 256) ends inside the first
  LANE_T = 64   RLS_LANE_T, segments per workgroup of the lane route: the mixed
                case has 200 rules (4 workgroups, the last one partial)
tests/test_rls_model.py fails when these drift from the header."""
import os
import re

import numpy as np

from sentinel_amd import abi
from tests import rls_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RLS_HEADER = os.path.join(ROOT, "sentinel_amd", "csrc", "sf_rls.h")
CHUNK, BLOCK, LANE_T = 64, 256, 64
EVENTS = range(7)                    # ClusterFlowEvent ordinals


def header_constants():
    src = open(RLS_HEADER).read()
    return {k: int(v) for k, v in re.findall(r"constexpr \w+ (RLS_\w+) = (\d+);", src)}


WAVE_MIN = header_constants()["RLS_WAVE_MIN"]

# every ill-formed class of the contract (include/sentinel_flow.h)
ILL_FORMED = {
    "overlong_2": b"a\xc0\x80", "overlong_c1": b"\xc1\xbf", "overlong_3": b"\xe0\x80\x80z", "overlong_3b": b"\xe0\x9f\xbf",
    "overlong_4": b"\xf0\x80\x80\x80", "overlong_4b": b"\xf0\x8f\xbf\xbf",
    "lone_continuation": b"ab\x80", "lone_continuation_bf": b"\xbf",
    "missing_continuation_2": b"\xc3A", "missing_continuation_3": b"\xe2\x82A", "missing_continuation_4": b"\xf0\x9f\x98A",
    "cut_2": b"abc\xc3", "cut_3": b"\xe2\x82", "cut_4": b"x\xf0\x9f\x98",
    "surrogate_d800": b"\xed\xa0\x80", "surrogate_dfff": b"\xed\xbf\xbf", "surrogate_pair": b"\xed\xa0\xbd\xed\xb8\x80",
    "above_10ffff": b"\xf4\x90\x80\x80", "f5": b"\xf5\x80\x80\x80", "f7": b"\xf7\xbf\xbf\xbf",
    "f8": b"\xf8\x88\x80\x80\x80", "fc": b"\xfc\x84\x80\x80\x80\x80", "fe": b"\xfe", "ff": b"a\xffb",
}


def flow_rule(key, count, sample_count=1, interval=1000, ns=0, threshold_type=abi.THRESHOLD_GLOBAL, flow_id=None):
    fid = rm.generate_flow_id(key) if flow_id is None else flow_id
    return abi.sf_cluster_flow_rule(flow_id=fid, count=float(count), threshold_type=threshold_type, namespace_id=ns,
                                    sample_count=sample_count, window_interval_ms=interval)


class Case:
    def __init__(self, name, flow, calls, namespaces=(), param=(), max_batch=None):
        self.name, self.flow, self.calls = name, list(flow), calls
        self.namespaces, self.param = list(namespaces), list(param)
        nd = [sum(len(r[1]) for r in c[1]) for c in calls if c[0] == "rls"]
        nr = [len(c[1]) for c in calls if c[0] == "rls"] + [c[1].n for c in calls if c[0] == "tok"]
        self.max_batch = max_batch or max(nd + nr + [16])

    def config(self, **kw):
        return abi.default_config(max_resources=4, max_batch=self.max_batch, **kw)

    def rules_at_end(self):
        flow = self.flow
        for c in self.calls:
            if c[0] == "load":
                flow = c[1]
        return flow

    def last_ts(self):
        ts = [c[1][-1][3] for c in self.calls if c[0] == "rls" and c[1]] + \
             [int(c[1].ts_ms[-1]) for c in self.calls if c[0] == "tok"]
        return max(ts)


class Reference:
    """The model's answers of a case: computed once, read by every test that needs them."""

    def __init__(self, case, so):
        m = rm.RlsModel(so, case.config(), case.flow, case.namespaces, case.param)
        self.results = []
        for kind, arg in case.calls:
            if kind == "rls":
                self.results.append(m.should_rate_limit(arg))
            elif kind == "tok":
                self.results.append(m.request_tokens(arg))
            else:
                m.load_cluster_rules(arg, case.param)
                self.results.append(None)
        self.sums = sums(m, case)
        self.model = m


def sums(x, case):
    """ClusterMetric.getSum of all 7 events of every rule at the last ts_ms and one interval later."""
    out = {}
    now = case.last_ts()
    for f in case.rules_at_end():
        if f.flow_id <= 0:
            continue
        for when in (now, now + f.window_interval_ms):
            for ev in EVENTS:
                out[(f.flow_id, ev, when)] = x.cluster_sum(f.flow_id, ev, when)
    return out


_REF = {}


def reference(case, so) -> Reference:
    if case.name not in _REF:
        _REF[case.name] = Reference(case, so)
    return _REF[case.name]


def segments(case, ref):
    """Per rls call: {flow id: descriptors that reach the checker}, i.e. the segment lengths of the sort."""
    out = []
    for (kind, _), res in zip(case.calls, ref.results):
        if kind != "rls":
            continue
        ids, cnt = np.unique(res.flow_id[res.limit != abi.RLS_NO_LIMIT], return_counts=True)
        out.append(dict(zip(ids.tolist(), cnt.tolist())))
    return out


def routes(case, ref):
    """(segments on the lane route, segments on the wave route) the model predicts."""
    lens = [n for call in segments(case, ref) for n in call.values()]
    return sum(n < WAVE_MIN for n in lens), sum(n >= WAVE_MIN for n in lens)


# ---------------------------------------------------------------- 1. mixed traffic
def mixed(seed=7, n_req=20_000, n_rules=200, span_ms=5000, n_calls=3):
    rng = np.random.default_rng(seed)
    counts = ([0, 0.5, 2.5] + list(range(1, 51))) * 4
    keys = [("mesh", [("svc", f"s{i}")] + ([("route", f"r{i % 7}")] if i % 3 == 0 else [])) for i in range(n_rules)]
    flow = [flow_rule(rm.generate_key(d, e), counts[i], sample_count=(1, 2, 10)[i % 3]) for i, (d, e) in enumerate(keys)]
    w = 1.0 / np.arange(1, n_rules + 1) ** 1.1
    w /= w.sum()
    ts = np.sort(rng.integers(100_000, 100_000 + span_ms, n_req))
    hits_of = [0, 1, 1, 1, 2, 5, -1]
    reqs = []
    for i in range(n_req):
        descs = []
        for _ in range(int(rng.integers(0, 5))):
            if rng.random() < 0.1:
                descs.append([("svc", f"unknown{int(rng.integers(0, 50))}")])
            else:
                descs.append(keys[int(rng.choice(n_rules, p=w))][1])
        reqs.append(("mesh", descs, hits_of[int(rng.integers(0, len(hits_of)))], int(ts[i])))
    cuts = np.linspace(0, n_req, n_calls + 1).astype(int)
    return Case("mixed", flow, [("rls", reqs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])


def guard_mixed(case, ref, stats=None):
    code = np.concatenate([r.code for r in ref.results])
    fid = np.concatenate([r.flow_id for r in ref.results])
    limit = np.concatenate([r.limit for r in ref.results])
    overall = np.concatenate([r.overall for r in ref.results])
    both = sum(1 for f in case.flow
               if {abi.RLS_OK, abi.RLS_OVER_LIMIT} <= set(code[(fid == f.flow_id) & (limit != abi.RLS_NO_LIMIT)].tolist()))
    assert both >= 20, both
    n_err = int((overall == abi.RLS_ERROR).sum())
    n_norule = int(((limit == abi.RLS_NO_LIMIT) & (code == abi.RLS_OK)).sum())
    assert n_err > 0 and n_norule > 0
    lane, wave = routes(case, ref)
    assert lane > 0 and wave > 0, (lane, wave)
    if stats is not None:
        assert stats.error_requests == n_err and stats.no_rule == n_norule
        assert (stats.segs_lane, stats.segs_wave) == (lane, wave)
        assert stats.requests == len(overall) and stats.descriptors == len(code)


# ---------------------------------------------------------------- 2. wave borders
BORDER_LENGTHS = [1, CHUNK - 1, CHUNK, CHUNK + 1, WAVE_MIN - 1, WAVE_MIN, WAVE_MIN + 1, 4 * WAVE_MIN + 17]
FIRST_BLOCK = [0, CHUNK // 2 - 1, CHUNK - 1, CHUNK]


def _border_requests(L):
    """(descriptors, acquireCount) of the requests that carry L descriptors:
    some requests have two (two consecutive acquisitions on one id); 7 is
    asked for on the first-block positions and on every ninth descriptor."""
    out, i = [], 0
    while i < L:
        two = len(out) % 3 == 0 and i + 1 < L and not ({i, i + 1} & set(FIRST_BLOCK))
        out.append((2 if two else 1, 7 if (i in FIRST_BLOCK or i % 9 == 4) else 1))
        i += out[-1][0]
    return out


def wave_border(L):
    """Rule k alone receives L descriptors in call k.  Rules 0-3 (sampleCount 1,
    1 s) have the count that makes descriptor FIRST_BLOCK[k] the first blocked
    one; it asks for 7, so descriptors asking for 1 pass after it.  Times
    advance 3 ms per descriptor from 600 ms into a window: the first bucket
    boundary falls on descriptor 134 or 135, inside the chunk [128, 192).  Rules 4 and
    5 have 10 and 2 buckets (boundaries every 34 / 167 descriptors)."""
    shape = _border_requests(L)
    per_desc = [h for n, h in shape for _ in range(n)]
    assert len(per_desc) == L
    flow, calls = [], []
    for k in range(6):
        dom = f"border{k}"
        if k < 4:
            p = min(FIRST_BLOCK[k], L - 1)
            count = sum(per_desc[:p]) + per_desc[p] - 1
            flow.append(flow_rule(rm.generate_key(dom, [("k", "v")]), count))
        else:
            flow.append(flow_rule(rm.generate_key(dom, [("k", "v")]), 20, sample_count=(10, 2)[k - 4]))
        base = (k + 1) * 10_000 + 600
        reqs, d = [], 0
        for n, h in shape:
            reqs.append((dom, [[("k", "v")]] * n, h, base + 3 * d))
            d += n
        calls.append(("rls", reqs))
    return Case(f"border_{L}", flow, calls)


def pass_after_block_in_chunk(res, wl=1000, ts=None):
    """A descriptor that passes right after a blocked one, both in one chunk of the first window."""
    c = res.code
    for i in range(len(c) - 1):
        if c[i] == abi.RLS_OVER_LIMIT and c[i + 1] == abi.RLS_OK and i % CHUNK != CHUNK - 1 and \
                (ts is None or ts[i] // wl == ts[i + 1] // wl):
            return True
    return False


def guard_border(case, ref, L, stats=None):
    lane, wave = routes(case, ref)
    assert (wave > 0) == (L >= WAVE_MIN) and lane + wave == 6
    if L >= WAVE_MIN:
        assert any(pass_after_block_in_chunk(r) for r in ref.results[:4])
    if L > 1:
        assert all({abi.RLS_OK, abi.RLS_OVER_LIMIT} <= set(r.code.tolist()) for r in ref.results[1:4])
    if stats is not None:
        assert (stats.segs_lane, stats.segs_wave) == (lane, wave)
        if L >= WAVE_MIN:
            assert stats.rounds > stats.chunks > 0


def old_window():
    """A call whose ts_ms lie in a window older than the rule's bucket (left by
    the call before): LeapArray.currentWindow hands out a throwaway bucket, so
    sums are read and nothing is added."""
    L = WAVE_MIN + 44
    flow = [flow_rule(rm.generate_key("old", [("k", "v")]), 50)]
    now = [("old", [[("k", "v")]], 1, 5600 + i) for i in range(40)]
    old = [("old", [[("k", "v")]], 1, 4600 + i // 2) for i in range(L)]
    return Case("old_window", flow, [("rls", now), ("rls", old), ("rls", [("old", [[("k", "v")]], 1, 5700)])])


def guard_old_window(case, ref, stats=None):
    first, old, after = ref.results
    assert int((first.code == abi.RLS_OK).sum()) == 40
    # nothing was added by the old call: each of its descriptors saw the same sum, so all pass with one remaining
    assert set(old.code.tolist()) == {abi.RLS_OK} and set(old.remaining.tolist()) == {9}
    assert after.remaining[0] == 9
    if stats is not None:
        assert stats.chunks_serial > 0 or stats.segs_wave == 0


# ---------------------------------------------------------------- 3. strings
CODE_POINTS = ["a", "é", "€", "\U0001F600"]          # 1, 2, 3 and 4 bytes of UTF-8


def strings():
    keys = []
    for first in CODE_POINTS:
        for last in CODE_POINTS:
            s = first + "mid" + last
            keys.append((s, [(s + "k", s + "v")]))
    keys += [("dom", [("k", "")]), ("", [("k", "v")]), ("only-domain", []), ("dom", [("", "")]),
             ("dom", [("k1", "v1"), ("k2", "v2"), ("k3", "v3")])]
    flow = [flow_rule(rm.generate_key(d, e), 3) for d, e in keys]
    # a rule whose id is the hash of a whitespace-only key: the key is blank, so it is never looked up
    blank = " \t\u2003\u3000\u001f"
    flow.append(flow_rule(None, 3, flow_id=rm.INT_MAX + rm.java_hash(blank)))
    flow.append(flow_rule(None, 3, flow_id=rm.INT_MAX))         # ... and of the empty key (hash 0)
    reqs, t = [], 50_000
    for rep in range(5):
        for d, e in keys:
            reqs.append((d, [e, e] if rep == 0 else [e], 1, t))
            t += 1
        reqs.append((blank, [[]], 1, t))
        reqs.append(("", [[], [("k", "v")]], 1, t))
        # U+00A0, U+2007, U+202F and U+180E are not Java whitespace: such a key is not blank (and has no rule)
        reqs.append(("\u00a0", [[]], 1, t))
        reqs.append(("\u180e\u2007\u202f", [[]], 1, t))
    good = keys[0]
    for name, raw in ILL_FORMED.items():
        # in a domain, and in the last entry of the last descriptor: well-formed siblings come first
        reqs.append((raw, [good[1], keys[5][1]], 1, t))
        reqs.append((good[0], [good[1], keys[5][1], [("k", "v"), ("last", raw)]], 1, t))
        reqs.append((good[0], [[(raw, "v")], good[1]], 1, t))
        t += 1
    reqs.append((good[0], [good[1]], 1, t))
    return Case("strings", flow, [("rls", reqs)])


def guard_strings(case, ref, stats=None):
    res = ref.results[0]
    reqs = case.calls[0][1]
    n_bad = 3 * len(ILL_FORMED)
    assert int((res.overall == abi.RLS_ERROR).sum()) == n_bad
    blank_ids = {f.flow_id for f in case.flow[-2:]}
    d = 0
    for dom, descs, _, _ in reqs:
        for e in descs:
            if isinstance(dom, str) and not e and rm.is_blank(dom):
                assert res.flow_id[d] == -1 and res.limit[d] == abi.RLS_NO_LIMIT
            d += 1
    assert not (set(res.flow_id.tolist()) & blank_ids)
    # every keyed rule was reached, passed 3 times and then blocked
    for f in case.flow[:-2]:
        sel = res.flow_id == f.flow_id
        assert int((res.code[sel] == abi.RLS_OK).sum()) == 3 and int((res.code[sel] == abi.RLS_OVER_LIMIT).sum()) >= 1
    if stats is not None:
        assert stats.error_requests == n_bad


# ---------------------------------------------------------------- 4. shared state
def shared():
    """sf_request_tokens and sf_request_rls interleaved on the same flowIds.
    Namespace 1 has a limiter of 1 request per second and 3 connected clients.
    Rule A is GLOBAL 10, rule B AVG_LOCAL 4 (the token path allows 12, the
    rate-limit path 4).  A prioritized token request occupies the next window
    (SHOULD_WAIT) and the rate-limit call after the roll sees the transfer."""
    ns = [abi.sf_namespace(1, 3, 1.0)]
    ka, kb = rm.generate_key("shared", [("k", "a")]), rm.generate_key("shared", [("k", "b")])
    a = flow_rule(ka, 10, sample_count=10, ns=1)
    b = flow_rule(kb, 4, sample_count=10, ns=1, threshold_type=abi.THRESHOLD_AVG_LOCAL)
    da, db = [("k", "a")], [("k", "b")]

    def tok(rows):
        return abi.HostTokenBatch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])

    P = abi.TOK_PRIORITIZED
    calls = [
        ("rls", [("shared", [da, db], 1, 10_000 + i) for i in range(12)]),              # A and B filled in bucket 0
        ("tok", tok([(a.flow_id, 1, P, 10_950), (b.flow_id, 1, 0, 10_951), (a.flow_id, 1, P, 10_952)])),
        ("rls", [("shared", [da, db], 1, 11_000 + 40 * i) for i in range(20)]),         # the roll: occupy transfers
        ("tok", tok([(b.flow_id, 3, 0, 12_200), (a.flow_id, 1, 0, 12_201)])),
        ("rls", [("shared", [db, da, db], 2, 12_300 + i) for i in range(8)]),
        ("tok", tok([(a.flow_id, 2, P, 13_900), (b.flow_id, 1, P, 13_901)])),
        ("rls", [("shared", [da], 0, 14_000 + i) for i in range(15)]),
    ]
    return Case("shared", [a, b], calls, namespaces=ns)


def guard_shared(case, ref, so):
    toks = [r for (k, _), r in zip(case.calls, ref.results) if k == "tok"]
    assert toks[0].status.tolist() == [abi.TOKEN_SHOULD_WAIT, abi.TOKEN_TOO_MANY_REQUEST, abi.TOKEN_TOO_MANY_REQUEST]
    # what the token path gives for the same descriptor stream (the real namespace table throughout)
    o = so.OracleEngine(case.config())
    o.load_namespaces(case.namespaces)
    o.load_cluster_rules(case.flow)
    differ = 0
    for (kind, arg), res in zip(case.calls, ref.results):
        if kind == "tok":
            o.request_tokens(arg)
            continue
        flat = [(rm.generate_flow_id(rm.generate_key(dom, e)), h or 1, 0, t) for dom, descs, h, t in arg for e in descs]
        got = o.request_tokens(abi.HostTokenBatch(*zip(*flat)))
        differ += int(((got.status == abi.TOKEN_OK) != (res.code == abi.RLS_OK)).sum())
    assert differ > 0
