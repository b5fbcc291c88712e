"""The breaker border workloads of tests/degrade_cases.py on the CPU: the
constants the cases are built around against the source text, every case's
guard (the input sits on the border it names), oracle/degrade.py against the C
oracle's slot chain on every case (the two independent restatements of the
reference: verdicts, breaker indices, breaker states), the host build of the
engine's decision code against the C oracle on the chain cases, the
hand-derived expectations (thresholds, the recovery time's Java int
arithmetic) and the registry meta-check.  The GPU twin is
tests/test_gpu_degrade_cases.py."""
import numpy as np
import pytest

from oracle import degrade as od
from sentinel_amd import abi
from tests import degrade_cases as dc
from tests import degrade_chain_cases as cc
from tests.test_degrade_chain import _breaker_rows
from tests.test_golden import _state_row

_PROVED = {}


def test_constants_match_the_source():
    """A retune of HEAVY, MAXC, the grid cap or the breaker limit moves the borders: move the cases with it."""
    assert dc.source_constants() == dc.MIRROR


def c_chain(so, c):
    """The C oracle's chain with the case's degrade rules alone."""
    o = so.OracleEngine(abi.default_config(max_resources=c["R"], max_batch=max(b.n for b in c["batches"])))
    try:
        n = o.load_degrade_rules(c["rules"])
        outs = [o.submit(b) for b in c["batches"]]
        return n, outs, _breaker_rows(o, n)
    finally:
        o.close()


def check_oracles_agree(so, c, an):
    n, outs, rows = c_chain(so, c)
    assert n == len(an["states"])
    for k, (v, st, ri) in enumerate(zip(outs, an["status"], an["rule_idx"])):
        bad = np.nonzero(v.status != st)[0]
        assert bad.size == 0, f"batch {k}: {bad.size} verdicts differ, first at {bad[:5]}"
        blk = st == od.V_BLOCK_DEGRADE
        assert np.array_equal(v.rule_idx[blk], ri[blk]), f"batch {k}: breaker index"
        assert np.all(v.wait_ms == 0)
    want = np.array([_state_row(s) for s in an["states"]], np.int64).reshape(n, 5)
    assert np.array_equal(rows, want), np.nonzero((rows != want).any(axis=1))[0][:8]


@pytest.mark.parametrize("name", list(dc.CASES))
def test_case_guard_and_oracles(so, name):
    build, guard = dc.CASES[name]
    c = build()
    last = 0
    for b in c["batches"]:
        assert b.ts_ms[0] >= last and np.all(np.diff(b.ts_ms) >= 0) and b.ts_ms[0] >= 0
        last = b.ts_ms[-1]
        ex = (b.flags & abi.EV_EXIT) != 0                      # exits after the entries of their millisecond
        same = (b.ts_ms[1:] == b.ts_ms[:-1]) & (b.res_id[1:] == b.res_id[:-1])
        assert not np.any(same & ex[:-1] & ~ex[1:])
    an = dc.analyze(c)
    _PROVED[name] = guard(c, an)
    print(name, sum(b.n for b in c["batches"]), "events", sorted(_PROVED[name]))
    check_oracles_agree(so, c, an)


def test_registry_covers_every_path():
    """Over the whole registry some guard reports each walk, each of the four
    entry-lookup routes of the wave walk, and each kind of transition both as
    the cut of a bulk prefix and inside the serial walk."""
    got = set()
    for name, (build, guard) in dc.CASES.items():
        if name not in _PROVED:
            c = build()
            _PROVED[name] = guard(c, dc.analyze(c))
        got |= _PROVED[name]
    assert dc.PROPS <= got, sorted(dc.PROPS - got)
    for fam in ("seg_lengths", "first_change_lane", "window_rolls", "thresholds", "retry_and_probe", "ignored_exits",
                "batch_cuts", "many_segments", "key_widths"):
        assert any(n.startswith(fam) and _PROVED[n] for n in dc.CASES), fam


# ---------------------------------------------------------------- literal expectations
def test_recovery_time_is_java_int_arithmetic():
    """recoveryTimeoutMs = timeWindow * 1000 wraps (AbstractCircuitBreaker.java:36,54): literals, no oracle."""
    for tw, ms in dc.RECOVERY_MS.items():
        assert od.Breaker(dc.rule(0, dc.COUNT, 0, tw=tw)).recovery == ms, tw
    assert dc.RECOVERY_MS == {2147483: 2147483000, 2147484: -2147483296, 4294967: -296, 4294968: 704,
                              2147483647: -1000}


def test_recovery_time_python_oracle():
    c = dc.recovery()
    an = dc.analyze(c)
    got = dc.recovery_observed(c, an["status"][0], lambda k: an["states"][k]["next_retry_ms"])
    assert got == dc.recovery_expect()


@pytest.mark.parametrize("which", ["c_oracle", "hostsim"])
def test_recovery_time_chain(so, which):
    """The same literals on the C oracle's chain and on the host build of the
    engine's decision code (it shares make_dev_breaker_rule with the GPU loader)."""
    c = dc.recovery()
    if which == "c_oracle":
        make = so.OracleEngine
    else:
        from tests.hostsim import hostsim
        make = hostsim.HostSimEngine
    e = make(abi.default_config(max_resources=c["R"], max_batch=c["full"].n))
    try:
        assert e.load_degrade_rules(c["rules"]) == len(dc.RECOVERY_MS)
        v = e.submit(c["batches"][0])
        got = dc.recovery_observed(c, v.status, lambda k: e.read_breaker(k).next_retry_ms)
    finally:
        e.close()
    assert got == dc.recovery_expect()


def test_thresholds_c_oracle_literals(so):
    c = dc.thresholds()
    _, outs, _ = c_chain(so, c)
    assert dc.threshold_verdicts(c, outs[0].status, outs[0].rule_idx) == dc.threshold_expect()


# ---------------------------------------------------------------- the chain cases
@pytest.fixture(scope="module")
def hs():
    from tests.hostsim import hostsim
    hostsim.lib()
    return hostsim


@pytest.mark.parametrize("name", list(cc.CASES))
def test_chain_case_guard_and_host_build(hs, so, name):
    build, guard = cc.CASES[name]
    w = build()
    for b in w["batches"]:
        assert np.all(np.diff(b.ts_ms) >= 0) and b.ts_ms[0] >= 0
    print(name, guard(w, cc.oracle_run(so, w)))
    eng = ora = None
    try:
        eng, ora = cc.run(hs.HostSimEngine, so.OracleEngine, w)
    finally:
        for x in (eng, ora):
            if x is not None:
                x.close()
