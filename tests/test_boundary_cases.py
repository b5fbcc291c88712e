"""The border workloads of tests/boundary_cases.py on the CPU: the constants
the cases are built around against the source text, every coverage guard
(computed from the batch and the oracle's verdicts), and the host build of the
interpreter against the oracle on every case (verdicts, waits, rule indices,
node rows, rule states).  The GPU twin is tests/test_gpu_boundary.py.

The host build shares sf_decide.h and the routing and window algorithms of
sf_heavy.h with the kernels; its team has one lane, so team_first_true is a
binary search here and the rings of sf_stream.h do not exist: those borders
are only reached on the GPU, which is what the guards are for."""
import numpy as np
import pytest

from sentinel_amd import abi
from tests import boundary_cases as bc
from tests import workloads


def test_constants_match_the_source():
    """A retune of a tile, ring or threshold moves the borders: move the cases with it."""
    assert bc.source_constants() == bc.MIRROR
    assert bc.RUN_FAR == 8191 and bc.LX_SPLIT == 131_008
    assert bc.acc_cap(3456, 8) == 65_536 and bc.acc_cap(1 << 20) == 131_072 and bc.acc_cap(1 << 30, 2) == 1 << 24
    assert [bc.sort_digits(r) for r in bc.KEY_RESOURCES] == [(1, 1), (1, 1), (1, 8), (2, 5), (2, 8), (3, 6)]


def test_placement_covers_every_border():
    got = bc.placement_straddles()
    want = {(k, B) for k in bc.HEAVY_KINDS for B in bc.BORDERS}
    assert want <= got, sorted(want - got)


@pytest.fixture(scope="module")
def hs():
    from tests.hostsim import hostsim
    hostsim.lib()
    return hostsim


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_guard_and_host_build(hs, so, name):
    make, guard = bc.CASES[name]
    w = make()
    for b in w["batches"]:
        assert np.all(np.diff(b.ts_ms) >= 0)
    st, wait = bc.oracle_status(so, w)
    print(name, guard(w, st, wait))
    eng = ora = None
    try:
        eng, ora, _ = workloads.run(hs.HostSimEngine, so.OracleEngine, w)
    finally:
        for x in (eng, ora):
            if x is not None:
                x.close()


def test_rule_state_index_counts_loaded_rules(hs, so):
    """read_rule_state(k) addresses the k-th rule the loader kept, in the
    host build as in the oracle: a rule FlowRuleUtil.isValidRule rejects (a
    RateLimiter rule without maxQueueingTimeMs, a WarmUp rule without a period)
    takes no index, so a workload's n_flow counts valid rules, whatever the
    number of resources without a rule."""
    rules = [bc._qps(0, 5), abi.sf_flow_rule(resource=1, grade=abi.GRADE_QPS, count=5.0,
                                             control_behavior=abi.BEHAVIOR_RATE_LIMITER),
             abi.sf_flow_rule(resource=2, grade=abi.GRADE_QPS, count=5.0, control_behavior=abi.BEHAVIOR_WARM_UP),
             bc._rl(4, 100, 7)]
    cfg = abi.default_config(max_resources=6, max_batch=64)
    e, o = hs.HostSimEngine(cfg), so.OracleEngine(cfg)
    e.load_flow_rules(rules)
    o.load_flow_rules(rules)
    ts = bc.T0 + np.arange(40, dtype=np.int64)
    b = abi.HostBatch(np.full(40, 4, np.uint32), ts, np.ones(40, np.int32), np.full(40, abi.EV_IN, np.uint8))
    e.submit(b)
    o.submit(b)
    try:
        _check_rule_state_indices(e, o)
    finally:
        e.close()
        o.close()


def _check_rule_state_indices(e, o):
    for k in range(2):
        x, y = e.read_rule_state(k), o.read_rule_state(k)
        assert (x.stored_tokens, x.last_filled_time, x.latest_passed_time) == \
               (y.stored_tokens, y.last_filled_time, y.latest_passed_time)
    assert e.read_rule_state(1).latest_passed_time >= bc.T0          # index 1 is the fourth rule of the list
    with pytest.raises(AssertionError):
        e.read_rule_state(2)
    with pytest.raises(AssertionError):
        o.read_rule_state(2)
