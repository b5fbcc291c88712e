"""GPU: the embedded token server (sf_load_cluster_binds) -- cluster-mode flow
rules that take their tokens from the engine's own token server inside
sf_submit*.  Exact against the serial model (tests/embedded_model.py; its known
answers and the reachability of the traffic: tests/test_embedded_model.py,
tests/embedded_cases.py) and, where the chain holds what the model does not
(ParamFlow, a SystemRule, a circuit breaker), against the whole-chain oracle.
Run with -m gpu on an MI355X."""
import itertools

import numpy as np
import pytest

from sentinel_amd import abi
from tests import embedded_cases as ec
from tests import embedded_model as em
from tests import parity, workloads
from tests.token_cases import frule, nsp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


def make_engine(eng_mod, config, tabs, order=("ns", "cluster", "flow", "binds")):
    rules, binds, namespaces, crules = tabs
    e = eng_mod.FlowEngine(config)
    for what in order:
        if what == "ns":
            e.load_namespaces(namespaces)
        elif what == "cluster":
            e.load_cluster_rules(flow=crules)
        elif what == "flow":
            e.load_flow_rules(rules)
        else:
            e.load_cluster_binds(binds)
    return e


def compare_state(e, m, config, flow_ids, now, what):
    for res in range(config.max_resources):
        em.compare_node(e.read_node(res), m.node_state(res), config.sample_count, f"{what}: node {res}")
    for fid in flow_ids:
        got = [e.cluster_sum(fid, ev, now) for ev in range(7)]
        assert got == m.cluster_sums(fid, now), f"{what}: ClusterMetric sums of flowId {fid}"


def host_verdicts(dv, n):
    got = abi.HostVerdicts(n)
    got.status, got.wait_ms, got.rule_idx = dv.status.numpy(), dv.wait_ms.numpy(), dv.rule_idx.numpy()
    return got


# ---------------------------------------------------------------- 1. parity with the model, random traces
_model = {}


def model_of(so):
    """The model's replay of the mixed trace, computed once."""
    if not _model:
        case = ec.random_case(7)
        m, outs, tail = ec.run_model(case)
        ec.reach(m, outs)
        _model.update(case=case, m=m, outs=outs, tail=tail)
    return _model


@pytest.mark.parametrize("path", ["submit", "async", "packed"])
def test_model_parity_random(eng_mod, so, path):
    """About 4k events over 8 resources, 3 loaded flowIds (one bound from two resources, two in a
    namespace with a limiter) and two that are not loaded: verdicts, waits, rule indices, every
    ClusterNode, the 7 ClusterMetric sums per flowId, and a trailing sf_request_tokens batch that
    pins the limiter and the occupy state, through sf_submit, sf_submit_async and a packed form."""
    k = model_of(so)
    case, m = k["case"], k["m"]
    config, tabs = ec.cfg(), ec.tables()
    e = make_engine(eng_mod, config, tabs)
    if path == "submit":
        got = [e.submit(b) for b in case["batches"]]
    elif path == "packed":
        got = [e.submit_packed(abi.PackedBatch(b)) for b in case["batches"]]
    else:
        dbs = [eng_mod.DeviceBatch(e, b) for b in case["batches"]]
        dvs = [eng_mod.DeviceVerdicts(e, b.n, with_wait=True, with_rule=True) for b in case["batches"]]
        for db, dv in zip(dbs, dvs):
            e.submit_device_async(db, dv)
        # (no sync: the token call below has to wait for the batches in flight itself)
    tail = e.request_tokens(case["tail"])
    if path == "async":
        e.sync()
        got = [host_verdicts(dv, b.n) for dv, b in zip(dvs, case["batches"])]
    for i, (g, w) in enumerate(zip(got, k["outs"])):
        parity.compare_verdicts(g, w, f"{path} batch {i}")
    assert (tail.status == k["tail"].status).all() and (tail.wait_ms == k["tail"].wait_ms).all() and \
        (tail.remaining == k["tail"].remaining).all(), "the trailing token batch differs from the model's server"
    compare_state(e, m, config, (101, 102, 201, 999), case["t_end"], path)
    e.close()


# ---------------------------------------------------------------- 2. differentials against the whole-chain oracle
def chain_workload():
    """ParamFlow rules, IN entries with exits and a flow rule on every even resource
    (workloads.param_mixed), a QPS SystemRule and a slow-call breaker on top; then a cluster-mode
    rule last on resources 0..7 (FlowRuleComparator sorts cluster rules last)."""
    w = workloads.param_mixed(seed=23, R=12, n=4000)
    b = w["batches"][0]
    w["system"] = [abi.sf_system_rule(highest_system_load=-1, highest_cpu_usage=-1, qps=40.0, avg_rt=-1,
                                      max_thread=-1)]
    w["degrade"] = [abi.degrade_rule(r, abi.DEGRADE_GRADE_RT, 30, 1, min_request_amount=3, slow_ratio_threshold=0.4)
                    for r in (1, 2, 9)]
    assert b.n > 4000
    return w


def run_chain(eng_mod, so, w, eng_flow, ora_flow, binds, crules):
    e, ora = eng_mod.FlowEngine(w["cfg"]), so.OracleEngine(w["cfg"])
    for x in (e, ora):
        x.set_system_status(0.0, 0.0)
        x.load_system_rules(list(w["system"]))
    e.load_namespaces([nsp(1)])
    e.load_cluster_rules(flow=crules)
    e.load_flow_rules(eng_flow)
    ora.load_flow_rules(ora_flow)
    for x in (e, ora):
        x.load_param_rules(list(w["param"]), list(w["items"]))
        assert x.load_degrade_rules(list(w["degrade"])) == len(w["degrade"])
    e.load_cluster_binds(binds)
    outs = []
    for i, b in enumerate(w["batches"]):
        g, o = e.submit(b), ora.submit(b)
        parity.compare_verdicts(g, o, f"batch {i}")
        outs.append(o)
    parity.compare_all_nodes(e, ora, w["cfg"].max_resources, sample_count=w["cfg"].sample_count)
    parity.compare_entry_node(e, ora, sample_count=w["cfg"].sample_count)
    st = np.concatenate([o.status for o in outs])
    for v in (abi.V_BLOCK_PARAM, abi.V_BLOCK_SYSTEM, abi.V_BLOCK_DEGRADE, abi.V_PASS):
        assert (st == v).any(), f"the workload never reaches verdict {v}"
    return e, st


def with_cluster(w, count, fallback, cluster=True):
    n0 = len(w["flow"])
    extra = [em.flow_rule(r, count, cluster=cluster, fallback=fallback) for r in range(8)]
    return list(w["flow"]) + extra, [(n0 + r, 500 + r) for r in range(8)]


def test_chain_huge_threshold_equals_no_fallback(eng_mod, so):
    """Every request is OK: the bound rule passes, as a cluster rule without fallback does today.
    The bound rule is the last flow rule, so exactly the entries that pass or are stopped by the
    breaker have taken a token: PASS_REQUEST of the flowId (one 60-s window) counts them."""
    w = chain_workload()
    flow, binds = with_cluster(w, 1, fallback=False)
    e, st = run_chain(eng_mod, so, w, flow, flow, binds, [frule(500 + r, 1e9, I=60_000) for r in range(8)])
    b = w["batches"][0]
    took = np.isin(st, (abi.V_PASS, abi.V_PASS_WAIT, abi.V_BLOCK_DEGRADE))
    for r in range(8):
        want = int((took & (b.res_id == r)).sum())
        assert want > 5 and e.cluster_sum(500 + r, 2, int(b.ts_ms[-1])) == want, f"requests of resource {r}"
    e.close()


@pytest.mark.parametrize("fallback", [False, True])
def test_chain_flow_id_not_loaded_equals_todays_fallback(eng_mod, so, fallback):
    w = chain_workload()
    flow, binds = with_cluster(w, 4, fallback=fallback)
    e, st = run_chain(eng_mod, so, w, flow, flow, binds, [frule(77, 5)])
    assert (st == abi.V_BLOCK_FLOW).any()
    e.close()


def test_chain_server_count_zero_equals_local_count_zero(eng_mod, so):
    """count 0 on the server, no prioritized entry, every acquireCount 1: each request is BLOCKED,
    which is what a local Default QPS rule of count 0 at the same list position decides."""
    w = chain_workload()
    flow, binds = with_cluster(w, 7, fallback=False)
    ora_flow, _ = with_cluster(w, 0, fallback=False, cluster=False)
    e, st = run_chain(eng_mod, so, w, flow, ora_flow, binds, [frule(500 + r, 0) for r in range(8)])
    assert (st == abi.V_BLOCK_FLOW).sum() > 100
    e.close()


# ---------------------------------------------------------------- 3. borders of one hot resource
def one_resource(eng_mod, so, events, crule, ns=None, local=3, before=None, config=None):
    """One resource with one bound rule -> flowId 101: exact against the model.  Returns the
    model's statuses, the model and (wave chunks, serial chunks) of k_decide_xcl (sf_stats)."""
    config = config or ec.cfg()
    tabs = ([em.flow_rule(0, local, cluster=True)], [(0, 101)], ns or [nsp(1, connected=3)], [crule])
    hb = abi.HostBatch([0] * len(events), [t for t, _, _ in events], [c for _, c, _ in events], [f for _, _, f in events],
                       entry_ref=[-1] * len(events))
    m = em.EmbeddedModel(config, *tabs)
    e = make_engine(eng_mod, config, tabs)
    if before is not None:                                   # a token request of a remote client first
        tb = abi.HostTokenBatch([101], [1], [0], [before])
        assert e.request_tokens(tb).status[0] == m.srv.request_tokens(tb).status[0]
    want = m.submit(hb)
    parity.compare_verdicts(e.submit(hb), want, "one resource")
    t_end = max(int(hb.ts_ms[-1]), before or 0)
    compare_state(e, m, config, (101,), t_end, "one resource")
    stats = e.stats()
    e.close()
    return want.status, m, (int(stats.xcl_chunks_wave), int(stats.xcl_chunks_serial))


def burst(t, n, c=1, fl=0):
    return [(t, c, fl)] * n


XCL_MIN = 256            # sf_xflow.h: the shortest segment k_decide_xcl takes
FILL = burst(29_000, XCL_MIN)     # makes a short case a segment the wave route takes (a window of its own, 4 chunks)


def chunks(events, wl, sec=500):
    """Chunks of the wave route: runs of at most 64 events inside one ClusterMetric window, one
    second bucket of the node (``sec`` ms) and one minute bucket (1 s)."""
    n, k = 0, 0
    key = lambda t: (t // wl, t // sec, t // 1000)  # noqa: E731
    while k < len(events):
        w = key(events[k][0])
        j = k
        while j < len(events) and j - k < 64 and key(events[j][0]) == w:
            j += 1
        n, k = n + 1, j
    return n


@pytest.mark.parametrize("n", [XCL_MIN - 1, XCL_MIN, XCL_MIN + 1])
def test_segment_lengths_around_the_minimum(eng_mod, so, n):
    """A segment one short of XCL_MIN stays on k_decide_x's lane (no chunk counted); XCL_MIN and
    XCL_MIN + 1 take k_decide_xcl (4 and 5 chunks of one window).  The threshold (40) is hit
    exactly inside the first chunk (nextRemaining == 0)."""
    st, m, route = one_resource(eng_mod, so, burst(20_010, n), frule(101, 40), local=0)
    assert (st == abi.V_PASS).sum() == 40 and (st == abi.V_BLOCK_FLOW).sum() == n - 40
    assert m.cluster_sums(101, 20_010)[:4] == [40, n - 40, 40, n - 40]
    assert route == ((0, 0) if n < XCL_MIN else ((n + 63) // 64, 0))


@pytest.mark.parametrize("n", [63, 64, 65])
def test_chunk_lengths(eng_mod, so, n):
    """63 / 64 / 65 events inside one window (then a second window): chunks of 63; 64; 64 + 1."""
    ev = burst(20_010, n, c=2) + burst(20_100, XCL_MIN - n)
    st, _, route = one_resource(eng_mod, so, ev, frule(101, 100), local=0)
    assert (st[:n] == abi.V_PASS).sum() == 50 and route == (chunks(ev, 100), 0)
    assert route[0] == {63: 5, 64: 4, 65: 5}[n]


@pytest.mark.parametrize("S,I", [(10, 1000), (4, 1000), (2, 600)])
def test_window_borders(eng_mod, so, S, I):
    """Events at k * wl - 1 and k * wl over more than one interval: buckets roll and expire.  With
    sample_count 4 the 500-ms border of the node's second window is a cluster-window border only
    every other time; with wl 300 a cluster-window border is no second-bucket border."""
    wl = I // S
    ev = []
    for k in range(20_000 // wl, 20_000 // wl + 2 * S + 3):
        ev += burst(k * wl - 1, 20) + burst(k * wl, 20, c=2)
    assert len(ev) >= XCL_MIN
    st, _, route = one_resource(eng_mod, so, ev, frule(101, 12, S=S, I=I), local=0)
    assert (st == abi.V_PASS).any() and (st == abi.V_BLOCK_FLOW).any() and route == (chunks(ev, wl), 0)


def test_gap_longer_than_the_interval(eng_mod, so):
    ev = burst(20_000, 100) + burst(20_950, 60) + burst(23_500, 100) + burst(23_501, 20)
    st, _, route = one_resource(eng_mod, so, ev, frule(101, 6), local=0)
    assert st.tolist() == [0] * 6 + [3] * 94 + [3] * 60 + [0] * 6 + [3] * 94 + [3] * 20
    assert route == (2 + 1 + 2, 0)                           # (23 500 and 23 501 share a window)


def test_smaller_count_passes_after_a_larger_one_blocked(eng_mod, so):
    ev = [(20_000, 3, 0), (20_000, 3, 0), (20_001, 3, 0), (20_001, 1, 0), (20_002, 2, 0), (20_002, 1, 0), (20_003, 1, 0)]
    st, _, route = one_resource(eng_mod, so, ev + FILL, frule(101, 8), local=0)
    assert st[:7].tolist() == [0, 0, 3, 0, 3, 0, 3]          # 3 + 3, 3 blocked, + 1 = 7, 2 blocked, + 1 = 8, full
    assert route == (1 + 4, 0)


def test_prioritized_and_zero_count_entries(eng_mod, so):
    """Prioritized entries occupy the next window (SHOULD_WAIT) once the head bucket leaves;
    acquireCount 0 is a BAD_REQUEST and falls back to the local rule.  Their chunks are replayed
    by lane 0 (the windows 20 900 and 21 000); the others are solved by the wavefront."""
    ev = burst(20_000, 5) + burst(20_500, 2) + [(20_900, 0, 0)] + burst(20_900, 4, fl=abi.EV_PRIO) + \
        burst(20_901, 2) + burst(21_000, 3) + burst(21_001, 3, fl=abi.EV_PRIO)
    st, m, route = one_resource(eng_mod, so, ev + FILL, frule(101, 5), local=100)
    kinds = {c for c, _ in m.trace}
    assert {em.OK, em.BLOCKED, em.SHOULD_WAIT, em.BAD_REQUEST} <= kinds and (st == abi.V_PASS_WAIT).any()
    assert route == (2 + 4, 2)


def test_remote_request_at_a_later_time_gives_the_throwaway_bucket(eng_mod, so):
    """A remote client's sf_request_tokens at 21 050 rolls bucket 0 forward; the chain's entries
    at 20 050 then find a window older than the bucket (LeapArray.currentWindow's throwaway case):
    that chunk is replayed serially, the window 20 150 is solved by the wavefront."""
    ev = burst(20_050, 6) + burst(20_150, XCL_MIN)
    st, _, route = one_resource(eng_mod, so, ev, frule(101, 4), local=0, before=21_050)
    assert (st == abi.V_PASS).any() and route == (4, 1)


@pytest.mark.parametrize("connected,passes", [(0, 0), (3, 6)])
def test_avg_local_threshold(eng_mod, so, connected, passes):
    st, _, route = one_resource(eng_mod, so, burst(20_000, 300), frule(101, 2, tt=abi.THRESHOLD_AVG_LOCAL),
                                ns=[nsp(1, connected=connected)], local=0)
    assert (st == abi.V_PASS).sum() == passes and route == (5, 0)


def test_exits_and_blocked_entries_in_wave_chunks(eng_mod, so):
    """Exits and SF_EV_BLOCKED entries inside wave chunks make no request and keep their verdict."""
    case_b = ec.trace(77, 400, 20_000, 900, res=0, prio_p=0.0, zero_p=0.0, blocked_p=0.1, exit_p=0.5)
    config = ec.cfg()
    tabs = ([em.flow_rule(0, 3, cluster=True)], [(0, 101)], [nsp(1)], [frule(101, 30)])
    m = em.EmbeddedModel(config, *tabs)
    want = m.submit(case_b)
    assert (want.status == abi.V_EXIT).any() and (want.status == abi.V_EXIT_IGNORED).any() and \
        (want.status == abi.V_BLOCK_OTHER).any() and (want.status == abi.V_BLOCK_FLOW).any()
    e = make_engine(eng_mod, config, tabs)
    parity.compare_verdicts(e.submit(case_b), want, "exits in wave chunks")
    compare_state(e, m, config, (101,), int(case_b.ts_ms[-1]), "exits in wave chunks")
    s = e.stats()
    assert s.xcl_chunks_wave >= 9 and s.xcl_chunks_serial == 0
    e.close()


def test_bound_chain_rule_keeps_its_context_node(eng_mod, so, monkeypatch):
    """A bound CHAIN rule: every entry and exit of the named context is accounted on the
    (context, resource) DefaultNode, so the segment stays on the lane (no wave chunk) however long
    it is.  With a threshold every request passes the whole-chain oracle decides the same (the rule
    as cluster-mode without fallback); with a low one the default engine and one with the minimum
    raised agree on verdicts, ClusterNode and context node."""
    b = ec.trace(78, 500, 20_000, 900, res=0, prio_p=0.0, zero_p=0.0, blocked_p=0.05, exit_p=0.5)
    rng = np.random.default_rng(3)
    ctx = rng.choice([3, 5], b.n).astype(np.uint32)
    ex = b.entry_ref >= 0
    ctx[ex] = ctx[b.entry_ref[ex]]
    hb = abi.HostBatch(b.res_id, b.ts_ms, b.count, b.flags, entry_ref=b.entry_ref, context=ctx)
    rule = abi.sf_flow_rule(resource=0, grade=abi.GRADE_QPS, count=5.0, strategy=abi.STRATEGY_CHAIN, control_behavior=0,
                            warm_up_period_sec=10, max_queueing_time_ms=500, cluster_mode=1, ref_resource=3,
                            limit_app=abi.APP_DEFAULT, cluster_fallback=0)
    config = ec.cfg()

    def run(count):
        e = make_engine(eng_mod, config, ([rule], [(0, 101)], [nsp(1)], [frule(101, count)]))
        out = e.submit(hb)
        s = e.stats()
        assert (int(s.xcl_chunks_wave), int(s.xcl_chunks_serial)) == (0, 0)
        return e, out
    e, got = run(1e9)
    ora = so.OracleEngine(config)
    ora.load_flow_rules([rule])
    parity.compare_verdicts(got, ora.submit(hb), "bound CHAIN rule, every request OK")
    parity.compare_nodes(e, ora, [0])
    parity.compare_aux_nodes(e, ora, context_nodes=[(3, 0)])
    assert e.read_context_node(3, 0).cur_thread_num >= 0 and e.cluster_sum(101, 2, int(hb.ts_ms[-1])) > 0
    e.close()
    e1, out1 = run(20)
    monkeypatch.setenv("SF_XCL_MIN", "1000000")
    e2, out2 = run(20)
    parity.compare_verdicts(out1, out2, "bound CHAIN rule, default against the raised minimum")
    assert (out1.status == abi.V_BLOCK_FLOW).any() and (out1.status == abi.V_PASS).any()
    for read in (lambda x: x.read_node(0), lambda x: x.read_context_node(3, 0)):
        assert abi.node_state_to_dict(read(e1)) == abi.node_state_to_dict(read(e2))
    e1.close()
    e2.close()


def test_minimum_raised_takes_the_lane_route(eng_mod, so, monkeypatch):
    """SF_XCL_MIN (diagnostics, read at sf_create) raises the minimum: the same segment is decided
    by k_decide_x's lane, with the same result."""
    monkeypatch.setenv("SF_XCL_MIN", "1000000")
    st, _, route = one_resource(eng_mod, so, burst(20_010, 300), frule(101, 40), local=0)
    assert (st == abi.V_PASS).sum() == 40 and route == (0, 0)


def test_model_parity_sample_count_4(eng_mod, so):
    """The walks' other instance (sample_count > 2: NodeWin<16>), lane and wave route."""
    config = ec.cfg(sample_count=4)
    case = ec.random_case(11, n_entries=1500, batches=2, duration_ms=2600)
    m, outs, tail = ec.run_model(case, config=config)
    e = make_engine(eng_mod, config, ec.tables())
    for i, b in enumerate(case["batches"]):
        parity.compare_verdicts(e.submit(b), outs[i], f"S=4 batch {i}")
    assert (e.request_tokens(case["tail"]).status == tail.status).all()
    compare_state(e, m, config, (101, 102, 201), case["t_end"], "S=4")
    e.close()
    st, _, route = one_resource(eng_mod, so, burst(20_010, 300) + burst(20_600, 100), frule(101, 40), local=0,
                                config=ec.cfg(sample_count=4))
    assert (st == abi.V_PASS).sum() == 40 and route == (5 + 2, 0)


# ---------------------------------------------------------------- 4. grouping
def test_limiter_namespace_orders_two_resources(eng_mod, so):
    """Two resources bound to two flowIds of one limiter namespace (4 requests a second),
    interleaved: which request is the fifth, and so falls back, depends on their submission order."""
    rules = [em.flow_rule(2, 0, cluster=True), em.flow_rule(5, 0, cluster=True)]
    tabs = (rules, [(0, 301), (1, 302)], [nsp(3, qps=4)], [frule(301, 100, ns=3), frule(302, 100, ns=3)])
    res = [2, 5, 5, 2, 5, 2, 2, 5] * 3
    hb = abi.HostBatch(res, [30_000 + 40 * (i // 8) for i in range(len(res))], [1] * len(res), [0] * len(res),
                       entry_ref=[-1] * len(res))
    m = em.EmbeddedModel(ec.cfg(), *tabs)
    want = m.submit(hb)
    assert want.status[:8].tolist() == [0, 0, 0, 0, 3, 3, 3, 3] and [c for c, _ in m.trace[:5]] == [em.OK] * 4 + [em.TOO_MANY]
    e = make_engine(eng_mod, ec.cfg(), tabs)
    parity.compare_verdicts(e.submit(hb), want, "limiter namespace")
    compare_state(e, m, ec.cfg(), (301, 302), 30_100, "limiter namespace")
    e.close()


def test_one_flow_id_bound_from_two_resources(eng_mod, so):
    rules = [em.flow_rule(1, 0, cluster=True), em.flow_rule(6, 0, cluster=True)]
    tabs = (rules, [(0, 101), (1, 101)], [nsp(1)], [frule(101, 5)])
    res = [6, 1, 1, 6, 1, 6, 6, 1, 1, 6]
    hb = abi.HostBatch(res, [30_000 + i for i in range(10)], [1] * 10, [0] * 10, entry_ref=[-1] * 10)
    m = em.EmbeddedModel(ec.cfg(), *tabs)
    want = m.submit(hb)
    assert want.status.tolist() == [0] * 5 + [3] * 5
    e = make_engine(eng_mod, ec.cfg(), tabs)
    parity.compare_verdicts(e.submit(hb), want, "shared flowId")
    compare_state(e, m, ec.cfg(), (101,), 30_010, "shared flowId")
    e.close()


# ---------------------------------------------------------------- 5. loads
def test_load_errors(eng_mod):
    rules = [em.flow_rule(0, 5), em.flow_rule(0, 5, cluster=True), em.flow_rule(1, -1.0, cluster=True)]
    e = eng_mod.FlowEngine(ec.cfg())
    e.load_flow_rules(rules)

    def fails(binds, code):
        with pytest.raises(eng_mod.EngineError) as x:
            e.load_cluster_binds(binds)
        assert x.value.code == code, x.value
    fails([(3, 101)], abi.SF_ERR_INVALID)                    # rule_index out of range
    fails([(0, 101)], abi.SF_ERR_INVALID)                    # cluster_mode == 0
    fails([(2, 101)], abi.SF_ERR_INVALID)                    # the load dropped the rule as invalid (count < 0)
    fails([(1, 0)], abi.SF_ERR_INVALID)                      # validClusterRuleId
    fails([(1, -5)], abi.SF_ERR_INVALID)
    fails([(1, 101), (1, 102)], abi.SF_ERR_INVALID)          # two binds name one rule
    e.load_cluster_binds([(1, 101)])                         # a flowId the server does not hold is legal
    fails([(1, 102), (7, 1)], abi.SF_ERR_INVALID)            # ... and a failed load changes nothing
    e.load_cluster_rules(flow=[frule(101, 1)])
    hb = abi.HostBatch([0, 0], [40_000, 40_000], [1, 1], [0, 0])
    assert e.submit(hb).status.tolist() == [abi.V_PASS, abi.V_BLOCK_FLOW]      # still bound to 101
    e.close()
    sharded = eng_mod.FlowEngine(abi.default_config(max_resources=8, max_batch=64, shard_count=2, shard_index=0))
    sharded.load_flow_rules([em.flow_rule(0, 5, cluster=True)])
    with pytest.raises(eng_mod.EngineError) as x:
        sharded.load_cluster_binds([(0, 101)])
    assert x.value.code == abi.SF_ERR_UNSUPPORTED
    sharded.load_cluster_binds([])
    sharded.close()


def test_flow_rule_load_and_empty_list_clear_the_binds(eng_mod, so):
    """sf_load_flow_rules clears the binds, and so does n == 0: the recorded trace then gets the
    verdicts of an engine that never had a bind (the whole-chain oracle's)."""
    case = ec.random_case(3, n_entries=900, batches=1, duration_ms=1500)
    config = ec.cfg()
    rules, binds, namespaces, crules = ec.tables()
    hb = case["batches"][0]
    ora = so.OracleEngine(config)
    ora.load_flow_rules(rules)
    want = ora.submit(hb)
    bound_model, outs, _ = ec.run_model(case, with_tail=False)
    assert (outs[0].status != want.status).sum() > 50        # the binds do change this trace
    for clear in ("empty", "flow"):
        e = make_engine(eng_mod, config, ec.tables())
        if clear == "empty":
            e.load_cluster_binds([])
        else:
            e.load_flow_rules(rules)
        parity.compare_verdicts(e.submit(hb), want, f"binds cleared by {clear}")
        parity.compare_all_nodes(e, ora, config.max_resources)
        assert e.cluster_sum(101, 2, int(hb.ts_ms[-1])) == 0                    # no request was made
        e.close()
        ora = so.OracleEngine(config)
        ora.load_flow_rules(rules)
        ora.submit(hb)


def test_loads_in_every_order_give_the_same_groups(eng_mod, so):
    """The groups depend on the flow rules, binds, cluster rules and namespaces; whichever load
    comes last rebuilds them.  (The flow rule load clears the binds, so it comes before them.)"""
    case = ec.random_case(3, n_entries=900, batches=1, duration_ms=1500)
    m, outs, _ = ec.run_model(case, with_tail=False)
    orders = [o for o in itertools.permutations(("ns", "cluster", "flow", "binds")) if o.index("flow") < o.index("binds")]
    assert len(orders) == 12
    for order in orders:
        e = make_engine(eng_mod, ec.cfg(), ec.tables(), order)
        parity.compare_verdicts(e.submit(case["batches"][0]), outs[0], "loads in order " + " ".join(order))
        e.close()


def test_no_binds_existing_workload_unchanged(eng_mod, so):
    """With no bind loaded nothing differs: an existing workload (cluster token tables loaded
    beside it) gives the oracle's verdicts, node digests and controller states as before."""
    w = workloads.multi_rule()

    class WithTokenTables(eng_mod.FlowEngine):
        def __init__(self, cfg):
            super().__init__(cfg)
            self.load_namespaces([nsp(1), nsp(2, qps=10)])
            self.load_cluster_rules(flow=[frule(101, 5), frule(201, 5, ns=2)])
    e, _, _ = workloads.run(WithTokenTables, so.OracleEngine, w)
    e.close()
