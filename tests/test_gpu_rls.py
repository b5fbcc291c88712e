"""GPU parity of the batched Envoy rate-limit service (sf_request_rls) against
the model (tests/rls_model.py: the reference's front-end over the oracle's
ClusterMetric): overall, code, limit, remaining and flow_id of every call, and
afterwards ClusterMetric.getSum of all 7 events of every rule at the last
ts_ms and one interval later.  Each workload (tests/rls_cases.py) has a guard,
from the model's results and sf_rls_get_stats, that proves it reaches what it
is for.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from sentinel_amd import abi, rls
from tests import rls_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


def compare_rls(got, want, what):
    for f in ("overall", "code", "limit", "remaining", "flow_id"):
        g, w = getattr(got, f), getattr(want, f)
        assert g.shape == w.shape, f"{what}: {f} has {g.shape}, the model {w.shape}"
        bad = np.nonzero(g != w)[0]
        assert not bad.size, (f"{what}: {bad.size} {f} values differ; first at {bad[0]}: engine {g[bad[0]]} "
                              f"model {w[bad[0]]}")


def compare_tokens(got, want, what):
    for f in ("status", "remaining", "wait_ms"):
        g, w = getattr(got, f), getattr(want, f)
        assert (g == w).all(), f"{what}: token {f} differs: engine {g.tolist()} oracle {w.tolist()}"


def run_case(eng_mod, so, case, prehashed=False, device=False):
    """The calls of a case on a fresh engine, each against the model's answer; then every sum."""
    ref = rc.reference(case, so)
    e = eng_mod.FlowEngine(case.config())
    if case.namespaces:
        e.load_namespaces(case.namespaces)
    e.load_cluster_rules(case.flow, case.param)
    for k, ((kind, arg), want) in enumerate(zip(case.calls, ref.results)):
        if kind == "rls":
            compare_rls(e.request_rls(rls.pack_requests(arg, prehashed=prehashed), device=device), want,
                        f"{case.name} call {k}")
        elif kind == "tok":
            compare_tokens(e.request_tokens(arg), want, f"{case.name} call {k}")
        else:
            e.load_cluster_rules(arg, case.param)
    got = rc.sums(e, case)
    bad = [(k, got[k], ref.sums[k]) for k in ref.sums if got[k] != ref.sums[k]]
    assert not bad, f"{case.name}: {len(bad)} sums differ; first (flowId, event, now) engine model: {bad[0]}"
    stats = e.rls_stats()
    e.close()
    return ref, stats


@pytest.mark.parametrize("prehashed,device", [(False, False), (False, True), (True, False), (True, True)])
def test_rls_mixed_traffic(eng_mod, so, prehashed, device):
    case = rc.mixed()
    ref, stats = run_case(eng_mod, so, case, prehashed, device)
    rc.guard_mixed(case, ref, stats)


@pytest.mark.parametrize("L", rc.BORDER_LENGTHS)
def test_rls_wave_borders(eng_mod, so, L):
    case = rc.wave_border(L)
    ref, stats = run_case(eng_mod, so, case)
    rc.guard_border(case, ref, L, stats)


def test_rls_old_window(eng_mod, so):
    case = rc.old_window()
    ref, stats = run_case(eng_mod, so, case)
    rc.guard_old_window(case, ref, stats)


@pytest.mark.parametrize("device", [False, True])
def test_rls_strings(eng_mod, so, device):
    case = rc.strings()
    ref, stats = run_case(eng_mod, so, case, device=device)
    rc.guard_strings(case, ref, stats)


def test_rls_shared_state(eng_mod, so):
    case = rc.shared()
    ref, _ = run_case(eng_mod, so, case)
    rc.guard_shared(case, ref, so)


def test_rls_wave_route_switched_off(eng_mod, so, monkeypatch):
    """SF_RLS_WAVE=0 (read at engine creation): every segment takes the lane route, same answers."""
    monkeypatch.setenv("SF_RLS_WAVE", "0")
    case = rc.wave_border(rc.BORDER_LENGTHS[-1])
    _, stats = run_case(eng_mod, so, case)
    assert stats.segs_wave == 0 and stats.chunks == 0 and stats.segs_lane == 6


def test_rls_rule_reload_between_calls(eng_mod, so):
    """sf_load_cluster_rules between two calls: the metrics start again, as it defines."""
    key = [("k", "v")]
    flow = [rc.flow_rule("reload|k|v", 2)]
    reqs = [("reload", [key], 1, 7000 + i) for i in range(4)]
    case = rc.Case("reload", flow, [("rls", reqs), ("load", [rc.flow_rule("reload|k|v", 3)]),
                                    ("rls", [("reload", [key], 1, 7010 + i) for i in range(5)])])
    ref, _ = run_case(eng_mod, so, case)
    assert ref.results[0].code.tolist() == [1, 1, 2, 2] and ref.results[2].code.tolist() == [1, 1, 1, 2, 2]


# ---------------------------------------------------------------- errors
def _small(eng_mod, max_batch=64, **kw):
    flow = [rc.flow_rule("err|k|v", 5)]
    e = eng_mod.FlowEngine(abi.default_config(max_resources=4, max_batch=max_batch, **kw))
    e.load_cluster_rules(flow)
    reqs = [("err", [[("k", "v")], [("k", "w")]], 1, 1000 + i) for i in range(6)]
    return e, flow[0], reqs


def _all_sums(e, fid, now=1010):
    return [e.cluster_sum(fid, ev, now) for ev in rc.EVENTS]


def test_rls_sharded_engine_is_unsupported(eng_mod):
    e, _, reqs = _small(eng_mod, shard_count=2, shard_index=0)
    with pytest.raises(eng_mod.EngineError) as ei:
        e.request_rls(rls.pack_requests(reqs))
    assert ei.value.code == -4                          # SF_ERR_UNSUPPORTED
    e.close()


@pytest.mark.parametrize("device", [False, True])
def test_rls_malformed_tables_are_invalid(eng_mod, device):
    e, rule, reqs = _small(eng_mod)
    e.request_rls(rls.pack_requests(reqs[:2]))
    before = _all_sums(e, rule.flow_id)
    assert before[0] == 2

    def broken(change):
        b = rls.pack_requests(reqs)
        change(b)
        with pytest.raises(eng_mod.EngineError) as ei:
            e.request_rls(b, device=device)
        assert ei.value.code == -1, ei.value               # SF_ERR_INVALID
        assert _all_sums(e, rule.flow_id) == before        # nothing was decided

    def ent_off_decreases(b):
        b.ent_off[3] = b.ent_off[2] - 1

    def string_index_is_n_str(b):
        b.ent_val[-1] = b.n_str

    def domain_index_is_n_str(b):
        b.domain[2] = b.n_str

    def desc_off_decreases(b):
        b.desc_off[2] = b.desc_off[1] - 1

    def str_off_decreases(b):
        b.str_off[1] = b.str_off[2] + 1

    def time_is_negative(b):
        b.ts_ms[:] = -5

    for change in (ent_off_decreases, string_index_is_n_str, domain_index_is_n_str, desc_off_decreases, str_off_decreases,
                   time_is_negative):
        broken(change)
    got = e.request_rls(rls.pack_requests(reqs), device=device)        # the engine goes on working
    assert got.code.tolist() == [1, 1] * 3 + [2, 1] * 3
    e.close()


def test_rls_negative_time_on_a_long_segment_is_invalid(eng_mod):
    """A ts_ms < 0 has no bucket window: the call is refused before any route runs, also with a segment for the wave route."""
    e, rule, _ = _small(eng_mod, max_batch=2 * rc.WAVE_MIN)
    reqs = [("err", [[("k", "v")]], 1, -1000 + i // 8) for i in range(rc.WAVE_MIN + 9)]
    for prehashed in (False, True):
        with pytest.raises(eng_mod.EngineError) as ei:
            e.request_rls(rls.pack_requests(reqs, prehashed=prehashed))
        assert ei.value.code == -1
    assert _all_sums(e, rule.flow_id) == [0] * 7 and e.rls_stats().segs_wave == 0
    e.close()


@pytest.mark.parametrize("device", [False, True])
def test_rls_call_without_descriptors_after_error_requests(eng_mod, so, device):
    """A string-form call whose requests have no descriptors, right after a call
    with error requests at the same indices: a good domain is OK, an ill-formed
    one an error, whatever the call before left behind."""
    d = [("k", "v")]
    bad = rc.ILL_FORMED["overlong_2"]
    first = [(bad, [d], 1, 1000), ("err", [d, [("k", bad)]], 1, 1000), ("err", [d], 1, 1000), ("err", [d], 1, 1000)]
    empty = [("err", [], 1, 1001), ("err", [], 1, 1001), (bad, [], 1, 1001), ("err", [], -1, 1001)]
    case = rc.Case("no_descriptors", [rc.flow_rule("err|k|v", 5)], [("rls", first), ("rls", empty), ("rls", first[2:])])
    ref, stats = run_case(eng_mod, so, case, device=device)
    assert ref.results[0].overall.tolist() == [abi.RLS_ERROR, abi.RLS_ERROR, abi.RLS_OK, abi.RLS_OK]
    assert ref.results[1].overall.tolist() == [abi.RLS_OK, abi.RLS_OK, abi.RLS_ERROR, abi.RLS_ERROR]
    assert ref.results[1].code.size == 0 and stats.error_requests == 4


def test_rls_more_descriptors_than_max_batch(eng_mod):
    e, rule, reqs = _small(eng_mod)
    many = [("err", [[("k", "v")]] * 65, 1, 1000)]
    with pytest.raises(eng_mod.EngineError) as ei:
        e.request_rls(rls.pack_requests(many))
    assert ei.value.code == -5                          # SF_ERR_CAPACITY
    assert _all_sums(e, rule.flow_id) == [0] * 7
    e.close()
