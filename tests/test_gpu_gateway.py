"""GPU parity of the API-gateway flow rules against the model
(tests/gateway_model.py) and the oracle fed by it.  Every workload of
tests/gateway_cases.py runs two ways at once: (a) the columns sf_gateway_args
writes equal the model's exactly -- res_id, ts, count, flags, n_args, every tag
and bits, and every position it must not touch; (b) the batch the engine
produced is decided through workloads.run against the oracle that got the
model's converted rules and columns: every verdict, wait, rule index, node row,
ENTRY_NODE and touched thread count exact.  That each workload sits on its
borders is proved on the CPU (tests/test_gateway_model.py).  Run with -m gpu on
an MI355X."""
import numpy as np
import pytest

from sentinel_amd import abi, gateway as gw
from tests import gateway_cases as gc
from tests import gateway_model as gm
from tests import workloads

pytestmark = pytest.mark.gpu

COLS = [c for c, _ in abi.HostGatewayEvents.COLUMNS]


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


_built = {}


def built(name, make):
    if name not in _built:
        _built[name] = gc.build(make())
    return _built[name]


def poisoned(hb, ev):
    """A copy of ``ev`` whose positions sf_gateway_args must write hold garbage."""
    got = abi.HostGatewayEvents(ev.n_total, ev.entry_ref, ev.exit_pos)
    for c in COLS:
        getattr(got, c)[...] = getattr(ev, c)
    for i in range(hb.n):
        lo, hi = int(hb.ev_index[i]), int(hb.ev_index[i]) + int(hb.res_off[i + 1] - hb.res_off[i])
        for c in COLS:
            getattr(got, c)[..., lo:hi] = 0xAB
    for c in ("n_args", "arg_tag", "arg_bits"):
        getattr(got, c)[..., ev.exit_pos] = 0xCD
    return got


def compare_columns(got, want, what):
    for c in COLS:
        g, w = getattr(got, c), getattr(want, c)
        bad = np.argwhere(g != w)
        assert not bad.size, f"{what}: {len(bad)} {c} values differ; first at {bad[0].tolist()}: engine {g[tuple(bad[0])]} model {w[tuple(bad[0])]}"


def gateway_engine(base, b, device, param_first=False, dup=False):
    """FlowEngine that loads the case's gateway rules and ordinary param rules
    itself (the oracle gets the model's combined list) and, per submit, parses
    the batch's requests with sf_gateway_args, checks the columns against the
    model and decides the batch it produced."""
    case, touched = b["case"], b["case"].get("touched", ())

    class GwEngine(base):
        def __init__(self, cfg):
            super().__init__(cfg)
            self.k, self.threads = 0, []

        def load_param_rules(self, rules, items=()):
            mine = lambda: super(GwEngine, self).load_param_rules(list(case.get("prules", ())), list(case.get("items", ())))  # noqa: E731
            if param_first:
                mine()
            b["table"].load(self)
            if not param_first:
                mine()

        def submit(self, batch, *a):
            hb, ev, want, ct = b["built"][self.k]
            got = poisoned(hb, ev)
            self.gateway_args(gc.duplicate_field(hb) if dup else hb, got, device=device)
            compare_columns(got, want, f"{case['name']} batch {self.k}")
            self.k += 1
            out = super().submit(got.batch(ct), *a)
            self.threads.append([self.param_thread(r, i, (t, x)) for r, i, t, x in touched])
            return out
    return GwEngine


def oracle_engine(base, b):
    touched = b["case"].get("touched", ())

    class Ora(base):
        def __init__(self, cfg):
            super().__init__(cfg)
            self.threads = []

        def submit(self, batch, *a):
            out = super().submit(batch, *a)
            self.threads.append([self.param_thread(r, i, (t, x)) for r, i, t, x in touched])
            return out
    return Ora


def run(eng_mod, so, b, **kw):
    eng, ora, outs = workloads.run(gateway_engine(eng_mod.FlowEngine, b, **kw), oracle_engine(so.OracleEngine, b), b["w"])
    assert eng.threads == ora.threads
    gc.guard_decisions(b, [o for _, o in outs])
    eng.close()


@pytest.mark.parametrize("device", [False, True])
def test_strings(eng_mod, so, device):
    run(eng_mod, so, built("strings", gc.strings), device=device)


@pytest.mark.parametrize("device,param_first", [(False, False), (True, True)])
def test_rule_rows(eng_mod, so, device, param_first):
    run(eng_mod, so, built("rule_rows", gc.rule_rows), device=device, param_first=param_first)


@pytest.mark.parametrize("device", [False, True])
def test_threads_and_exits(eng_mod, so, device):
    run(eng_mod, so, built("threads", gc.threads), device=device)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("n", gc.LAYOUT_N)
def test_layout(eng_mod, so, n, device):
    run(eng_mod, so, built(f"layout{n}", lambda: gc.layout(n)), device=device, dup=(n == 65))


def test_lists_replace_independently(eng_mod):
    b = built("rule_rows", gc.rule_rows)
    hb, ev, want, _ = b["built"][0]
    e = eng_mod.FlowEngine(b["w"]["cfg"])
    got = poisoned(hb, ev)
    e.gateway_args(hb, got)                                 # no gateway rule loaded: every entry without arguments
    ent = (want.flags & abi.EV_EXIT) == 0
    assert (got.n_args[ent] == 0).all() and (got.arg_tag[:, ent] == 0).all() and (got.res_id == want.res_id).all()
    b["table"].load(e)
    prule = abi.sf_param_rule(resource=7, grade=abi.GRADE_QPS, param_idx=0, count=4.0, duration_in_sec=1,
                              max_queueing_time_ms=500)       # equals the converted client-IP rule of resource 7
    with pytest.raises(eng_mod.EngineError) as ei:
        e.load_param_rules([prule])
    assert ei.value.code == abi.SF_ERR_UNSUPPORTED
    e.load_gateway_rules([])                                # clears the gateway list only
    e.load_param_rules([prule])
    with pytest.raises(eng_mod.EngineError) as ei:
        b["table"].load(e)
    assert ei.value.code == abi.SF_ERR_UNSUPPORTED
    many = [abi.sf_param_rule(resource=7, grade=abi.GRADE_QPS, param_idx=0, count=float(10 + k), duration_in_sec=1)
            for k in range(7)]                              # 7 + the 2 converted rules of resource 7
    e.load_param_rules(many)
    with pytest.raises(eng_mod.EngineError) as ei:
        b["table"].load(e)
    assert ei.value.code == abi.SF_ERR_CAPACITY
    got = poisoned(hb, ev)
    e.gateway_args(hb, got)                                 # the failed loads left no gateway rule behind
    assert (got.n_args[ent] == 0).all()
    e.close()


def _mutations(hb, ev):
    """(name, batch arrays to replace, events changes, expected code)."""
    n_total = ev.n_total
    gap = next(p for p in range(n_total) if p not in set(
        int(hb.ev_index[i]) + k for i in range(hb.n) for k in range(int(hb.res_off[i + 1] - hb.res_off[i]))))
    ref = np.full(n_total, -1, np.int64)
    ref_gap = ref.copy(); ref_gap[gap] = gap                 # an EXIT whose entry is no gateway entry
    ref_ent = ref.copy(); ref_ent[int(hb.ev_index[0])] = int(hb.ev_index[1])

    def arr(name, idx, val):
        a = getattr(hb, name).copy()
        a[idx] = val
        return {name: a}
    return [
        ("res_off decreases", arr("res_off", 3, hb.res_off[2] - 1), {}, abi.SF_ERR_INVALID),
        ("res_off[0] != 0", arr("res_off", 0, 1), {}, abi.SF_ERR_INVALID),
        ("val_off decreases", arr("val_off", 2, hb.val_off[1] - 1) if hb.val_off[1] else arr("val_off", 3, hb.val_off[2] - 1), {},
         abi.SF_ERR_INVALID),
        ("str_off decreases", arr("str_off", 1, hb.str_off[2] + 1), {}, abi.SF_ERR_INVALID),
        ("string index", arr("val_str", 0, hb.n_str), {}, abi.SF_ERR_INVALID),
        ("ranges overlap", arr("ev_index", 1, hb.ev_index[0] + 1), {}, abi.SF_ERR_INVALID),
        ("range passes n_total", arr("ev_index", hb.n - 1, n_total), {}, abi.SF_ERR_INVALID),
        ("resource of no shard", arr("res_id", 5, gc.R), {}, abi.SF_ERR_INVALID),
        ("exit of no gateway entry", {}, dict(entry_ref=ref_gap, exit_pos=[gap]), abi.SF_ERR_INVALID),
        ("exit_pos on a gateway entry", {}, dict(entry_ref=ref_ent, exit_pos=[int(hb.ev_index[0])]), abi.SF_ERR_INVALID),
        ("exit_pos out of range", {}, dict(entry_ref=ref, exit_pos=[n_total]), abi.SF_ERR_INVALID),
    ]


@pytest.mark.parametrize("device", [False, True])
def test_errors_leave_the_columns(eng_mod, device):
    b = built("layout65", lambda: gc.layout(65))
    hb, ev, want, _ = b["built"][0]
    e = eng_mod.FlowEngine(b["w"]["cfg"])
    b["table"].load(e)
    for name, repl, evc, code in _mutations(hb, ev):
        bad = abi.HostGatewayBatch(**{**{a: getattr(hb, a) for a in hb.ARRAYS}, **repl})
        got = poisoned(hb, ev)
        if evc:
            got.entry_ref, got.exit_pos = evc["entry_ref"], np.ascontiguousarray(evc["exit_pos"], np.uint32)
        before = {c: getattr(got, c).copy() for c in COLS}
        with pytest.raises(eng_mod.EngineError) as ei:
            e.gateway_args(bad, got, device=device)
        assert ei.value.code == code, name
        for c in COLS:
            assert (getattr(got, c) == before[c]).all(), f"{name}: {c} was written"
    small = eng_mod.FlowEngine(abi.default_config(max_resources=gc.R, max_batch=ev.n_total - 1))
    with pytest.raises(eng_mod.EngineError) as ei:
        small.gateway_args(hb, poisoned(hb, ev), device=device)
    assert ei.value.code == abi.SF_ERR_CAPACITY
    small.close()
    got = poisoned(hb, ev)                                   # and the engine still works after the refusals
    e.gateway_args(hb, got, device=device)
    compare_columns(got, want, "after errors")
    e.close()
