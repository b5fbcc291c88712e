"""DegradeSlot border cases through the whole slot chain (sf_submit, not
sf_degrade_submit): breakers on resources whose flow rule would otherwise
take a window algorithm, entries that FlowSlot / ParamFlowSlot block or hold
with a PriorityWaitException in front of an OPEN breaker, and breakers on
resources decided by the cross-resource walk (RELATE, CHAIN, origin-specific
rules).  Companion of tests/degrade_cases.py; shared by
tests/test_degrade_cases.py (host build against the C oracle) and
tests/test_gpu_degrade_cases.py (the engine against the C oracle).

CASES[name] = (build, guard).  build() returns a workload dict as
tests/workloads.py does, with ``degrade`` rules beside ``flow`` / ``param``;
guard(w, (verdicts per batch, breaker rows)) sees the C oracle's results only.
"""
import numpy as np

from sentinel_amd import abi
from tests import boundary_cases as bc
from tests import degrade_cases as dc
from tests import parity
from tests.test_degrade_chain import _breaker_rows

T0 = dc.T0


def _load(e, w):
    if w.get("flow"):
        e.load_flow_rules(list(w["flow"]))
    if w.get("param"):
        e.load_param_rules(list(w["param"]), list(w.get("items", ())))
    return e.load_degrade_rules(list(w["degrade"]))


def oracle_run(so, w):
    o = so.OracleEngine(w["cfg"])
    try:
        n = _load(o, w)
        return [o.submit(b) for b in w["batches"]], _breaker_rows(o, n)
    finally:
        o.close()


def run(make_engine, make_oracle, w):
    """Both through the chain; verdicts, waits, rule indices, node rows, rule
    states, ENTRY_NODE and every breaker's state compared exactly."""
    eng, ora = make_engine(w["cfg"]), make_oracle(w["cfg"])
    n = _load(eng, w)
    assert n == _load(ora, w)
    for k, b in enumerate(w["batches"]):
        parity.compare_verdicts(eng.submit(b), ora.submit(b), f"batch{k}")
    assert np.array_equal(_breaker_rows(eng, n), _breaker_rows(ora, n)), "breaker states"
    sc = w["cfg"].sample_count
    parity.compare_nodes(eng, ora, w["nodes"], sample_count=sc)
    if hasattr(eng, "node_digests"):
        parity.compare_all_nodes(eng, ora, w["cfg"].max_resources, sample_count=sc)
        if w.get("n_flow"):
            parity.compare_all_rule_states(eng, ora, w["n_flow"])
    if getattr(eng, "has_entry_node", False):
        parity.compare_entry_node(eng, ora, sample_count=sc)
    if w.get("n_flow"):
        parity.compare_rule_states(eng, ora, w["n_flow"])
    parity.compare_aux_nodes(eng, ora, w.get("origin_nodes", ()), w.get("context_nodes", ()), sample_count=sc)
    return eng, ora


def _with(full, **kw):
    """The batch with further per-event arrays (origin, context, args, flags)."""
    return abi.HostBatch(full.res_id, full.ts_ms, full.count, kw.pop("flags", full.flags), entry_ref=full.entry_ref,
                         create_ts=full.create_ts, **kw)


# ---------------------------------------------------------------- routing
ROUTE_KINDS = ("qps", "warm", "rl", "thread")


def chain_routing():
    """A breaker on resources of every segment length on k_classify's routing
    borders (boundary_cases.ROUTE_LENGTHS: the light length classes, one
    under, on and one over the default heavy_min_events) for each flow rule
    that has a window algorithm of its own: with a breaker every heavy one of
    them is SM_GENERIC."""
    S, flow, degrade, meta = dc.Script(), [], [], []
    for kind in ROUTE_KINDS:
        for m in bc.ROUTE_LENGTHS:
            r = len(meta)
            meta.append((kind, m))
            c = 2 + r % 4
            flow.append({"qps": bc._qps(r, 6 * c), "warm": bc._warm(r, 18 * c), "rl": bc._rl(r, 15 * c, 30),
                         "thread": bc._thread(r, c)}[kind])
            degrade.append(dc.rule(r, dc.COUNT, 1, interval=300))
            dc.churn(S, r, m, seed=500 + r, dt_max=12)
    full, _ = S.assemble(extra_flags=abi.EV_IN)
    R = len(meta)
    modes = {r: bc.SM_GENERIC for r, (_, m) in enumerate(meta) if m > bc.HEAVY_MIN}
    return dict(cfg=abi.default_config(max_resources=R, max_batch=full.n), flow=flow, degrade=degrade, batches=[full],
                full=full, nodes=list(range(R)), n_flow=len(flow), meta=meta, modes=modes)


def guard_chain_routing(w, out):
    full, st = w["full"], out[0][0].status
    lens = np.bincount(full.res_id, minlength=len(w["meta"]))
    assert [int(x) for x in lens] == [m for _, m in w["meta"]]
    for B in (bc.HEAVY_MIN - 1, bc.HEAVY_MIN, bc.HEAVY_MIN + 1):
        assert B in bc.ROUTE_LENGTHS
    assert len(w["modes"]) == 2 * len(ROUTE_KINDS)
    for kind in ROUTE_KINDS:
        sel = np.isin(full.res_id, [r for r, (k, _) in enumerate(w["meta"]) if k == kind])
        for v in (abi.V_PASS, abi.V_BLOCK_FLOW, abi.V_BLOCK_DEGRADE, abi.V_EXIT_IGNORED):
            assert (st[sel] == v).any(), (kind, v)
        for r in w["modes"]:                                   # the heavy ones: the breaker moves there, too
            if w["meta"][r][0] == kind:
                assert (st[full.res_id == r] == abi.V_BLOCK_DEGRADE).any(), r
    return dict(events=full.n, heavy=len(w["modes"]), degrade_blocks=int((st == abi.V_BLOCK_DEGRADE).sum()))


# ---------------------------------------------------------------- the slots in front of DegradeSlot
WRAP_TW = 4294967                                              # recovery -296 ms: the retry time is reached at once


def chain_slots():
    """An OPEN breaker whose retry time is reached, and the entries the slots
    before DegradeSlot answer: the literal expectations are in guard_chain_slots."""
    S = dc.Script()
    # resource 0: QPS 1.  Breaker 0 trips at the first error, breaker 1 at the second.
    x = dc.Res(S, 0, T0 + 10)
    e1 = x.entry()                                             # passes, takes the window's one token
    x.exit(of=e1, err=True)                                    # breaker 0 OPEN, next_retry in the past
    # half a second on e1's token still fills the window, and the next bucket can be occupied
    # (StatisticNode.tryOccupyNext): a prioritized entry waits for it
    x.at(T0 + 512)
    e2 = x.entry(flags=abi.EV_PRIO)                            # PriorityWaitException: never reaches the breakers
    e3 = x.entry()                                             # FlowException: neither
    x.exit(of=e3, err=True)                                    # blockError set: ignored
    x.exit(of=e2, err=True)                                    # completes: breaker 1's second error trips it
    t_trip = x.t
    e4 = x.at(T0 + 2010).entry(dt=0)                           # a second later: passes FlowSlot, probes both
    # resource 1: ParamFlow QPS 1 on the argument
    y = dc.Res(S, 1, T0 + 10)
    f1 = y.entry()
    y.exit(of=f1, err=True)                                    # OPEN, retry reached
    f2 = y.entry()                                             # ParamFlowException: does not probe
    y.exit(of=f2, err=True)                                    # ignored
    f3 = y.at(T0 + 2010).entry(dt=0)                           # probes
    # resource 2: IN entries refused by an OPEN breaker (blocks of the node and of ENTRY_NODE)
    z = dc.Res(S, 2, T0 + 10)
    z.exit(of=z.entry(), err=True)
    blk = [z.entry() for _ in range(5)]
    full, _ = S.assemble(extra_flags=abi.EV_IN)
    n = full.n
    full = _with(full, arg_tag=np.full((1, n), abi.TAG_LONG, np.uint8), arg_bits=np.full((1, n), 7, np.uint64),
                 n_args=np.ones(n, np.uint8))
    degrade = [dc.rule(0, dc.COUNT, 0, tw=WRAP_TW), dc.rule(0, dc.COUNT, 1, tw=1), dc.rule(1, dc.COUNT, 0, tw=WRAP_TW),
               dc.rule(2, dc.COUNT, 0, tw=50)]
    h = dict(e1=e1, e2=e2, e3=e3, e4=e4, f1=f1, f2=f2, f3=f3, blk=blk)
    pos = {k: ([int(S.pos[i]) for i in v] if isinstance(v, list) else int(S.pos[v])) for k, v in h.items()}
    return dict(cfg=abi.default_config(max_resources=3, max_batch=n, param_capacity=1 << 10), flow=[bc._qps(0, 1)],
                param=[bc._prule(1, 1)], degrade=degrade, batches=[full], full=full, nodes=[0, 1, 2], n_flow=1, pos=pos,
                t_trip=t_trip)


def guard_chain_slots(w, out):
    """Literal verdicts and states, from DegradeSlot.java:50-94: performChecking
    runs only when the slots before it let the entry through; exit() returns
    early when the entry carries a blockError, and a PriorityWaitException is
    none."""
    (v,), rows = out
    full, p = w["full"], w["pos"]
    st = v.status
    got = {k: int(st[i]) for k, i in p.items() if k != "blk"}
    assert got == dict(e1=abi.V_PASS, e2=abi.V_PRIORITY_WAIT, e3=abi.V_BLOCK_FLOW, e4=abi.V_PASS, f1=abi.V_PASS,
                       f2=abi.V_BLOCK_PARAM, f3=abi.V_PASS), got
    assert [int(st[i]) for i in p["blk"]] == [abi.V_BLOCK_DEGRADE] * 5
    ex = {int(full.entry_ref[i]): int(st[i]) for i in np.nonzero(full.flags & abi.EV_EXIT)[0]}
    assert ex[p["e2"]] == abi.V_EXIT and ex[p["e3"]] == abi.V_EXIT_IGNORED and ex[p["f2"]] == abi.V_EXIT_IGNORED
    # rows: state, next_retry, window_start, hits, total.  Resource 0: the probe at e4 finds both
    # OPEN (breaker 1 tripped by the waiting entry's exit at t_trip): HALF_OPEN, retry times kept
    assert rows[0][0] == abi_cb("HALF_OPEN") and rows[0][1] == T0 + 12 - 296 and tuple(rows[0][3:]) == (2, 2)
    assert rows[1][0] == abi_cb("HALF_OPEN") and rows[1][1] == w["t_trip"] + 1000 and tuple(rows[1][3:]) == (2, 2)
    assert rows[2][0] == abi_cb("HALF_OPEN") and tuple(rows[2][3:]) == (1, 1)      # f2 neither probed nor completed
    assert rows[3][0] == abi_cb("OPEN")
    return dict(events=full.n)


def abi_cb(name):
    from oracle import degrade as od
    return getattr(od, name)


# ---------------------------------------------------------------- the cross-resource walk
def chain_xflow():
    """Two breakers (retry after 1 s and after 5 s: a probe of the first that
    the second sends back) on resources whose flow rule reads another node: a
    RELATE rule, a CHAIN rule and an origin-specific rule, each on a short and
    on a long segment."""
    S, flow, degrade, meta = dc.Script(), [], [], []
    kw = dict(strategy=0, control_behavior=0, warm_up_period_sec=10, max_queueing_time_ms=500)
    for n_ev in (40, 400):
        for kind in ("relate", "chain", "origin"):
            r = 2 * len(meta)
            meta.append((kind, n_ev, r))
            long_ = n_ev > 100
            # relate: limited by the traffic of r + 1; chain: entries of context 1; origin: those of origin 3
            extra, count = {"relate": (dict(strategy=abi.STRATEGY_RELATE, ref_resource=r + 1), 6.0 if long_ else 1.0),
                            "chain": (dict(strategy=abi.STRATEGY_CHAIN, ref_resource=1), 1.0 if long_ else 0.0),
                            "origin": (dict(limit_app=3), 4.0 if long_ else 1.0)}[kind]
            flow.append(abi.sf_flow_rule(resource=r, grade=abi.GRADE_QPS, count=count, **{**kw, **extra}))
            degrade += [dc.rule(r, dc.COUNT, 0, tw=1), dc.rule(r, dc.COUNT, 0, tw=5)]
            dc.churn(S, r, n_ev, seed=711 + r, dt_max=60 if long_ else 300, err_p=0.3)
            dc.churn(S, r + 1, n_ev // 2, seed=800 + r, dt_max=120 if long_ else 150)
    full, _ = S.assemble(extra_flags=abi.EV_IN)
    rng = np.random.default_rng(7)
    og = np.where(rng.random(full.n) < 0.6, 3, np.where(rng.random(full.n) < 0.5, 2, abi.ORIGIN_NONE)).astype(np.uint32)
    cx = rng.integers(0, 2, full.n).astype(np.uint32)
    ex = np.nonzero(full.entry_ref >= 0)[0]                    # an exit carries its entry's origin and context
    og[ex], cx[ex] = og[full.entry_ref[ex]], cx[full.entry_ref[ex]]
    full = _with(full, origin=og, context=cx)
    R = 2 * len(meta)
    return dict(cfg=abi.default_config(max_resources=R, max_batch=full.n), flow=flow, degrade=degrade, batches=[full],
                full=full, nodes=list(range(R)), n_flow=len(flow), meta=meta)


def guard_chain_xflow(w, out):
    (v,), rows = out
    full, st = w["full"], v.status
    for kind, n_ev, r in w["meta"]:
        sel = full.res_id == r
        assert int(sel.sum()) == n_ev
        s, ri = st[sel], v.rule_idx[sel]
        assert (s == abi.V_BLOCK_FLOW).any() and (s == abi.V_PASS).any(), (kind, n_ev)
        # refused by the second breaker: the first one's retry time was reached (probe sent back) or not
        assert ((s == abi.V_BLOCK_DEGRADE) & (ri == 1)).any() and (s == abi.V_EXIT_IGNORED).any(), (kind, n_ev)
    return dict(events=full.n, degrade_blocks=int((st == abi.V_BLOCK_DEGRADE).sum()),
                flow_blocks=int((st == abi.V_BLOCK_FLOW).sum()))


CASES = {
    "chain_routing": (chain_routing, guard_chain_routing),
    "chain_slots": (chain_slots, guard_chain_slots),
    "chain_xflow": (chain_xflow, guard_chain_xflow),
}
