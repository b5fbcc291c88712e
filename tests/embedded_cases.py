"""TEST ONLY -- traffic for the embedded token server (the model:
tests/embedded_model.py), shared by the CPU check of the engine's host-compiled
walk (tests/test_embedded_check.py) and the GPU parity (tests/test_gpu_embedded.py).

``random_case`` is the mixed trace: 8 resources, 3 loaded flowIds and two that
are not, two namespaces of which one has a GlobalRequestLimiter.  ``reach``
asserts on the model alone that the generated traffic takes every branch of
applyTokenResult, so a green parity run cannot come from cases that never get
there."""
import numpy as np

from sentinel_amd import abi
from tests import embedded_model as em
from tests.token_cases import frule, nsp

R = 8
FLOW_IDS = (101, 102, 201)
T0 = 10_000


def tables():
    """(flow rules, binds, namespaces, cluster rules) of the mixed trace."""
    rules = [
        em.flow_rule(0, 8, cluster=True),                                         # 0 -> 101
        em.flow_rule(1, 30),                                                      # 1  local, ahead of
        em.flow_rule(1, 9, cluster=True, fallback=False),                         # 2 -> 102 (AVG_LOCAL)
        em.flow_rule(2, 5, cluster=True),                                         # 3 -> 201, limiter namespace
        em.flow_rule(3, 1, cluster=True, fallback=False, limit_app=abi.APP_OTHER),  # 4 -> 201 too
        em.flow_rule(4, 6, cluster=True),                                         # 5 -> 999, not loaded: local 6
        em.flow_rule(5, 20, behavior=abi.BEHAVIOR_RATE_LIMITER, max_queue=200),   # 6  RateLimiter, ahead of
        em.flow_rule(5, 7, cluster=True),                                         # 7 -> 101 (shared with resource 0)
        em.flow_rule(6, 4, grade=abi.GRADE_THREAD),                               # 8  THREAD, and
        em.flow_rule(6, 12, cluster=True),                                        # 9  a cluster rule without a bind
        em.flow_rule(7, 3, cluster=True, fallback=False),                         # 10 -> 888, not loaded: pass
    ]
    binds = [(0, 101), (2, 102), (3, 201), (4, 201), (5, 999), (7, 101), (10, 888)]
    namespaces = [nsp(1, connected=2), nsp(2, connected=1, qps=25)]
    crules = [frule(101, 20), frule(102, 8, S=4, tt=abi.THRESHOLD_AVG_LOCAL), frule(201, 15, ns=2)]
    return rules, binds, namespaces, crules


def trace(seed, n_entries, t0, duration_ms, res=None, prio_p=0.1, zero_p=0.01, blocked_p=0.02, exit_p=0.4):
    """One time-ordered batch: entries of random resources, some prioritized, some with
    acquireCount 0 / 2 / 3, some SF_EV_BLOCKED; exit_p of them exit inside the batch."""
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.integers(t0, t0 + duration_ms, n_entries))
    ev = []                                           # (ts, order, res, count, flags, entry id or -1)
    for i, t in enumerate(ts):
        r = int(rng.integers(0, R)) if res is None else res
        c = int(rng.choice([1, 1, 1, 1, 2, 3]))
        if rng.random() < zero_p:
            c = 0
        fl = 0
        u = rng.random()
        if u < prio_p:
            fl = abi.EV_PRIO
        elif u < prio_p + blocked_p:
            fl = abi.EV_BLOCKED
        ev.append((int(t), 2 * i, r, c, fl, -1))
        if rng.random() < exit_p:
            te = min(int(t) + int(rng.integers(1, 300)), t0 + duration_ms - 1)
            ev.append((te, 2 * i + 1 + 2 * n_entries, r, c, abi.EV_EXIT | (abi.EV_ERROR if rng.random() < 0.1 else 0), i))
    ev.sort(key=lambda e: (e[0], e[1]))
    pos = {e[1] // 2: k for k, e in enumerate(ev) if e[5] < 0}
    ref = [pos[e[5]] if e[5] >= 0 else -1 for e in ev]
    return abi.HostBatch([e[2] for e in ev], [e[0] for e in ev], [e[3] for e in ev], [e[4] for e in ev], entry_ref=ref)


def random_case(seed=7, n_entries=2900, batches=3, duration_ms=4200):
    """The mixed trace in ``batches`` consecutive batches (about 4k events), and a trailing
    token batch after them that pins the limiter and metric state."""
    span = duration_ms // batches
    bs = [trace(seed * 100 + k, n_entries // batches, T0 + k * span, span) for k in range(batches)]
    t_end = T0 + batches * span
    rng = np.random.default_rng(seed + 1)
    m = 40
    tail = abi.HostTokenBatch(rng.choice([101, 102, 201, 999], m), rng.choice([1, 1, 2], m),
                              (rng.random(m) < 0.2).astype(np.uint8) * abi.TOK_PRIORITIZED,
                              np.sort(rng.integers(t_end, t_end + 300, m)))
    return {"batches": bs, "tail": tail, "t_end": t_end + 300}


def cfg(max_batch=8192, **kw):
    return abi.default_config(max_resources=R, max_batch=max_batch, **kw)


def run_model(case, tabs=None, config=None, with_tail=True):
    """The model's replay of a case -> (model, [verdicts per batch], tail results)."""
    rules, binds, namespaces, crules = tabs or tables()
    m = em.EmbeddedModel(config or cfg(), rules, binds, namespaces, crules)
    outs = [m.submit(b) for b in case["batches"]]
    tail = m.srv.request_tokens(case["tail"]) if with_tail and case.get("tail") is not None else None
    return m, outs, tail


def reach(m, outs):
    """Every outcome of applyTokenResult occurs, with both fallback settings where it can matter."""
    got = set(m.trace)
    classes = {c for c, _ in got}
    assert classes == {em.OK, em.BLOCKED, em.SHOULD_WAIT, em.NO_RULE, em.BAD_REQUEST, em.TOO_MANY}, classes
    for c in (em.NO_RULE, em.BAD_REQUEST, em.TOO_MANY):
        assert (c, True) in got and (c, False) in got, (c, got)
    st = np.concatenate([o.status for o in outs])
    wt = np.concatenate([o.wait_ms for o in outs])
    assert ((st == abi.V_PASS_WAIT) & (wt > 0)).any() and (st == abi.V_PRIORITY_WAIT).any()
    assert (st == abi.V_BLOCK_FLOW).sum() > 100 and (st == abi.V_PASS).sum() > 100
    assert (st == abi.V_BLOCK_OTHER).any() and (st == abi.V_EXIT).any() and (st == abi.V_EXIT_IGNORED).any()


def case_text(config, tabs, case, m, outs):
    """The case file tests/embedded_check.cpp replays: tables, batches with the model's verdicts,
    every resource's ClusterNode and the ClusterMetric sums of every flowId as the model left them."""
    rules, binds, namespaces, crules = tabs
    S = config.sample_count
    L = [f"CFG {S} {config.interval_ms} {config.occupy_timeout_ms} {config.statistic_max_rt} {config.cold_factor} "
         f"{config.exceed_count!r} {config.max_occupy_ratio!r} {config.max_resources}"]
    L.append(f"NS {len(namespaces)}")
    L += [f"{x.namespace_id} {x.connected_count} {x.max_allowed_qps!r}" for x in namespaces]
    L.append(f"CR {len(crules)}")
    L += [f"{x.flow_id} {x.count!r} {x.threshold_type} {x.namespace_id} {x.sample_count} {x.window_interval_ms}" for x in crules]
    L.append(f"FR {len(rules)}")
    L += [f"{r.resource} {r.grade} {r.count!r} {r.control_behavior} {r.max_queueing_time_ms} {r.cluster_mode} "
          f"{r.limit_app} {r.cluster_fallback}" for r in rules]
    L.append(f"BIND {len(binds)}")
    L += [f"{k} {fid}" for k, fid in binds]
    for b, o in zip(case["batches"], outs):
        L.append(f"BATCH {b.n}")
        L += [f"{b.res_id[i]} {b.ts_ms[i]} {b.count[i]} {b.flags[i]} {b.entry_ref[i]} {o.status[i]} {o.wait_ms[i]} {o.rule_idx[i]}"
              for i in range(b.n)]
    absent = (abi.WS_ABSENT, 0, 0, 0, 0, 0, 0, 0)
    for res in range(config.max_resources):
        st = m.node_state(res) or {"second": [absent] * S, "borrow": [(abi.WS_ABSENT, 0)] * S, "minute": [absent] * 60,
                                   "threads": 0}
        L.append(f"NODE {res} {int(res in m.nodes)} {st['threads']}")
        L += [" ".join(map(str, st["second"][i] + st["borrow"][i])) for i in range(S)]
        L += [" ".join(map(str, b)) for b in st["minute"]]
    t_last = max(int(b.ts_ms[-1]) for b in case["batches"])
    for fid in sorted({x.flow_id for x in crules} | {f for _, f in binds}):
        for now in (t_last, t_last + 450):
            L.append(f"SUM {fid} {now} " + " ".join(map(str, m.cluster_sums(fid, now))))
    return "\n".join(L) + "\n"
