"""AuthorityRule black / white lists decided inside the engine
(sf_load_authority_rules, the k_auth_mark pass, verdict V_BLOCK_AUTHORITY)
against the reference semantics.

The expectation never comes from the engine: the string model
(tests/authority_model.py) marks the entries AuthoritySlot blocks, the oracle
replays the batch with those entries flagged EV_BLOCKED, and its verdict 9
becomes 10 at the marked positions (tests/authority_cases.py); wait, rule_idx,
every node digest, the origin nodes of blocked pairs, ENTRY_NODE, rule and
breaker state must be bit-equal.  References are computed once per workload
and shared."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sentinel_amd import abi, system_shard, trace
from tests import authority_cases as ac
from tests import authority_model as am
from tests import parity, workloads

pytestmark = pytest.mark.gpu

# ---- the mark kernel's constants, restated (test_constants_match_the_source) ----
AUTH_VEC = 4                # sf_authority.hip: events per vector group (one dwordx4 of ids, one dword of flags)
AUTH_TILE = 4096            # sf_authority.hip: events per workgroup tile
AUTH_LINEAR_MAX = 8         # sf_authority.h: longest list searched linearly
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sentinel_amd", "csrc")


def test_constants_match_the_source():
    hip = open(os.path.join(_CSRC, "sf_authority.hip")).read()
    hdr = open(os.path.join(_CSRC, "sf_authority.h")).read()
    assert int(re.search(r"constexpr uint32_t AUTH_VEC = (\d+);", hip).group(1)) == AUTH_VEC
    assert int(re.search(r"constexpr uint32_t AUTH_TILE = (\d+);", hip).group(1)) == AUTH_TILE
    assert int(re.search(r"constexpr uint32_t AUTH_LINEAR_MAX = (\d+);", hdr).group(1)) == AUTH_LINEAR_MAX


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


def _load(e, w):
    if w.get("status") is not None:
        e.set_system_status(*w["status"])
    if w.get("system"):
        e.load_system_rules(list(w["system"]))
    if w.get("flow"):
        e.load_flow_rules(list(w["flow"]))
    if w.get("param"):
        e.load_param_rules(list(w["param"]), list(w.get("items", ())))


def _cfg(w, **kw):
    c = abi.sf_config.from_buffer_copy(w["cfg"])
    for k, v in kw.items():
        setattr(c, k, v)
    return c


class Ref:
    """A workload, its AuthorityRules and the expectation of every batch."""

    def __init__(self, so, w, rules=None, **pick):
        self.w, self.it = w, am.Interner()
        self.rules = ac.pick_rules(w["batches"], w["cfg"].max_resources, self.it, **pick) if rules is None else rules
        self.mgr = am.AuthorityRuleManager()
        self.mgr.load_rules(self.rules)
        self.tables = am.to_tables(self.rules, ac.res_id, self.it)
        self.share = ac.share_of(self.mgr, w["batches"], self.it)
        parts = [ac.split_for(self.mgr, b, self.it) for b in w["batches"]]
        self.batches = [p[0] for p in parts]
        self.marks = [p[2] for p in parts]
        self.ora = so.OracleEngine(w["cfg"])
        _load(self.ora, w)
        self.n_breakers = self.ora.load_degrade_rules(w["degrade"]) if w.get("degrade") else 0
        self.want = [ac.expected(self.ora.submit(p[1]), p[2]) for p in parts]
        self.status = np.concatenate([v.status for v in self.want])

    def engine(self, eng_mod, **cfg):
        e = eng_mod.FlowEngine(_cfg(self.w, **cfg))
        _load(e, self.w)
        if self.w.get("degrade"):
            assert e.load_degrade_rules(self.w["degrade"]) == self.n_breakers
        assert e.load_authority_rules(self.tables) == len(self.mgr.get_rules())
        return e

    def count(self, v):
        return int((self.status == v).sum())

    def compare_state(self, e):
        c = self.w["cfg"]
        parity.compare_all_nodes(e, self.ora, c.max_resources, sample_count=c.sample_count)
        if self.w.get("n_flow"):
            parity.compare_all_rule_states(e, self.ora, self.w["n_flow"])
        parity.compare_entry_node(e, self.ora, sample_count=c.sample_count)
        parity.compare_aux_nodes(e, self.ora, origin_nodes=ac.blocked_pairs(self.batches, self.marks),
                                 context_nodes=self.w.get("context_nodes", ()), sample_count=c.sample_count)


def _build(so, name):
    if name == "xflow":
        return Ref(so, workloads.xflow(), seed=1)
    if name == "config3":
        return Ref(so, ac.add_origins(workloads.config3(R=2000, n=80_000), seed=3), seed=2)
    if name == "xflow_both":                                   # caller-flagged entries beside the engine's
        return Ref(so, workloads.preblocked(workloads.xflow(seed=52), frac=0.04, seed=6), seed=5)
    if name in ("system_qps", "system_thread"):
        return Ref(so, ac.add_origins(workloads.system(name[7:]), seed=4), seed=3, share=0.2, listed=2)
    if name == "chain":
        from tests import test_degrade_chain as tc
        cfg, flow, rules, b = tc.chain_workload(21, prio=0.1, n=60_000)
        cut = b.n // 3
        w = dict(cfg=cfg, flow=flow, degrade=rules, batches=[b.subset(0, cut), b.subset(cut, b.n)], n_flow=len(flow))
        return Ref(so, ac.add_origins(w, seed=5), seed=4)
    raise KeyError(name)


@pytest.fixture(scope="module")
def refs(so):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _build(so, name)
        return cache[name]
    yield get
    for r in cache.values():
        r.ora.close()


# ---------------------------------------------------------------- the mark pass alone
MARK_R = 64
MARK_LENS = [1, 2, 3, AUTH_LINEAR_MAX, AUTH_LINEAR_MAX + 1, 64, 1000]
MARK_SIZES = [1, AUTH_VEC - 1, AUTH_VEC, AUTH_VEC + 1, AUTH_TILE - 1, AUTH_TILE, AUTH_TILE + 1]


@pytest.fixture(scope="module")
def mark_case(eng_mod):
    """Rules on row 0, the last row and between, every list length; one batch
    of 2 tiles + a vector + 1 whose prefixes are the border sizes."""
    it = am.Interner()
    rng = np.random.default_rng(8)
    rows = [0, MARK_R - 1] + rng.choice(np.arange(1, MARK_R - 1), size=2 * len(MARK_LENS) - 2, replace=False).tolist()
    rules, names = [], []
    for k, r in enumerate(rows):
        n = MARK_LENS[k % len(MARK_LENS)]
        mine = [f"app{k}_{j}" for j in range(n)]
        rng.shuffle(mine)
        names += mine[:2] + mine[-1:]
        rules.append(am.AuthorityRule(ac.res_name(r), ",".join(mine), am.AUTHORITY_BLACK if k % 2 else am.AUTHORITY_WHITE))
    mgr = am.AuthorityRuleManager()
    mgr.load_rules(rules)
    n = 2 * AUTH_TILE + AUTH_VEC + 1
    ids = np.array([it.id(s) for s in names] + [abi.ORIGIN_NONE, 0, 1, it.id("nobody")], np.uint32)
    res = rng.integers(0, MARK_R + 2, n).astype(np.uint32)           # (two ids past the last row: never blocked)
    res[:8] = [0, MARK_R - 1, 0, MARK_R - 1, MARK_R, 0xFFFFFFFF, 0, MARK_R - 1]
    og = ids[rng.integers(0, ids.size, n)]
    IN, X, B = abi.EV_IN, abi.EV_EXIT, abi.EV_BLOCKED
    kinds = np.array([IN, IN, IN | abi.EV_PRIO, 0, IN | X, X | abi.EV_ERROR, IN | B, IN | 0x20, IN | 0x40, 0x60,
                      IN | B | 0x20, IN | X | 0x60], np.uint8)
    fl = kinds[rng.integers(0, kinds.size, n)]
    blocks = am.blocked_mask(mgr, ac.res_name, res, og, np.zeros(n, np.uint8), it) & (res < MARK_R)
    want = (fl & np.uint8(0x9F)).astype(np.uint8)
    want[blocks & ((fl & (X | B)) == 0)] |= B
    assert 0.1 < blocks.mean() < 0.9
    e = eng_mod.FlowEngine(abi.default_config(max_resources=MARK_R, max_batch=n))
    assert e.load_authority_rules(am.to_tables(rules, ac.res_id, it)) == len(rows)
    yield e, res, og, fl, want
    e.close()


@pytest.mark.parametrize("n", MARK_SIZES + [2 * AUTH_TILE + AUTH_VEC + 1])
@pytest.mark.parametrize("mem", ["host", "device"])
def test_mark_borders(eng_mod, mark_case, mem, n):
    """sf_authority_mark against the model at the vector and tile borders:
    exits are never marked, a caller-flagged entry is left alone, the reserved
    bits 0x20 / 0x40 are stripped, nothing but EV_BLOCKED is added."""
    e, res, og, fl, want = mark_case
    if mem == "host":
        got = e.authority_mark(res[:n], og[:n], fl[:n])
    else:
        d = [eng_mod.DeviceArray(e, np.ascontiguousarray(a[:n])) for a in (res, og, fl)]
        out = eng_mod.DeviceArray.empty(e, n, np.uint8)
        e.authority_mark_device(d[0], d[1], d[2], out)
        got = out.numpy()
        for a in d + [out]:
            a.free()
    bad = np.nonzero(got != want[:n])[0]
    assert bad.size == 0, f"{bad.size} flags differ; first {bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"
    assert not (got[(fl[:n] & abi.EV_EXIT) != 0] & abi.EV_BLOCKED).any()


def test_mark_unaligned_device_arrays(eng_mod, mark_case):
    """Device arrays that are not 16-byte aligned take the event-by-event kernel."""
    e, res, og, fl, want = mark_case
    n = AUTH_TILE + AUTH_VEC + 2
    d = [eng_mod.DeviceArray(e, np.ascontiguousarray(a[:n + 1])) for a in (res, og, fl)]
    out = eng_mod.DeviceArray.empty(e, n + 1, np.uint8)
    rc = eng_mod.lib().sf_authority_mark(e.h, d[0].ptr + 4, d[1].ptr + 4, d[2].ptr + 1, n, abi.MEM_DEVICE, out.ptr + 1)
    assert rc == 0
    got = out.numpy()[1:]
    for a in d + [out]:
        a.free()
    assert np.array_equal(got, want[1:n + 1])


def test_mark_without_origins_or_rules_is_a_copy(eng_mod, mark_case):
    e, res, og, fl, _ = mark_case
    assert np.array_equal(e.authority_mark(res[:100], None, fl[:100]), fl[:100] & 0x9F)
    e2 = eng_mod.FlowEngine(abi.default_config(max_resources=MARK_R, max_batch=128))
    try:
        assert np.array_equal(e2.authority_mark(res[:100], og[:100], fl[:100]), fl[:100] & 0x9F)
    finally:
        e2.close()


def test_loader_validity_and_failed_load(eng_mod, mark_case):
    """n_loaded follows the manager; a malformed range is SF_ERR_INVALID and leaves the loaded map in force."""
    e, res, og, fl, want = mark_case
    arr, apps = abi.authority_tables([(0, abi.AUTHORITY_BLACK, [5, 6]), (1, abi.AUTHORITY_BLACK, [7])])
    arr[1].app_off, arr[1].app_cnt = 2, 5                     # leaves apps[]
    rc = eng_mod.lib().sf_load_authority_rules(e.h, arr, 2, apps.ctypes.data, apps.size, None)
    assert rc == abi.SF_ERR_INVALID
    assert np.array_equal(e.authority_mark(res[:AUTH_TILE], og[:AUTH_TILE], fl[:AUTH_TILE]), want[:AUTH_TILE])
    e2 = eng_mod.FlowEngine(abi.default_config(max_resources=8, max_batch=16))
    try:
        kept = e2.load_authority_rules([(1, -1, [5]), (1, abi.AUTHORITY_BLACK, [5]), (1, abi.AUTHORITY_WHITE, [5]),
                                        (2, abi.AUTHORITY_BLACK, []), (0xFFFFFFFF, abi.AUTHORITY_BLACK, [5]),
                                        (3, 2, [5])])
        assert kept == 2                                       # resource 1's first valid rule, resource 3's
        f = np.full(4, abi.EV_IN, np.uint8)
        got = e2.authority_mark([1, 1, 3, 2], [5, 6, 5, 5], f)
        assert got.tolist() == [abi.EV_IN | abi.EV_BLOCKED, abi.EV_IN, abi.EV_IN, abi.EV_IN]
        assert e2.load_authority_rules([]) == 0
        assert np.array_equal(e2.authority_mark([1, 1, 3, 2], [5, 6, 5, 5], f), f)
    finally:
        e2.close()


# ---------------------------------------------------------------- pipeline parity
@pytest.mark.parametrize("heavy_min", [0, 8, 512])
@pytest.mark.parametrize("name", ["xflow", "config3"])
def test_pipeline_parity(eng_mod, refs, name, heavy_min):
    """Origin-bearing traffic with white and black rules on a tenth of the
    resources, the busiest included: lane, heavy and stream paths all see
    marked entries."""
    ref = refs(name)
    assert 0.03 <= ref.share <= 0.10, ref.share               # (the model's share, before any GPU call)
    for v in (abi.V_BLOCK_AUTHORITY, abi.V_BLOCK_FLOW, abi.V_EXIT_IGNORED, abi.V_PASS_WAIT):
        assert ref.count(v) > 0, v
    e = ref.engine(eng_mod, heavy_min_events=heavy_min)
    try:
        for k, b in enumerate(ref.batches):
            parity.compare_verdicts(e.submit(b), ref.want[k], f"{name} batch {k}")
        ref.compare_state(e)
    finally:
        e.close()


def _host(v_status, v_wait, v_rule, n):
    out = abi.HostVerdicts(n)
    out.status[:], out.wait_ms[:], out.rule_idx[:] = v_status, v_wait, v_rule
    return out


def _run_form(eng_mod, e, ref, form):
    if form == "host":
        return [e.submit(b) for b in ref.batches]
    if form == "device_async":                                # both batches in flight
        dbs = [eng_mod.DeviceBatch(e, b) for b in ref.batches]
        dvs = [eng_mod.DeviceVerdicts(e, b.n, with_wait=True, with_rule=True) for b in ref.batches]
        for db, dv in zip(dbs, dvs):
            e.submit_device_async(db, dv)
        e.sync()
        outs = [_host(dv.status.numpy(), dv.wait_ms.numpy(), dv.rule_idx.numpy(), b.n) for dv, b in zip(dvs, ref.batches)]
        for x in dbs + dvs:
            x.free()
        return outs
    pin = eng_mod.PinnedArrays(e)
    try:
        pbs = [abi.PackedBatch(b, alloc=pin.array, narrow=form == "packed4") for b in ref.batches]
        if form == "sparse":
            sv = [pin.sparse_verdicts(b.n, 64) for b in ref.batches]
            for pb, o in zip(pbs, sv):
                e.submit_packed_sparse_async(pb, o)
            outs = []
            for o in sv:
                e.sync_packed_sparse(o)
                d = o.dense()
                outs.append(_host(d.status, d.wait_ms, d.rule_idx, d.status.size))
            e.sync()
            return outs
        hv = [pin.verdicts(b.n) for b in ref.batches]
        if form == "packed8_sync":
            for pb, o in zip(pbs, hv):
                e.submit_packed(pb, o)
        else:
            for pb, o in zip(pbs, hv):
                e.submit_packed_async(pb, o)
            e.sync()
        return [_host(o.status, o.wait_ms, o.rule_idx, o.status.size) for o in hv]
    finally:
        pin.free()


def test_every_form_gives_the_same_verdicts(eng_mod, refs):
    """Host SoA, HBM-resident sf_submit_async (two batches in flight), the
    packed 8-byte form synchronous and asynchronous, the 4-byte form and sparse
    verdicts: identical status arrays, equal to the expectation."""
    ref = refs("xflow")
    seen = {}
    for form in ("host", "device_async", "packed8_sync", "packed8", "packed4", "sparse"):
        e = ref.engine(eng_mod)
        try:
            outs = _run_form(eng_mod, e, ref, form)
            for k, o in enumerate(outs):
                parity.compare_verdicts(o, ref.want[k], f"{form} batch {k}")
            ref.compare_state(e)
            seen[form] = np.concatenate([o.status for o in outs])
        finally:
            e.close()
    for form, st in seen.items():
        assert np.array_equal(st, seen["host"]), form
    assert (seen["host"] == abi.V_BLOCK_AUTHORITY).sum() == sum(int(m.sum()) for m in ref.marks) > 0


@pytest.mark.parametrize("loaded", [True, False])
def test_reserved_flag_bits_have_no_effect(eng_mod, so, refs, loaded):
    """Caller bits 0x20 / 0x40 change nothing, with the mark pass (rules
    loaded) and without it (the caller's flags go to the sort as they are)."""
    ref = refs("xflow")
    rng = np.random.default_rng(3)
    e = ref.engine(eng_mod)
    try:
        if not loaded:
            assert e.load_authority_rules([]) == 0
        ora = so.OracleEngine(ref.w["cfg"]) if not loaded else None
        if ora:
            _load(ora, ref.w)
        for k, b in enumerate(ref.batches):
            nb = abi.HostBatch(b.res_id, b.ts_ms, b.count, b.flags | rng.choice([0, 0x20, 0x40, 0x60], b.n).astype(np.uint8),
                               entry_ref=b.entry_ref, create_ts=b.create_ts, origin=b.origin, context=b.context)
            want = ref.want[k] if loaded else ora.submit(b)
            parity.compare_verdicts(e.submit(nb), want, f"batch {k}")
        if ora:
            ora.close()
    finally:
        e.close()


# ---------------------------------------------------------------- SystemRule, degrade
@pytest.mark.parametrize("kind", ["qps", "thread"])
def test_system_rule_planner_skips_marked_entries(eng_mod, refs, kind):
    """AuthoritySlot runs before SystemSlot: a marked IN entry is a block on
    ENTRY_NODE that the planner never classifies."""
    ref = refs("system_" + kind)
    assert ref.rules[0].strategy == am.AUTHORITY_BLACK        # a black list on the busiest resource
    marked_in = sum(int((m & ((b.flags & abi.EV_IN) != 0)).sum()) for b, m in zip(ref.batches, ref.marks))
    assert marked_in > 0 and ref.count(abi.V_BLOCK_AUTHORITY) > 0 and ref.count(abi.V_BLOCK_SYSTEM) > 0
    e = ref.engine(eng_mod)
    try:
        for k, b in enumerate(ref.batches):
            parity.compare_verdicts(e.submit(b), ref.want[k], f"batch {k}")
        ref.compare_state(e)
    finally:
        e.close()


@pytest.mark.parametrize("heavy_min", [512, 8])
def test_degrade_chain_never_sees_marked_entries(eng_mod, refs, heavy_min):
    """Breakers inside sf_submit: a marked entry is never probed, its exit completes nothing."""
    from tests import test_degrade_chain as tc
    ref = refs("chain")
    assert ref.count(abi.V_BLOCK_AUTHORITY) > 0 and ref.count(abi.V_BLOCK_DEGRADE) > 0
    e = ref.engine(eng_mod, heavy_min_events=heavy_min)
    try:
        for k, b in enumerate(ref.batches):
            parity.compare_verdicts(e.submit(b), ref.want[k], f"batch {k}")
        assert np.array_equal(tc._breaker_rows(e, ref.n_breakers), tc._breaker_rows(ref.ora, ref.n_breakers))
        ref.compare_state(e)
    finally:
        e.close()


def test_degrade_only_chain(eng_mod):
    """sf_degrade_submit marks first: oracle/degrade.py on the pre-flagged batches."""
    from oracle import degrade as od
    R = 3000
    rules = trace.degrade_rules(R, seed=7)
    full = trace.degrade_workload(R, 60_000, duration_ms=8000, seed=7, err_p=0.2)
    w = ac.add_origins(dict(batches=[full.subset(0, full.n // 2), full.subset(full.n // 2, full.n)]), seed=9)
    it, mgr = am.Interner(), am.AuthorityRuleManager()
    mgr.load_rules(ac.pick_rules(w["batches"], R, it, seed=9, share=0.1, listed=2))
    parts = [ac.split_for(mgr, b, it) for b in w["batches"]]
    o = od.DegradeOracle()
    n = o.load_rules(rules)
    e = eng_mod.FlowEngine(abi.default_config(max_resources=R, max_batch=max(b.n for b in w["batches"])))
    try:
        assert e.load_degrade_rules(rules) == n
        e.load_authority_rules(am.to_tables(mgr.get_rules(), ac.res_id, it))
        seen = []
        for k, (eb, ob, mark) in enumerate(parts):
            st, ri = o.submit(ob.res_id, ob.ts_ms, ob.flags, ob.entry_ref, ob.create_ts)
            assert (st[mark] == abi.V_BLOCK_OTHER).all() and mark.sum() > 0
            st = st.copy()
            st[mark] = abi.V_BLOCK_AUTHORITY
            v = e.degrade_submit(eb)
            bad = np.nonzero(v.status != st)[0]
            assert bad.size == 0, f"batch {k}: {bad.size} verdicts differ, first at {bad[:5]}"
            blk = st == od.V_BLOCK_DEGRADE
            assert np.array_equal(v.rule_idx[blk], ri[blk]) and np.all(v.rule_idx[mark] == 0)
            seen.append(st)
        for k in range(n):
            assert e.read_breaker(k) == o.state(k), f"breaker {k}"
        allst = np.concatenate(seen)
        assert (allst == od.V_BLOCK_DEGRADE).sum() > 0 and (allst == abi.V_EXIT_IGNORED).sum() > 0
    finally:
        e.close()


# ---------------------------------------------------------------- two engines on one GPU
def _node_workload(kind):
    from tests.test_system_exchange import exchange_workload
    if kind == "exchange":                                    # an inbound-QPS rule: the per-window exchange
        w, batches = exchange_workload("mixed", 30_000)
        w["batches"] = batches
        return w
    return workloads.system("thread")                         # a thread rule: the event all-gather fallback


@pytest.mark.parametrize("kind", ["exchange", "gather"])
def test_two_engines_equal_one_replay(eng_mod, so, kind):
    """shard_count 2 through system_shard.submit_node with LocalComm: every
    rank loads the whole rule list (the loader keeps its shard's), marks its own
    events, and the node's verdicts and ENTRY_NODE equal one replay."""
    from tests.test_system_exchange import _rank_cfg, _threads
    from tests.test_system_shard import _load as load_rank, _merge
    ref = Ref(so, ac.add_origins(_node_workload(kind), seed=11), seed=6, share=0.2, listed=2)
    assert ref.count(abi.V_BLOCK_AUTHORITY) > 0 and ref.count(abi.V_BLOCK_SYSTEM) > 0
    world = 2

    def rank(r, comm):
        e = eng_mod.FlowEngine(_rank_cfg(ref.w, ref.batches, world, r))
        try:
            load_rank(e, ref.w, world, r)
            kept = e.load_authority_rules(ref.tables)
            assert kept == sum(1 for x in ref.mgr.get_rules() if ac.res_id(x.resource) % world == r)
            pos, cols, off = [], [], 0
            for b in ref.batches:
                sel = np.nonzero(b.res_id % world == r)[0]
                v = system_shard.submit_node(e, b.shard(world, r), sel + off, comm)
                pos.append(sel + off)
                cols.append(np.stack([v.status, v.wait_ms, v.rule_idx]).astype(np.int64))
                off += b.n
            return np.concatenate(pos), np.concatenate(cols, axis=1), abi.node_state_to_dict(
                e.read_entry_node(), ref.w["cfg"].sample_count)
        finally:
            e.close()
    parts = _threads(rank, world)
    want = np.concatenate([np.stack([v.status, v.wait_ms, v.rule_idx]).astype(np.int64) for v in ref.want], axis=1)
    got = _merge(parts, want.shape[1])
    bad = np.nonzero((got != want).any(axis=0))[0]
    assert bad.size == 0, f"{bad.size} verdicts differ; first {bad[0]}: got {got[:, bad[0]]} want {want[:, bad[0]]}"
    want_en = abi.node_state_to_dict(ref.ora.read_entry_node(), ref.w["cfg"].sample_count)
    for p in parts:
        assert p[2] == want_en
    ref.ora.close()


# ---------------------------------------------------------------- reloads, both routes, no rules
def test_reload_between_batches(eng_mod, so):
    """Three batches under three maps (a rule list, a different one, none):
    each is decided under the map in force, node and controller state carry across."""
    w = workloads.multi_rule()
    full = w["batches"][0]
    cuts = [0, full.n // 3, 2 * full.n // 3, full.n]
    w["batches"] = [full.subset(cuts[i], cuts[i + 1]) for i in range(3)]
    ac.add_origins(w, seed=13)
    it = am.Interner()
    R = w["cfg"].max_resources
    lists = [ac.pick_rules(w["batches"], R, it, seed=1, share=0.3, listed=2),
             ac.pick_rules(w["batches"], R, it, seed=2, share=0.5, listed=3), []]
    mgr = am.AuthorityRuleManager()
    e, ora = eng_mod.FlowEngine(w["cfg"]), so.OracleEngine(w["cfg"])
    try:
        _load(e, w)
        _load(ora, w)
        counts = []
        for k, (b, rules) in enumerate(zip(w["batches"], lists)):
            mgr.load_rules(rules)
            assert e.load_authority_rules(am.to_tables(rules, ac.res_id, it)) == len(mgr.get_rules())
            eb, ob, mark = ac.split_for(mgr, b, it)
            parity.compare_verdicts(e.submit(eb), ac.expected(ora.submit(ob), mark), f"batch {k}")
            counts.append(int(mark.sum()))
        assert counts[0] > 0 and counts[1] > 0 and counts[2] == 0 and counts[0] != counts[1]
        parity.compare_all_nodes(e, ora, R, sample_count=w["cfg"].sample_count)
        parity.compare_all_rule_states(e, ora, w["n_flow"])
        parity.compare_entry_node(e, ora, sample_count=w["cfg"].sample_count)
    finally:
        e.close()
        ora.close()


def test_both_routes_in_one_batch(eng_mod, refs):
    """Caller-flagged entries (verdict 9) beside engine-marked ones (verdict
    10); a caller-flagged entry a rule would also block stays 9."""
    ref = refs("xflow_both")
    assert ref.count(abi.V_BLOCK_OTHER) > 0 and ref.count(abi.V_BLOCK_AUTHORITY) > 0
    both = 0
    for b in ref.batches:
        would = am.blocked_mask(ref.mgr, ac.res_name, b.res_id, b.origin, b.flags & ~np.uint8(abi.EV_BLOCKED), ref.it)
        both += int((would & ((b.flags & abi.EV_BLOCKED) != 0)).sum())
    assert both > 0
    e = ref.engine(eng_mod)
    try:
        for k, b in enumerate(ref.batches):
            parity.compare_verdicts(e.submit(b), ref.want[k], f"batch {k}")
        ref.compare_state(e)
    finally:
        e.close()


def test_no_rules_loaded_changes_nothing(eng_mod, refs):
    """Verdicts byte-identical to an engine whose loader was never called."""
    ref = refs("xflow")
    a, b = eng_mod.FlowEngine(ref.w["cfg"]), eng_mod.FlowEngine(ref.w["cfg"])
    try:
        _load(a, ref.w)
        _load(b, ref.w)
        assert a.load_authority_rules(ref.tables) > 0 and a.load_authority_rules([]) == 0    # loaded, then cleared
        for hb in ref.w["batches"]:
            x, y = a.submit(hb), b.submit(hb)
            assert x.status.tobytes() == y.status.tobytes() and x.wait_ms.tobytes() == y.wait_ms.tobytes()
            assert x.rule_idx.tobytes() == y.rule_idx.tobytes()
            assert not (x.status == abi.V_BLOCK_AUTHORITY).any()
    finally:
        a.close()
        b.close()
