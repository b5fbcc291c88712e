"""Host form against device form of every batch entry point that takes both
(sf_submit, sf_submit_packed, sf_request_tokens, sf_request_concurrent,
sf_degrade_submit, sf_serve_frames): the same small batch through two fresh
engines loaded alike, one given host arrays, the other device arrays with the
results read back.  Every result array must be byte-identical.  The host form
is pinned to the oracle by the other suites; this is the net under the staging
code, at the sizes where the 1-byte arrays shift the piece after them.
Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from sentinel_amd import abi, trace

pytestmark = pytest.mark.gpu

NS = (1, 255, 256, 257)
R = 8


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


def same(host, dev, what):
    assert host.dtype == dev.dtype and host.shape == dev.shape, what
    assert host.tobytes() == dev.tobytes(), f"{what}: host and device forms differ"


# ---------------------------------------------------------------- event batches
# name -> (batch options, result arrays asked for)
EVENT_CASES = {
    "plain": ({}, True),
    "exits": (dict(exits=True), True),
    "exits_create_ts": (dict(exits=True, create_ts=True), True),
    "origin": (dict(exits=True, origin=True), True),
    "origin_context": (dict(origin=True, context=True), True),
    "args": (dict(args=True), True),
    "args_n_args": (dict(exits=True, args=True, n_args=True), True),
    "collections_no_elems": (dict(args=True, coll=True), True),
    "status_only": (dict(exits=True), False),
}


def event_batch(n, exits=False, create_ts=False, origin=False, context=False, args=False, n_args=False, coll=False,
                degrade=False):
    """n time-ordered events on R resources; with `exits`, about a third are
    the EXIT of an earlier entry (same resource, count and origin)."""
    rng = np.random.default_rng(1000 + n)
    res = rng.integers(0, R, n).astype(np.uint32)
    ts = trace.T0 + np.sort(rng.integers(0, 1500, n)).astype(np.int64)
    cnt = rng.integers(1, 4, n).astype(np.int32)
    og = rng.integers(2, 6, n).astype(np.uint32)
    flags = np.full(n, 0 if degrade else abi.EV_IN, np.uint8)
    eref = np.full(n, -1, np.int64)
    cts = np.zeros(n, np.int64)
    open_entries = []
    for i in range(n):
        if exits and open_entries and rng.random() < 0.4:
            j = open_entries.pop(int(rng.integers(len(open_entries))))
            res[i], cnt[i], og[i], eref[i], cts[i] = res[j], cnt[j], og[j], j, ts[j]
            flags[i] |= abi.EV_EXIT | (abi.EV_ERROR if degrade and rng.random() < 0.3 else 0)
        else:
            open_entries.append(i)
    kw = {}
    if args:
        kw.update(arg_tag=np.full((1, n), abi.TAG_LONG, np.uint8), arg_bits=rng.integers(0, 5, (1, n)).astype(np.uint64))
    if n_args:
        kw.update(n_args=rng.integers(0, 2, n).astype(np.uint8))
    if coll:
        kw.update(elem_off=np.zeros(n + 1, np.uint32), elem_tag=np.zeros(0, np.uint8), elem_bits=np.zeros(0, np.uint64))
    return abi.HostBatch(res, ts, cnt, flags, entry_ref=eref if exits else None,
                         create_ts=cts if create_ts else None, origin=og if origin else None,
                         context=rng.integers(0, 3, n).astype(np.uint32) if context else None, **kw)


def flow_engine(eng_mod):
    e = eng_mod.FlowEngine(abi.default_config(max_resources=R, max_batch=512))
    grades = [abi.GRADE_QPS, abi.GRADE_THREAD] * (R // 2)
    behaviors = [abi.BEHAVIOR_DEFAULT, abi.BEHAVIOR_DEFAULT, abi.BEHAVIOR_WARM_UP, abi.BEHAVIOR_DEFAULT,
                 abi.BEHAVIOR_RATE_LIMITER, abi.BEHAVIOR_DEFAULT, abi.BEHAVIOR_DEFAULT, abi.BEHAVIOR_DEFAULT]
    e.load_flow_rules(trace.flow_rules_from_counts([3, 2, 5, 4, 6, 3, 20, 2], behaviors=behaviors, grades=grades,
                                                   max_queue=200))
    e.load_param_rules([abi.sf_param_rule(resource=r, grade=abi.GRADE_QPS, param_idx=0, control_behavior=0,
                                          count=2.0 + r, max_queueing_time_ms=0, burst_count=0, duration_in_sec=1,
                                          item_offset=0, item_count=0) for r in range(R)])
    return e


def host_verdicts(n, full):
    v = abi.HostVerdicts(n)
    if not full:
        v.wait_ms = v.rule_idx = None
    return v


def same_verdicts(host, dv, what):
    same(host.status, dv.status.numpy(), what + " status")
    if host.wait_ms is not None:
        same(host.wait_ms, dv.wait_ms.numpy(), what + " wait_ms")
        same(host.rule_idx, dv.rule_idx.numpy(), what + " rule_idx")


@pytest.mark.parametrize("case", list(EVENT_CASES))
@pytest.mark.parametrize("n", NS)
def test_submit_forms(eng_mod, n, case):
    opts, full = EVENT_CASES[case]
    hb = event_batch(n, **opts)
    eh, ed = flow_engine(eng_mod), flow_engine(eng_mod)
    host = eh.submit(hb, host_verdicts(n, full))
    db, dv = eng_mod.DeviceBatch(ed, hb), eng_mod.DeviceVerdicts(ed, n, with_wait=full, with_rule=full)
    ed.submit_device(db, dv)
    same_verdicts(host, dv, f"sf_submit {case} n={n}")
    eh.close(); ed.close()


PACKED_ARRAYS = ("ev", "exit_ref", "exit_cts", "count_ext", "origin", "ev4", "ms_end", "arg_event", "arg_off",
                 "arg_tag", "arg_bits", "elem_off", "elem_tag", "elem_bits", "context")


@pytest.mark.parametrize("case", list(EVENT_CASES))
@pytest.mark.parametrize("n", NS)
def test_submit_packed_forms(eng_mod, n, case):
    opts, full = EVENT_CASES[case]
    pb = abi.PackedBatch(event_batch(n, **opts), narrow=(n == 255))
    eh, ed = flow_engine(eng_mod), flow_engine(eng_mod)
    host = eh.submit_packed(pb, host_verdicts(n, full))
    b = pb.c_struct()
    b.mem = abi.MEM_DEVICE
    for name in PACKED_ARRAYS:
        a = getattr(pb, name)
        setattr(b, name, None if a is None else eng_mod.DeviceArray(ed, a).ptr)
    dv = eng_mod.DeviceVerdicts(ed, n, with_wait=full, with_rule=full)
    v = dv.c_struct()
    eng_mod._check(eng_mod.lib().sf_submit_packed(ed.h, C.byref(b), C.byref(v)))
    same_verdicts(host, dv, f"sf_submit_packed {case} n={n}")
    eh.close(); ed.close()


# ---------------------------------------------------------------- DegradeSlot breakers
DEGRADE_CASES = {
    "entry_ref": (dict(exits=True), True),
    "entry_ref_create_ts": (dict(exits=True, create_ts=True), True),
    "origin_marked": (dict(exits=True, origin=True), True),
    "status_only": (dict(exits=True), False),
}


@pytest.mark.parametrize("case", list(DEGRADE_CASES))
@pytest.mark.parametrize("n", NS)
def test_degrade_submit_forms(eng_mod, n, case):
    opts, full = DEGRADE_CASES[case]
    hb = event_batch(n, degrade=True, **opts)
    engines = []
    for _ in range(2):
        e = eng_mod.FlowEngine(abi.default_config(max_resources=R, max_batch=512))
        e.load_degrade_rules(trace.degrade_rules(R, seed=5, frac=1.0))
        e.load_authority_rules([(r, abi.AUTHORITY_BLACK, [2, 3]) for r in range(0, R, 2)])
        engines.append(e)
    eh, ed = engines
    host = host_verdicts(n, full)
    b, v = hb.c_struct(), host.c_struct()
    eng_mod._check(eng_mod.lib().sf_degrade_submit(eh.h, C.byref(b), C.byref(v)))
    db, dv = eng_mod.DeviceBatch(ed, hb), eng_mod.DeviceVerdicts(ed, n, with_wait=full, with_rule=full)
    ed.degrade_submit_device(db, dv)
    same_verdicts(host, dv, f"sf_degrade_submit {case} n={n}")
    eh.close(); ed.close()


# ---------------------------------------------------------------- cluster token server
def token_engine(eng_mod, ns, flow, param, items):
    e = eng_mod.FlowEngine(abi.default_config(max_resources=4, max_batch=1 << 12))
    e.load_namespaces(ns)
    e.load_cluster_rules(flow, param, items)
    return e


def token_batch(n, case):
    ns, flow, param, items, b = trace.token_workload(n, n_flow=20, n_param=6, n_values=50, duration_ms=1500, seed=n)
    if case == "no_params":
        b = abi.HostTokenBatch(b.flow_id, b.count, b.flags & ~np.uint8(abi.TOK_PARAM), b.ts_ms)
    elif case == "param_off_empty":                 # every request a collection of no values
        b = abi.HostTokenBatch(b.flow_id, b.count, b.flags, b.ts_ms, np.zeros(0, np.uint8), np.zeros(0, np.uint64),
                               np.zeros(n + 1, np.uint32))
    elif case == "param_off":                       # collections of 0..3 values
        rng = np.random.default_rng(n)
        off = np.concatenate([[0], np.cumsum(rng.integers(0, 4, n))]).astype(np.uint32)
        m = int(off[-1])
        b = abi.HostTokenBatch(b.flow_id, b.count, b.flags, b.ts_ms, np.full(m, abi.TAG_LONG, np.uint8),
                               rng.integers(0, 50, m).astype(np.uint64), off)
    return ns, flow, param, items, b


@pytest.mark.parametrize("case", ["no_params", "params", "param_off", "param_off_empty", "status_only"])
@pytest.mark.parametrize("n", NS)
def test_request_tokens_forms(eng_mod, n, case):
    ns, flow, param, items, tb = token_batch(n, case)
    eh, ed = token_engine(eng_mod, ns, flow, param, items), token_engine(eng_mod, ns, flow, param, items)
    full = case != "status_only"
    host = abi.HostTokenResults(n)
    if not full:
        host.remaining = host.wait_ms = None
    b, r = tb.c_struct(), host.c_struct()
    eng_mod._check(eng_mod.lib().sf_request_tokens(eh.h, C.byref(b), C.byref(r)))
    b = tb.c_struct()
    b.mem = abi.MEM_DEVICE
    for name in ("flow_id", "count", "flags", "ts_ms", "param_tag", "param_bits", "param_off"):
        a = getattr(tb, name)
        setattr(b, name, None if a is None else eng_mod.DeviceArray(ed, a).ptr)
    if full:
        res = {k: eng_mod.DeviceArray.empty(ed, n, dt) for k, dt in
               (("status", np.int8), ("remaining", np.int32), ("wait_ms", np.int32))}
        r = abi.sf_token_results(abi.MEM_DEVICE, res["status"].ptr, res["remaining"].ptr, res["wait_ms"].ptr)
        eng_mod._check(eng_mod.lib().sf_request_tokens(ed.h, C.byref(b), C.byref(r)))
        for k, a in res.items():
            same(getattr(host, k), a.numpy(), f"sf_request_tokens {case} n={n} {k}")
    else:           # device results need all three arrays: device inputs, host results without the optional two
        dev = abi.HostTokenResults(n)
        dev.remaining = dev.wait_ms = None
        r = dev.c_struct()
        eng_mod._check(eng_mod.lib().sf_request_tokens(ed.h, C.byref(b), C.byref(r)))
        same(host.status, dev.status, f"sf_request_tokens {case} n={n} status")
    eh.close(); ed.close()


# ---------------------------------------------------------------- cluster concurrency tokens
@pytest.mark.parametrize("n", NS)
def test_request_concurrent_forms(eng_mod, n):
    """Acquires, then a batch that releases half of the tokens (the ids of a
    form's own first batch) among new acquires."""
    rng = np.random.default_rng(n)
    flow = [abi.sf_cluster_flow_rule(f, 40.0 + f, abi.THRESHOLD_GLOBAL, 0, 10, 1000) for f in range(1, 6)]
    first = abi.HostConcurrentBatch(np.full(n, abi.CC_ACQUIRE, np.uint8), rng.integers(1, 7, n), rng.integers(1, 3, n),
                                    rng.integers(0, 4, n), np.full(n, trace.T0))
    op2 = (rng.random(n) < 0.5).astype(np.uint8)
    acq2 = rng.integers(1, 7, n)
    results = []
    for device in (False, True):
        e = token_engine(eng_mod, [], flow, [], [])
        got = []
        ids = None
        for k in range(2):
            cb = first if k == 0 else abi.HostConcurrentBatch(op2, np.where(op2 == abi.CC_RELEASE, ids, acq2),
                                                              first.count, first.client, np.full(n, trace.T0 + 5))
            out = abi.HostConcurrentResults(n)
            b, r = cb.c_struct(), out.c_struct()
            if device:
                b.mem = r.mem = abi.MEM_DEVICE
                for name in ("op", "id", "count", "client", "ts_ms"):
                    setattr(b, name, eng_mod.DeviceArray(e, getattr(cb, name)).ptr)
                st, tid = eng_mod.DeviceArray.empty(e, n, np.int8), eng_mod.DeviceArray.empty(e, n, np.int64)
                r.status, r.token_id = st.ptr, tid.ptr
            eng_mod._check(eng_mod.lib().sf_request_concurrent(e.h, C.byref(b), C.byref(r)))
            if device:
                out.status, out.token_id = st.numpy(), tid.numpy()
            ids = out.token_id
            got.append(out)
        results.append(got)
        e.close()
    for k in range(2):
        what = f"sf_request_concurrent n={n} batch {k}"
        h, d = results[0][k], results[1][k]
        same(h.status, d.status, what + " status")
        # the slot number inside an id is whatever the free stack held: its order
        # is decided by atomics among threads (cc_push, k_cc_commit) and differs
        # from run to run in either form.  What is fixed: which requests get an id.
        same(h.token_id != 0, d.token_id != 0, what + " token_id issued")


# ---------------------------------------------------------------- wire framing
@pytest.mark.parametrize("n", NS)
def test_serve_frames_forms(eng_mod, n):
    """n requests as frames over up to 7 connections (the results of
    sf_serve_frames are host arrays in both forms: only the inputs move)."""
    ns, flow, param, items, streams = trace.wire_workload(n, n_streams=min(n, 7), edge=True, seed=40 + n, n_flow=20,
                                                          n_param=6, n_values=50, duration_ms=1500)
    eh, ed = token_engine(eng_mod, ns, flow, param, items), token_engine(eng_mod, ns, flow, param, items)
    now = trace.T0 + 700
    host = eh.serve_frames(streams, now)
    dev = abi.WireResult(streams, now)
    b, o = dev.c_structs()
    b.mem = abi.MEM_DEVICE
    b.bytes, b.stream_off = eng_mod.DeviceArray(ed, dev.data).ptr, eng_mod.DeviceArray(ed, dev.off).ptr
    eng_mod._check(eng_mod.lib().sf_serve_frames(ed.h, C.byref(b), C.byref(o)))
    dev.finish(o)
    what = f"sf_serve_frames n={n}"
    assert (host.n_frames, host.n_requests, host.n_responses) == (dev.n_frames, dev.n_requests, dev.n_responses), what
    for k in ("resp", "resp_off", "consumed", "stop"):
        same(getattr(host, k), getattr(dev, k), f"{what} {k}")
    eh.close(); ed.close()
