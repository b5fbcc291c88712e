"""ParamFlow arguments, collection elements and context names in the compact
batch forms (sf_packed_batch's argument tables, include/sentinel_flow.h).

CPU: abi.PackedBatch carries them losslessly (a numpy unpack gives back what
the SoA batch holds), the two NULL shortcuts cost 9 bytes per event and slot,
and the expansion / validation the device runs (sentinel_amd/csrc/sf_pkargs.h)
is checked stand-alone under the address and undefined-behaviour sanitizers
(tests/packed_args_check.cpp): valid tables expand to a direct construction,
every malformed table is refused without an access outside its arrays.

GPU: packed batches with arguments, collections and contexts -- synchronous,
asynchronous and double-buffered over page-locked arrays, both word widths,
dense and sparse verdicts, under a SystemRule -- give the oracle's verdicts and
node state; the per-batch buffer grows and is recycled in one async stream; a
malformed table is SF_ERR_INVALID at the call or at the batch's own sync, and
the engine decides the next batch correctly."""
import os
import subprocess

import numpy as np
import pytest

from sentinel_amd import abi, trace
from tests import workloads

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- CPU: the wire form
def _unpack_args(pb: abi.PackedBatch):
    """(n_args [n], tag [slots, n], bits [slots, n], {(slot, event): [(tag, bits)...]}) of a packed batch."""
    n, S = pb.n, pb.arg_slots
    na = np.zeros(n, np.uint8)
    tag = np.zeros((S, n), np.uint8)
    bits = np.zeros((S, n), np.uint64)
    elems = {}
    if pb.arg_event is None:
        assert pb.n_arg_events in (0, n)
        ev = np.arange(pb.n_arg_events)
    else:
        ev = pb.arg_event
        assert ev.shape == (pb.n_arg_events,) and (np.diff(ev.astype(np.int64)) > 0).all() and ev[-1] < n
    if pb.arg_off is None:
        off = np.arange(pb.n_arg_events + 1) * S
    else:
        off = pb.arg_off
        assert off.shape == (pb.n_arg_events + 1,)
    assert int(off[-1]) == pb.n_values
    if pb.n_values:
        assert pb.arg_tag.shape == pb.arg_bits.shape == (pb.n_values,)
    if pb.elem_off is not None:
        assert pb.elem_off.shape == (pb.n_values + 1,) and int(pb.elem_off[-1]) == pb.n_elems
        assert pb.elem_tag.shape == pb.elem_bits.shape == (pb.n_elems,)
    for j, i in enumerate(ev):
        lo, hi = int(off[j]), int(off[j + 1])
        assert 0 <= hi - lo <= S
        na[i] = hi - lo
        for s in range(hi - lo):
            v = lo + s
            tag[s, i], bits[s, i] = pb.arg_tag[v], pb.arg_bits[v]
            if pb.arg_tag[v] == abi.TAG_COLLECTION:
                a, b = int(pb.elem_off[v]), int(pb.elem_off[v + 1])
                elems[(s, int(i))] = list(zip(pb.elem_tag[a:b].tolist(), pb.elem_bits[a:b].tolist()))
    return na, tag, bits, elems


def _assert_roundtrip(hb: abi.HostBatch, pb: abi.PackedBatch):
    n = hb.n
    slots = 0 if hb.arg_tag is None else hb.arg_tag.shape[0]
    want_na = np.zeros(n, np.uint8) if not slots else (np.full(n, slots, np.uint8) if hb.n_args is None else hb.n_args)
    na, tag, bits, elems = _unpack_args(pb)
    assert np.array_equal(na, want_na)
    n_coll = 0
    for s in range(slots):
        live = want_na > s
        assert np.array_equal(tag[s][live], hb.arg_tag[s][live])
        scalar = live & (hb.arg_tag[s] != abi.TAG_COLLECTION)
        assert np.array_equal(bits[s][scalar], hb.arg_bits[s][scalar])
        for i in np.nonzero(live & (hb.arg_tag[s] == abi.TAG_COLLECTION))[0]:
            k = s * n + int(i)
            a, b = int(hb.elem_off[k]), int(hb.elem_off[k + 1])
            assert elems[(s, int(i))] == list(zip(hb.elem_tag[a:b].tolist(), hb.elem_bits[a:b].tolist()))
            n_coll += 1
    assert n_coll == len(elems)
    if hb.context is None:
        assert pb.context is None
    else:
        assert np.array_equal(pb.context, hb.context)
    return n_coll


@pytest.mark.parametrize("narrow", [False, True])
def test_roundtrip_param_mixed(narrow):
    hb = workloads.param_mixed()["batches"][0]
    pb = abi.PackedBatch(hb, narrow=narrow)
    assert pb.arg_event is not None and pb.arg_off is not None           # n_args 0..2: the explicit lists
    assert pb.n_arg_events == int((hb.n_args > 0).sum()) < hb.n
    assert _assert_roundtrip(hb, pb) == 0


def test_roundtrip_param_collections():
    total = 0
    for hb in workloads.param_collections()["batches"]:
        pb = abi.PackedBatch(hb)
        assert pb.elem_off is not None and pb.n_elems > 0
        total += _assert_roundtrip(hb, pb)
    assert total > 1000                                                  # collections, some with null elements


def test_roundtrip_xflow_contexts():
    for hb in workloads.xflow()["batches"]:
        pb = abi.PackedBatch(hb)
        assert pb.n_arg_events == 0 and pb.arg_tag is None
        assert np.array_equal(pb.origin, hb.origin)
        _assert_roundtrip(hb, pb)
        assert len(np.unique(pb.context)) > 1


def test_shortcut_byte_count():
    """Config 4's traffic (one LONG argument on every event): both shortcuts,
    13 bytes per event in the narrow form against the SoA form's 26."""
    _, hb = trace.param_zipf(40, 50_000, 5000)
    pb = abi.PackedBatch(hb, narrow=True)
    assert pb.arg_event is None and pb.arg_off is None and pb.elem_off is None and pb.context is None
    assert pb.n_arg_events == hb.n and pb.n_values == hb.n and pb.arg_slots == 1
    n = hb.n
    assert pb.nbytes() == 4 * n + 4 * pb.n_ms + 9 * n
    _assert_roundtrip(hb, pb)


def test_struct_layout():
    """The tail sits after pad0, field by field as the header lists it."""
    names = [f for f, _ in abi.sf_packed_batch._fields_]
    tail = ["n_arg_events", "n_values", "arg_slots", "n_elems", "arg_event", "arg_off", "arg_tag", "arg_bits",
            "elem_off", "elem_tag", "elem_bits", "context"]
    assert names[names.index("pad0") + 1:] == tail
    assert abi.SF_ABI_VERSION == 2
    z = abi.PackedBatch(trace.mixed_zipf(50, 1000, seed=1)).c_struct()       # no arguments: a zeroed tail
    assert all(not getattr(z, f) for f in tail)


@pytest.fixture(scope="module")
def args_check_passed(tmp_path_factory):
    """tests/packed_args_check.cpp under ASan + UBSan: run before any malformed table reaches a GPU."""
    exe = str(tmp_path_factory.mktemp("pkargs") / "packed_args_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(HERE, "packed_args_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
    return True


def test_expansion_and_validation_under_sanitizers(args_check_passed):
    assert args_check_passed


# ---------------------------------------------------------------- GPU
MALFORMED = ["index_ge_n", "arg_event_equal", "arg_event_decreasing", "arg_event_duplicate_apart",
             "arg_off_decreasing", "span_above_slots", "arg_off_last", "elem_off_decreasing", "elem_off_last",
             "collection_without_elem_off"]


def _break(pb: abi.PackedBatch, case: str):
    """One entry of a valid table (explicit lists, collections) changed."""
    if case == "index_ge_n":
        pb.arg_event[-1] = pb.n
    elif case == "arg_event_equal":
        pb.arg_event[5] = pb.arg_event[4]
    elif case == "arg_event_decreasing":
        pb.arg_event[5] = pb.arg_event[3]
    elif case == "arg_event_duplicate_apart":
        # entries 5 and 7 name one event and each passes its own neighbour check; only entry 6 fails
        pb.arg_event[6] = pb.arg_event[4] - 1
        pb.arg_event[7] = pb.arg_event[5]
    elif case == "arg_off_decreasing":
        pb.arg_off[4] = pb.arg_off[3] - 1
    elif case == "span_above_slots":
        span = np.diff(pb.arg_off.astype(np.int64))
        j = int(np.nonzero((span[:-1] == pb.arg_slots) & (span[1:] >= 1))[0][0])
        pb.arg_off[j + 1] += 1
    elif case == "arg_off_last":
        pb.arg_off[-1] -= 1
    elif case == "elem_off_decreasing":
        v = int(np.nonzero(pb.elem_off)[0][0])
        assert v + 2 < pb.elem_off.size
        pb.elem_off[v + 1] = pb.elem_off[v] - 1
    elif case == "elem_off_last":
        pb.elem_off[-1] = pb.n_elems - 1
    elif case == "collection_without_elem_off":
        pb.elem_off = pb.elem_tag = pb.elem_bits = None
        pb.n_elems = 0
    else:
        raise KeyError(case)


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


class _Ref:
    """A workload decided once by the oracle: its batches, the oracle's verdicts
    of each and the oracle engine left as it is after the last one (read only)."""

    def __init__(self, w, parts, system=(), status=None):
        from oracle.oracle import OracleEngine
        self.w, self.parts = w, parts
        self.ora = OracleEngine(w["cfg"])
        if status is not None:
            self.ora.set_system_status(*status)
        self.load(self.ora, system)
        self.want = [self.ora.submit(p) for p in parts]
        self.system, self.status = system, status

    def load(self, x, system=()):
        if system:
            x.load_system_rules(list(system))
        if self.w.get("flow"):
            x.load_flow_rules(list(self.w["flow"]))
        if self.w.get("param"):
            x.load_param_rules(list(self.w["param"]), list(self.w.get("items", ())))

    def engine(self, eng_mod):
        e = eng_mod.FlowEngine(self.w["cfg"])
        if self.status is not None:
            e.set_system_status(*self.status)
        self.load(e, self.system)
        return e

    def compare_state(self, eng):
        from tests import parity
        cfg = self.w["cfg"]
        parity.compare_all_nodes(eng, self.ora, cfg.max_resources, sample_count=cfg.sample_count)
        parity.compare_entry_node(eng, self.ora, sample_count=cfg.sample_count)
        if self.w.get("n_flow"):
            parity.compare_all_rule_states(eng, self.ora, self.w["n_flow"])


@pytest.fixture(scope="module")
def refs():
    made = {}

    def get(name):
        if name in made:
            return made[name]
        if name == "param_mixed":
            w = workloads.param_mixed()
            b = w["batches"][0]
            cuts = np.linspace(0, b.n, 4).astype(int)
            r = _Ref(w, [b.subset(int(cuts[k]), int(cuts[k + 1])) for k in range(3)])
        elif name == "param_collections":
            w = workloads.param_collections()
            r = _Ref(w, w["batches"])
        elif name == "xflow":
            w = workloads.xflow(n=30_000, split=3)
            r = _Ref(w, w["batches"])
        elif name == "system":
            w = workloads.config4()
            n = w["batches"][0].n
            sysr = [abi.sf_system_rule(highest_system_load=-1, highest_cpu_usage=-1, qps=0.6 * n / 4.0,
                                       avg_rt=-1, max_thread=-1)]
            r = _Ref(w, w["batches"], system=sysr, status=(0.0, 0.0))
        elif name == "growth":
            w = workloads.param_collections()
            b0, b1 = w["batches"]
            a = b0.subset(0, 5000)
            tg = a.arg_tag[:1].copy()
            tg[tg == abi.TAG_COLLECTION] = abi.TAG_LONG                  # one slot, scalars only
            a = abi.HostBatch(a.res_id, a.ts_ms, a.count, a.flags, entry_ref=a.entry_ref, create_ts=a.create_ts,
                              arg_tag=tg, arg_bits=a.arg_bits[:1], n_args=np.minimum(a.n_args, 1))
            p = b0.subset(5000, 10_000)
            plain = abi.HostBatch(p.res_id, p.ts_ms, p.count, p.flags, entry_ref=p.entry_ref, create_ts=p.create_ts)
            r = _Ref(w, [a, plain, b0.subset(10_000, b0.n), b1])
        else:
            raise KeyError(name)
        made[name] = r
        return r
    yield get
    for r in made.values():
        r.ora.close()


def _run_dense(eng, pin, ref, mode, narrow=False):
    """The parts packed into pinned arrays and decided in `mode`; every batch against the oracle's verdicts."""
    from tests import parity
    pbs = [abi.PackedBatch(p, alloc=pin.array, narrow=narrow) for p in ref.parts]
    outs = [pin.verdicts(p.n) for p in ref.parts]
    if mode == "sync":
        for pb, o in zip(pbs, outs):
            eng.submit_packed(pb, o)
    elif mode == "async":
        for pb, o in zip(pbs, outs):
            eng.submit_packed_async(pb, o)
        eng.sync()
    else:
        eng.submit_packed_async(pbs[0], outs[0])
        for k in range(len(pbs)):
            if k + 1 < len(pbs):
                eng.submit_packed_async(pbs[k + 1], outs[k + 1])
            eng.sync_packed(outs[k])
            parity.compare_verdicts(outs[k], ref.want[k], f"batch {k} (in flight)")
        eng.sync()
    for k, o in enumerate(outs):
        parity.compare_verdicts(o, ref.want[k], f"batch {k}")
    return pbs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sync", "async", "double"])
def test_gpu_param_mixed(eng_mod, refs, mode):
    """Explicit lists, n_args 0..2, nulls, a negative param_idx, THREAD-grade rules with exits."""
    ref = refs("param_mixed")
    assert sum(p.n for p in ref.parts) == 45_000
    eng = ref.engine(eng_mod)
    pin = eng_mod.PinnedArrays(eng)
    try:
        pbs = _run_dense(eng, pin, ref, mode)
        assert all(pb.arg_event is not None for pb in pbs)
        ref.compare_state(eng)
        checked = 0
        for r in ref.w["param"]:
            if r.grade != abi.GRADE_THREAD:
                continue
            for idx in (0, 1):
                for v in range(0, 50, 7):
                    want = ref.ora.param_thread(r.resource, idx, (abi.TAG_LONG, v))
                    assert eng.param_thread(r.resource, idx, (abi.TAG_LONG, v)) == want, (r.resource, idx, v)
                    checked += 1
        assert checked
    finally:
        pin.free()
        eng.close()


@pytest.mark.gpu
def test_gpu_param_collections_narrow_sparse(eng_mod, refs):
    """The value-indexed element CSR through the sort, the thread-count
    callbacks and null elements; the narrow words, sparse verdicts (prefetch 64)."""
    from tests import parity
    ref = refs("param_collections")
    eng = ref.engine(eng_mod)
    pin = eng_mod.PinnedArrays(eng)
    try:
        pbs = [abi.PackedBatch(p, alloc=pin.array, narrow=True) for p in ref.parts]
        assert all(pb.ev4 is not None and pb.n_elems > 0 for pb in pbs)
        outs = [pin.sparse_verdicts(p.n, 64) for p in ref.parts]
        eng.submit_packed_sparse_async(pbs[0], outs[0])
        for k in range(len(pbs)):
            if k + 1 < len(pbs):
                eng.submit_packed_sparse_async(pbs[k + 1], outs[k + 1])
            eng.sync_packed_sparse(outs[k])
            parity.compare_verdicts(outs[k].dense(), ref.want[k], f"batch {k}")
        eng.sync()
        ref.compare_state(eng)
        for r in ref.w["param"]:
            if r.grade == abi.GRADE_THREAD:
                for v in range(0, 30, 5):
                    want = ref.ora.param_thread(r.resource, r.param_idx, (abi.TAG_LONG, v))
                    assert eng.param_thread(r.resource, r.param_idx, (abi.TAG_LONG, v)) == want, (r.resource, v)
    finally:
        pin.free()
        eng.close()


@pytest.mark.gpu
def test_gpu_xflow_origins_and_contexts(eng_mod, refs):
    """Origins and contexts from staged host arrays: CHAIN rules decide on the context node."""
    from tests import parity
    ref = refs("xflow")
    assert ref.w["context_nodes"]
    eng = ref.engine(eng_mod)
    pin = eng_mod.PinnedArrays(eng)
    try:
        pbs = _run_dense(eng, pin, ref, "double")
        assert all(pb.context is not None and pb.origin is not None for pb in pbs)
        ref.compare_state(eng)
        parity.compare_aux_nodes(eng, ref.ora, ref.w["origin_nodes"][:20], ref.w["context_nodes"][:20])
    finally:
        pin.free()
        eng.close()


@pytest.mark.gpu
def test_gpu_system_rule_with_arguments(eng_mod, refs):
    """Config 4's shape under an inbound-QPS SystemRule at 0.6x the offered
    rate: the planner reads the expanded arguments (param_inert) before the
    sort does.  Both shortcuts; the synchronous planner path."""
    ref = refs("system")
    st = ref.want[0].status
    assert (st == abi.V_BLOCK_SYSTEM).any() and (st == abi.V_BLOCK_PARAM).any()
    eng = ref.engine(eng_mod)
    pin = eng_mod.PinnedArrays(eng)
    try:
        pbs = _run_dense(eng, pin, ref, "sync")
        assert pbs[0].arg_event is None and pbs[0].arg_off is None
        ref.compare_state(eng)
    finally:
        pin.free()
        eng.close()


@pytest.mark.gpu
def test_gpu_buffer_growth_and_slot_recycling(eng_mod, refs):
    """One async stream: a one-slot argument batch, a batch without arguments,
    then batches with two slots and collections -- each slot's argument buffer
    is allocated, reused without arguments and grown."""
    ref = refs("growth")
    eng = ref.engine(eng_mod)
    pin = eng_mod.PinnedArrays(eng)
    try:
        pbs = _run_dense(eng, pin, ref, "async")
        assert [pb.arg_slots for pb in pbs] == [1, 0, 2, 2]
        assert pbs[0].n_elems == 0 and 0 < pbs[2].n_elems < pbs[3].n_elems
        ref.compare_state(eng)
    finally:
        pin.free()
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", MALFORMED)
def test_gpu_malformed_table(eng_mod, refs, args_check_passed, case):
    """A malformed table is SF_ERR_INVALID -- at the call when synchronous, at
    the batch's own sync when asynchronous (the cases alternate) -- and reads
    nothing through the bad index (checked under the sanitizers first).  Its
    events are on resources of their own, so the good batches that follow on
    the same engine must equal the oracle's."""
    from tests import parity
    ref = refs("param_collections")
    R = ref.w["cfg"].max_resources
    cfg = abi.default_config(max_resources=2 * R, max_batch=ref.w["cfg"].max_batch, param_capacity=1 << 14)
    eng = eng_mod.FlowEngine(cfg)
    pin = eng_mod.PinnedArrays(eng)
    try:
        ref.load(eng)
        b = ref.parts[0].subset(0, 4000)
        b.res_id = b.res_id + np.uint32(R)                               # resources without rules,
        b.ts_ms = b.ts_ms - 100_000                                      # before the good batches' clock
        bad = abi.PackedBatch(b, alloc=pin.array)
        _break(bad, case)
        o = pin.verdicts(b.n)
        if MALFORMED.index(case) % 2 == 0:
            with pytest.raises(eng_mod.EngineError):
                eng.submit_packed(bad, o)
        else:
            eng.submit_packed_async(bad, o)
            with pytest.raises(eng_mod.EngineError):
                eng.sync_packed(o)
            eng.sync()
        for k, p in enumerate(ref.parts):
            got = pin.verdicts(p.n)
            eng.submit_packed(abi.PackedBatch(p, alloc=pin.array), got)
            parity.compare_verdicts(got, ref.want[k], f"good batch {k} after {case}")
        parity.compare_nodes(eng, ref.ora, range(R))
    finally:
        pin.free()
        eng.close()


def test_java_flusher_fills_the_argument_lists():
    """EventBatcher.flushPacked cannot be run here (no JDK).  This pins the
    statements of its argument loop in the Java source, and checks that the
    same loop written out in Python below gives abi.PackedBatch's tables; it
    does not show that the Java code itself builds them."""
    from tests import javashim as j
    src = j.source("EventBatcher.java")
    fp = src[src.index("private boolean flushPacked"):]
    assert "t.context != 0) return false" not in fp and "t.args.length > 0) ||" not in fp
    for line in ("final int na = t.args == null ? 0 : Math.min(t.args.length, ARG_SLOTS);",
                 "if (na == 0) continue;",
                 "p.pargEvent.setAtIndex(JAVA_INT, nae, i);",
                 "p.pelemOff.setAtIndex(JAVA_INT, nv, ne);",
                 "p.pargOff.setAtIndex(JAVA_INT, nae, nv);",
                 'pk.set(ADDRESS, off(PACKED_BATCH, "context"), anyContext ? p.pcontext : MemorySegment.NULL);'):
        assert line in fp, line
    assert fp.index("p.pargOff.setAtIndex(JAVA_INT, nae, nv);") < fp.index("SUBMIT_PACKED_SPARSE_ASYNC.invokeExact")
    hb = workloads.param_collections()["batches"][0].subset(0, 3000)
    n, S = hb.n, hb.arg_tag.shape[0]
    arg_event, arg_off, tags, elem_off, etags = [], [0], [], [0], []
    for i in range(n):                                   # the loop of flushPacked
        na = min(int(hb.n_args[i]), S)
        if na == 0:
            continue
        arg_event.append(i)
        for s in range(na):
            tags.append(int(hb.arg_tag[s, i]))
            if hb.arg_tag[s, i] == abi.TAG_COLLECTION:
                k = s * n + i
                etags += hb.elem_tag[int(hb.elem_off[k]):int(hb.elem_off[k + 1])].tolist()
            elem_off.append(len(etags))
        arg_off.append(len(tags))
    pb = abi.PackedBatch(hb)
    assert np.array_equal(pb.arg_event, arg_event) and np.array_equal(pb.arg_off, arg_off)
    assert np.array_equal(pb.arg_tag, tags) and np.array_equal(pb.elem_off, elem_off)
    assert np.array_equal(pb.elem_tag, etags)
