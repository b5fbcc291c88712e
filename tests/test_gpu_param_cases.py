"""GPU parity on the borders of ParamFlow: the workloads of
tests/param_cases.py --

  a_bucket, a_invalid_counts, a_wmul   the token bucket: refill due or not at
                passTime == durationInSec * 1000 and one more, the integer
                steps of toAdd, newQps 0 and -1, acquireCount at maxCount,
                255 / 256 (the packed word's count escape), the (long) cast of
                count, hot items, a long multiply that wraps
  b_throttle    cost at a rounding half and at 0, the queue compare on and
                under maxQueueingTimeMs, two throttles whose waits add, a
                throttle's wait kept by the entry a later rule blocks
  c_identity    values that differ in one half of the bits or in the tag,
                null values, n_args <= paramIdx, neighbouring resources
  d_groups      SM_PARAM segments of 33 .. 129 events at 0, 1, 63 mod 64, two
                in one passbits word, 64 distinct values, 64 copies, caller-
                blocked and null entries, three rules on the index
  no_arg_slots, handover, growth, growth_async, table_wrap, inert

-- each family in the four routing contexts (lane, wave, generic, xflow), every
verdict, wait, rule index, node row and ENTRY_NODE exact against the oracle
(workloads.run), the thread count of every touched value after every batch,
and the routing from FlowEngine.heavy_profile() after every batch: the wave
context's segments SM_PARAM at their lengths, the generic ones SM_GENERIC, the
lane ones absent.  That each input sits on its border is proved on the CPU
(tests/test_param_cases.py).  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from sentinel_amd import abi
from tests import param_cases as pc
from tests import workloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


def recording(base, touched, profile):
    """``base`` (FlowEngine or OracleEngine) recording, after every submit, the
    thread count of every touched value and (engine) the heavy segments."""
    class Rec(base):
        def __init__(self, cfg):
            super().__init__(cfg)
            self.threads, self.profiles = [], []

        def submit(self, batch, *a):
            out = super().submit(batch, *a)
            self.threads.append([self.param_thread(r, 0, (t, b)) for r, t, b in touched])
            if profile:
                self.profiles.append({int(r): (int(n), int(m)) for r, n, m, _, _ in self.heavy_profile(cap=1 << 12)})
            return out
    return Rec


def run(eng_mod, so, w):
    eng, ora, outs = workloads.run(recording(eng_mod.FlowEngine, w["touched"], True),
                                   recording(so.OracleEngine, w["touched"], False), w)
    assert eng.threads == ora.threads, [(k, a, b) for k, (a, b) in enumerate(zip(eng.threads, ora.threads)) if a != b][:3]
    return eng, ora, outs


_built = {}


@pytest.mark.parametrize("ctx", pc.CONTEXTS)
@pytest.mark.parametrize("name", list(pc.CASES))
def test_case(eng_mod, so, name, ctx):
    if name not in _built:
        _built[name] = pc.CASES[name][0]()
    w = pc.emit(_built[name], ctx)
    eng, ora, _ = run(eng_mod, so, w)
    try:
        for k in range(w["main"]):
            prof = eng.profiles[k]
            if ctx == "xflow":
                continue                                   # (group segments are not heavy segments)
            assert prof == w["modes"][k], (k, sorted(set(prof.items()) ^ set(w["modes"][k].items()))[:8])
        assert any(t for row in eng.threads for t in row) or not w["touched"]
    finally:
        eng.close()
        ora.close()


def test_no_arg_slots(eng_mod, so):
    w = pc.no_arg_slots()
    eng, ora, outs = run(eng_mod, so, w)
    try:
        assert eng.profiles[0] == w["modes"] and (outs[0][0].status == abi.V_PASS).all()
    finally:
        eng.close()
        ora.close()


def test_handover(eng_mod, so):
    """lane -> wave -> generic (exit) -> generic (collection) -> wave on one
    resource's values: each walk reads the slots and thread counts the one
    before wrote."""
    w = pc.handover()
    eng, ora, _ = run(eng_mod, so, w)
    try:
        for k, mode in enumerate(pc.HAND_MODES):
            want = {0: (w["batches"][k].n, mode)} if mode else {}
            assert eng.profiles[k] == want, (k, eng.profiles[k])
        th = np.array(eng.threads)
        assert (th[1] > th[0]).all(), th                # (equal to the oracle's after every batch: run)
    finally:
        eng.close()
        ora.close()


def test_growth(eng_mod, so):
    w = pc.growth()
    eng, ora, _ = run(eng_mod, so, w)
    try:
        assert all(p == w["modes"] for p in eng.profiles), eng.profiles
        assert eng.stats().param_table_grows >= 3, eng.stats().param_table_grows
    finally:
        eng.close()
        ora.close()


def test_growth_async(eng_mod, so):
    """The same growth sequence as packed batches, two in flight: the
    pending-bound / idle-query branch of the table's reservation."""
    from tests import parity
    w = pc.growth()
    ora = so.OracleEngine(w["cfg"])
    ora.load_param_rules(list(w["param"]), list(w["items"]))
    want = [ora.submit(b) for b in w["batches"]]
    eng = eng_mod.FlowEngine(w["cfg"])
    pin = eng_mod.PinnedArrays(eng)
    try:
        eng.load_param_rules(list(w["param"]), list(w["items"]))
        pbs = [abi.PackedBatch(b, alloc=pin.array) for b in w["batches"]]
        outs = [pin.verdicts(b.n) for b in w["batches"]]
        eng.submit_packed_async(pbs[0], outs[0])
        for k in range(len(pbs)):
            if k + 1 < len(pbs):
                eng.submit_packed_async(pbs[k + 1], outs[k + 1])
            eng.sync_packed(outs[k])
            parity.compare_verdicts(outs[k], want[k], f"batch {k} (in flight)")
        eng.sync()
        assert eng.stats().param_table_grows >= 3, eng.stats().param_table_grows
        parity.compare_nodes(eng, ora, [0])
        for r, t, b in w["touched"]:
            assert eng.param_thread(r, 0, (t, b)) == ora.param_thread(r, 0, (t, b))
    finally:
        pin.free()
        eng.close()
        ora.close()


def test_table_wrap(eng_mod, so):
    w = pc.table_wrap()
    eng, ora, _ = run(eng_mod, so, w)
    try:
        assert all(p == w["modes"] for p in eng.profiles), eng.profiles
        ts = eng.param_table_stats()
        assert ts["capacity"] == pc.WRAP_CAP and ts["used"] == w["used"] and ts["max_probe"] >= w["min_probe"], ts
    finally:
        eng.close()
        ora.close()


def test_inert(eng_mod, so):
    w = pc.inert()
    eng, ora, _ = run(eng_mod, so, w)
    eng.close()
    ora.close()
