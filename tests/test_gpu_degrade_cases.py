"""GPU parity on the internal borders of the DegradeSlot kernels: the
workloads of tests/degrade_cases.py through sf_degrade_submit and those of
tests/degrade_chain_cases.py through sf_submit, each built to sit on a lane,
chunk, window or routing border of k_dg_walk / k_dg_wave that random traffic
reaches only by chance --

  seg_lengths        1 .. 257 walked events around the 64|65 lane/wave switch
                     and the two prefetch conditions; pre-blocked events that
                     shorten a segment to 64; 4 and 5 breakers; twins that
                     compare the wave walk with the lane walk directly
  first_change_lane  the one state change of a three-chunk segment at lane 0,
                     1, 62, 63 of the first, middle and tail chunk, for each
                     kind of change (trip, probe, close, re-open)
  window_rolls       stat_interval_ms boundaries between lanes 0|1, 31|32,
                     62|63 and on the chunk edge, three windows in a chunk,
                     counts carried from the previous chunk / batch into a trip
                     and not carried into a later run, a window only an entry
                     or an ignored exit enters, intervals 200 and 1000
  thresholds         counts and ratios on, one under and one over the rule's
                     threshold, Math.round edges, NaN rules dropped: verdicts
                     derived by hand, on the lane and on the wave walk
  retry_and_probe    entries at next_retry - 1 and at next_retry (lanes 0, 17,
                     63), the probe's exit in the same chunk, the next, two
                     later and the next batch, probes sent back by a later
                     breaker (2, 4 and 64 breakers)
  ignored_exits      exits of refused and of passed entries found through this
                     chunk's mask (before and after the cut), the previous
                     chunk's (bits 0 and 63), a status load (two and ten chunks
                     back), create_ts, entry_ref -2, no entry_ref array at all
  batch_cuts         a cut while OPEN, HALF_OPEN and mid-window, wave walk then
                     lane walk and the reverse (state between HBM and registers)
  many_segments      2048 + 3 wave segments (k_dg_wave's grid stride), about
                     140 K events; key_widths_*: 1, 2, 255, 256 breaker resources
  chain_*            sf_submit: breakers on resources that would route to a
                     window algorithm (all SM_GENERIC), entries that FlowSlot /
                     ParamFlowSlot refuse or hold (PriorityWaitException) in
                     front of an OPEN breaker, breakers under RELATE / CHAIN /
                     origin rules
  recovery           recoveryTimeoutMs in Java int arithmetic, literal

Everything is exact against the oracle.  That each input reaches its border is
proved on the CPU by the guards in tests/test_degrade_cases.py.  Run with
-m gpu on an MI355X."""
import numpy as np
import pytest

from oracle import degrade as od
from sentinel_amd import abi
from tests import boundary_cases as bc
from tests import degrade_cases as dc
from tests import degrade_chain_cases as cc

pytestmark = pytest.mark.gpu

SF_ERR_INVALID, SF_ERR_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


def _engine(eng_mod, R, max_batch):
    return eng_mod.FlowEngine(abi.default_config(max_resources=R, max_batch=max_batch))


def submit_and_compare(e, c, an):
    """As check_gpu of tests/test_degrade.py; returns the engine's verdicts."""
    assert e.load_degrade_rules(c["rules"]) == len(an["states"])
    got = []
    for bi, (b, st, ri) in enumerate(zip(c["batches"], an["status"], an["rule_idx"])):
        v = e.degrade_submit(b)
        got.append(v)
        bad = np.nonzero(v.status != st)[0]
        assert bad.size == 0, f"batch {bi}: {bad.size} verdicts differ, first at {bad[:5]}"
        blk = st == od.V_BLOCK_DEGRADE
        assert np.array_equal(v.rule_idx[blk], ri[blk]), f"batch {bi}: breaker index"
        assert np.all(v.wait_ms == 0)
    for k, want in enumerate(an["states"]):
        assert e.read_breaker(k) == want, f"breaker {k}"
    return got


@pytest.mark.parametrize("name", list(dc.CASES))
def test_degrade_border(eng_mod, name):
    c = dc.CASES[name][0]()
    an = dc.analyze(c)
    e = _engine(eng_mod, c["R"], max(b.n for b in c["batches"]))
    try:
        got = submit_and_compare(e, c, an)
        for a, b, nb in c.get("twins", ()):                    # the wave walk against the lane walk
            full = c["full"]
            assert np.array_equal(got[0].status[full.res_id == a], got[0].status[full.res_id == b])
            ka, kb = an["by_res"][a], an["by_res"][b]
            for j in range(nb):
                assert e.read_breaker(ka[j]) == e.read_breaker(kb[j]), (a, b, j)
        if name == "thresholds":
            assert dc.threshold_verdicts(c, got[0].status, got[0].rule_idx) == dc.threshold_expect()
    finally:
        e.close()


def test_recovery_time_degrade_submit(eng_mod):
    c = dc.recovery()
    e = _engine(eng_mod, c["R"], c["full"].n)
    try:
        assert e.load_degrade_rules(c["rules"]) == len(dc.RECOVERY_MS)
        v = e.degrade_submit(c["batches"][0])
        got = dc.recovery_observed(c, v.status, lambda k: e.read_breaker(k)["next_retry_ms"])
    finally:
        e.close()
    assert got == dc.recovery_expect()


def test_recovery_time_submit(eng_mod):
    c = dc.recovery()
    e = _engine(eng_mod, c["R"], c["full"].n)
    try:
        assert e.load_degrade_rules(c["rules"]) == len(dc.RECOVERY_MS)
        v = e.submit(c["batches"][0])
        got = dc.recovery_observed(c, v.status, lambda k: e.read_breaker(k)["next_retry_ms"])
    finally:
        e.close()
    assert got == dc.recovery_expect()


def test_sixty_five_breakers_are_refused(eng_mod):
    """65 valid rules on one resource: SF_ERR_UNSUPPORTED, and the rules loaded before stay in force."""
    rules = [dc.rule(0, dc.COUNT, 0, tw=50)] + [dc.rule(0, dc.COUNT, float(k)) for k in range(1, dc.MAX_BREAKERS + 1)]
    b = abi.HostBatch(np.zeros(3, np.uint32), dc.T0 + np.arange(3), np.ones(3, np.int32),
                      np.array([0, abi.EV_EXIT | abi.EV_ERROR, 0], np.uint8), entry_ref=np.array([-1, 0, -1]))
    e = _engine(eng_mod, 2, 16)
    try:
        assert e.load_degrade_rules(rules[:dc.MAX_BREAKERS]) == dc.MAX_BREAKERS
        with pytest.raises(eng_mod.EngineError) as ei:
            e.load_degrade_rules(rules)
        assert ei.value.code == SF_ERR_UNSUPPORTED
        v = e.degrade_submit(b)
        assert list(v.status) == [od.V_PASS, od.V_EXIT, od.V_BLOCK_DEGRADE] and v.rule_idx[2] == 0
        assert e.read_breaker(dc.MAX_BREAKERS - 1)["total_count"] == 1
    finally:
        e.close()


@pytest.mark.parametrize("n,walk", [(100, "wave"), (60, "lane")])
@pytest.mark.parametrize("bad", ["an_exit", "another_resource", "a_later_event"])
def test_bad_refs_and_clock(eng_mod, bad, n, walk):
    """An exit whose entry_ref names an exit, another resource's entry or a
    later event, on a wave-walk segment (k_dg_gather's check) and on a
    lane-walk one: SF_ERR_INVALID, and the engine clock stays where it was (a
    batch earlier than the refused one is still taken)."""
    res = np.zeros(n, np.uint32)
    res[n - 30] = 1                                            # one entry of the other resource
    fl = np.zeros(n, np.uint8)
    fl[n - 20:] = abi.EV_EXIT
    ref = np.full(n, -1, np.int64)
    ref[n - 20:] = np.arange(20)
    ref[n - 10] = {"an_exit": n - 15, "another_resource": n - 30, "a_later_event": n - 5}[bad]
    ts = dc.T0 + 1000 + np.arange(n, dtype=np.int64)
    rules = [dc.rule(0, dc.COUNT, 1), dc.rule(1, dc.COUNT, 1)]
    assert dc.paths(rules, abi.HostBatch(res, ts, np.ones(n, np.int32), fl, entry_ref=ref))[0]["walk"] == walk
    e = _engine(eng_mod, 2, 256)
    try:
        e.load_degrade_rules(rules)
        with pytest.raises(eng_mod.EngineError) as ei:
            e.degrade_submit(abi.HostBatch(res, ts, np.ones(n, np.int32), fl, entry_ref=ref))
        assert ei.value.code == SF_ERR_INVALID
        ref[n - 10] = 10
        v = e.degrade_submit(abi.HostBatch(res, ts - 1000, np.ones(n, np.int32), fl, entry_ref=ref))
        assert np.all(v.status[:n - 20] == od.V_PASS) and np.all(v.status[n - 20:] == od.V_EXIT)
    finally:
        e.close()


@pytest.mark.parametrize("name", list(cc.CASES))
def test_chain_border(eng_mod, so, name):
    w = cc.CASES[name][0]()
    eng = ora = None
    try:
        eng, ora = cc.run(eng_mod.FlowEngine, so.OracleEngine, w)
        if "modes" in w:                                       # every heavy breaker segment is SM_GENERIC
            lens = np.bincount(w["full"].res_id, minlength=w["cfg"].max_resources)
            want = {r: (int(lens[r]), m) for r, m in w["modes"].items()}
            assert bc.profile_modes(eng) == want
    finally:
        for x in (eng, ora):
            if x is not None:
                x.close()
