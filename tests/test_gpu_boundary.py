"""GPU parity on the internal borders of the hot path: the workloads of
tests/boundary_cases.py, each built to sit on a tile, ring, search or routing
border that random traffic reaches only by chance --

  far_runs      THREAD run mode: exits RUN_RC - 1 runs ahead and more (run_pre
                in HBM, the agent-scope fence before the next table step), in
                one batch and carried over a batch cut (k_thr_rec)
  lx_ring       THREAD window walk: exits on both sides of thr_mark_exit's
                split between the LDS ring and the HBM bitmap
  search_*      team_first_true's 64-ary steps: window ends and first failing
                entries at 0, 1, 63..65, 127..129, 4095..4097 (QPS, WarmUp,
                acquireCount 1-3 for team_next's tail)
  rl_chunks     RateLimiter segments ending on the HS_CH chunk edges
  batch_sizes   batches of 1 .. 12,289 events around the 16 / 64 / 2048 / 4096
                edges of the sort phase, with one, two and three radix passes
  placement     light and heavy segments of every mode starting, ending and
                straddling one under, on and one over the 64 / 2048 / 4096 /
                8192 tile edges, without and with origins
  routing       segment lengths on SHORT_MAX, the length classes, heavy_min
                and the 32-event SM_PARAM rule, for eight rule kinds
  zero_counts   rules of count 0 on every controller (a WarmUp rule's NaN
                threshold), on the heavy and on the light paths
  acc_overflow, many_windows   k_classify's two fallbacks to SM_GENERIC

Every verdict, wait, rule index, all node rows, rule states and ENTRY_NODE are
exact against the oracle (workloads.run).  That each input reaches its border
is proved on the CPU by the guards in tests/test_boundary_cases.py; here the
routing is checked as well, from FlowEngine.heavy_profile().  Run with -m gpu
on an MI355X."""
import numpy as np
import pytest

from tests import boundary_cases as bc
from tests import workloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


def seg_lengths(w):
    b = w["batches"][-1]
    return np.bincount(b.res_id, minlength=w["cfg"].max_resources)


def check_routing(name, w, eng):
    """The heavy segments of the last batch, as k_classify routed them."""
    prof = bc.profile_modes(eng)
    lens = seg_lengths(w)
    for r, (n, _) in prof.items():
        assert n == lens[r], (r, n, lens[r])
    if name.startswith(("far_runs", "lx_ring")):
        assert prof == {0: (int(lens[0]), bc.SM_THREAD)}, prof
    elif name.startswith(("search_", "rl_chunks", "routing", "zero_counts")):
        want = {r: (int(lens[r]), m) for r, m in w["modes"].items()}
        assert prof == want, sorted(set(prof.items()) ^ set(want.items()))[:8]
    elif name.startswith("placement"):
        want = {r: (int(lens[r]), m) for r, m in w["modes"].items()}
        got = {r: v for r, v in prof.items() if w["segs"][r][1] != "first"}
        assert got == want, sorted(set(got.items()) ^ set(want.items()))[:8]
    elif name == "many_windows":
        assert prof == {0: (int(lens[0]), bc.SM_GENERIC)}, prof
    elif name == "acc_overflow":
        assert len(prof) == w["cfg"].max_resources
        native = {0: bc.SM_NORULE, 1: bc.SM_QPS, 2: bc.SM_WARM, 3: bc.SM_RL}
        fell = [r for r, (_, m) in prof.items() if m == bc.SM_GENERIC]
        assert fell and len(fell) < len(prof), len(fell)
        assert all(m == native[r % 4] for r, (_, m) in prof.items() if r not in fell)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_border(eng_mod, so, name):
    w = bc.CASES[name][0]()
    eng, ora, _ = workloads.run(eng_mod.FlowEngine, so.OracleEngine, w)
    try:
        check_routing(name, w, eng)
    finally:
        eng.close()
        ora.close()
