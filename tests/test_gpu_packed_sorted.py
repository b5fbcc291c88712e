"""GPU parity on batches that need the escapes of the packed sorted-event word
(sf_decide.h): a time 65,535 ms or more after the batch's first event and an
acquireCount outside 1..255 are read from the caller's batch through the sort
permutation.  No other workload of the suite has a batch longer than 65 s.

Every verdict, wait, rule index, all node digests, rule states and ENTRY_NODE
are exact against the oracle (workloads.run).  Each case runs with
heavy_min_events 0 (the engine's default of 512) and 64, so the light, short,
lean-QPS, heavy-decide, heavy-stream (window walk and RateLimiter) and fill
paths all see escaped events.  The workloads (tests/packed_sorted_cases.py) are
checked on the CPU by tests/test_packed_sorted.py.  The counts case includes
acquireCount -1: the oracle accepts it for these rules.  Run with -m gpu on an
MI355X."""
import pytest

from tests import packed_sorted_cases as cases
from tests import workloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


@pytest.mark.parametrize("heavy_min", [0, 64])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_escaped_events(eng_mod, so, name, heavy_min):
    w = cases.CASES[name]()
    w["cfg"].heavy_min_events = heavy_min
    workloads.run(eng_mod.FlowEngine, so.OracleEngine, w)
