"""GPU parity on the borders of the token server and its wire framing: the
scripts of tests/token_cases.py and tests/wire_cases.py, each built to sit on
a search, ring, table or tile border that random traffic reaches only by
chance --

  ns_search         k_ns_limit's 64-ary window search: R requests of one
                    namespace, the window end on every step edge, one, two and
                    three levels deep
  ns_first_fail     the first failing request with a carried-in sum, fractional
                    and zero max_qps, 0 .. 129 requests in the strided scatter
  ns_table_*        limited, unlimited and unknown namespaces interleaved; 255
                    namespaces (index 254 beside NS_NONE); none at all
  metric_ring       bursts on every window and interval edge of ClusterMetric
                    for sample_count 1 .. 16 and 1-ms to 1-s windows, as one
                    call and as one call per burst
  occupy_*, exceed  tryOccupyNext (head bucket, transfer on a bucket restart
                    but not on a new bucket), max_occupy_ratio, exceed_count
  numeric           rule counts 0, negative, fractional, 1e12, inf, NaN;
                    acquireCount 2^31 - 1; flow ids up to 2^63 - 1
  param_columns_*   the same ring on one value; every tag, null, hot items
  param_table       a full value table; 4096 lanes claiming one slot
  param_serial      a rule alternating between the serial and the per-value
                    route over the same columns
  degenerate_*      calls of one request, calls that reach no checker, one
                    segment per request around 64, reloads
  wire cases        a tile of 8192 empty frames, frames / connections /
                    too-long frames on offsets 16383 and 0, 63 .. 130
                    connection starts in a tile, sizes of one and two tiles
                    +- 1, a HOST stop on a tile edge and the call after it

Every request's status, remaining and wait_ms (wire: counts, stop, consumed,
resp_off and the response bytes) and cluster_sum of every flow rule after every
call are exact against the oracle.  That each script reaches its border, and
that its probes separate a wrong hidden state from the right one, is proved on
the CPU by the guards in tests/test_token_wire_cases.py.  Run with -m gpu on
an MI355X."""
import pytest

from sentinel_amd import abi
from tests import token_cases as tc
from tests import wire_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


@pytest.mark.parametrize("name", list(tc.CASES))
def test_token_border(eng_mod, so, name):
    sc = tc.CASES[name]()
    eng, ora = eng_mod.FlowEngine(sc.config()), so.OracleEngine(sc.config())
    try:
        tc.compare(sc, tc.play(eng, sc), tc.play(ora, sc))
    finally:
        eng.close()
        ora.close()


def test_token_table_overflow(eng_mod):
    """A value more than the table has slots: SF_ERR_CAPACITY, not a wrong decision."""
    sc = tc.param_table_overflow()
    eng = eng_mod.FlowEngine(sc.config())
    try:
        eng.load_namespaces(sc.steps[0][1])
        eng.load_cluster_rules(*sc.steps[1][1:])
        first, second = sc.calls()
        assert (eng.request_tokens(first).status == tc.OK).all()
        with pytest.raises(eng_mod.EngineError) as err:
            eng.request_tokens(second)
        assert err.value.code == abi.SF_ERR_CAPACITY
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(wc.CASES))
def test_wire_border(eng_mod, so, name):
    case = wc.CASES[name]()
    cfg = tc.Script("wire").config()
    eng, ora = eng_mod.FlowEngine(cfg), so.OracleEngine(cfg)
    try:
        wc.compare(case, wc.play(eng, case), wc.play(ora, case))
    finally:
        eng.close()
        ora.close()
