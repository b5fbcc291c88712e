"""The border scripts of tests/token_cases.py and tests/wire_cases.py on the
CPU: the constants they are built around against the source text (and that the
check notices an edited constant), and every guard, computed from the inputs
and the oracle's answers alone.  The GPU twin, which compares the engine with
the oracle on the same scripts, is tests/test_gpu_token_wire_cases.py."""
import os
import shutil

import pytest

from tests import token_cases as tc
from tests import wire_cases as wc


def test_token_constants_match_the_source():
    """A retune of the limiter ring, the search fan-out or the table minimum moves the borders:
    move the cases with it."""
    assert tc.source_constants() == tc.MIRROR
    assert tc.search_nw(4097) == [1, 2, 63, 64, 65, 66, 4032, 4095, 4096, 4097]
    assert tc.search_nw(262145) == [1, 4097, 262144, 262145]
    assert tc.fit(3, 1000) == 3 and tc.fit(3, 999) == 2 and tc.fit(200, 16) == 4 and tc.fit(3, 16000) == 33


def test_wire_constants_match_the_source():
    assert wc.source_constants() == wc.MIRROR
    assert 2 ** wc.WIRE_ROUNDS >= wc.WIRE_TILE // 2 > 2 ** (wc.WIRE_ROUNDS - 1)      # 13 doublings, 8192 frames


@pytest.mark.parametrize("name,old,new", [
    ("sf_token.h", "LIM_WL = 100", "LIM_WL = 200"),
    ("sf_token.h", "constexpr int CL_MAXS = 16;", "constexpr int CL_MAXS = 32;"),
    ("sf_token.hip", "constexpr int TD_T = 64;", "constexpr int TD_T = 128;"),
    ("sf_token.hip", "NS_NONE = 0xff", "NS_NONE = 0xfe"),
    ("sf_token.hip", "while (e - a > 64)", "while (e - a > 32)"),
    ("sf_token.hip", "(e - a + 63) / 64", "(e - a + 31) / 32"),
    ("sf_decide.h", "PT_MAX_PROBE = 4096", "PT_MAX_PROBE = 1024"),
    ("sf_host_cluster.cpp", "uint64_t pc = 1024;", "uint64_t pc = 4096;"),
    ("sf_host_cluster.cpp", "if (n > 255) return fail", "if (n > 254) return fail"),
])
def test_token_drift_is_noticed(tmp_path, name, old, new):
    """The same check on a copy of the sources with one constant edited."""
    for f in ("sf_token.h", "sf_token.hip", "sf_decide.h", "sf_host_cluster.cpp"):
        shutil.copy(os.path.join(tc._CSRC, f), tmp_path / f)
    src = (tmp_path / name).read_text()
    assert src.count(old) == 1, (name, old)
    (tmp_path / name).write_text(src.replace(old, new))
    try:
        same = tc.source_constants(str(tmp_path)) == tc.MIRROR
    except AssertionError:
        same = False
    assert not same


@pytest.mark.parametrize("name,old,new", [
    (("sentinel_amd", "csrc", "sf_wire.h"), "WIRE_TILE = 16384", "WIRE_TILE = 8192"),
    (("sentinel_amd", "csrc", "sf_wire.hip"), "r < 13; r++", "r < 12; r++"),
    (("include", "sentinel_flow.h"), "SF_WIRE_MAX_FRAME 1024", "SF_WIRE_MAX_FRAME 2048"),
])
def test_wire_drift_is_noticed(tmp_path, name, old, new):
    for f in (("sentinel_amd", "csrc", "sf_wire.h"), ("sentinel_amd", "csrc", "sf_wire.hip"),
              ("include", "sentinel_flow.h")):
        os.makedirs(tmp_path.joinpath(*f[:-1]), exist_ok=True)
        shutil.copy(os.path.join(wc._ROOT, *f), tmp_path.joinpath(*f))
    p = tmp_path.joinpath(*name)
    src = p.read_text()
    assert src.count(old) == 1, (name, old)
    p.write_text(src.replace(old, new))
    try:
        same = wc.source_constants(str(tmp_path)) == wc.MIRROR
    except AssertionError:
        same = False
    assert not same


@pytest.mark.parametrize("name", list(tc.CASES))
def test_token_case_guard(so, name):
    sc = tc.CASES[name]()
    tc.check_times(sc)
    ora = so.OracleEngine(sc.config())
    try:
        R = tc.play(ora, sc)
    finally:
        ora.close()
    print(name, sc.guard(R))


def test_token_table_overflow_script():
    """The overflow script asks for one value more than the smallest table has slots."""
    sc = tc.param_table_overflow()
    a, b = sc.calls()
    assert sc.cfg["param_capacity"] == 1 and a.n == tc.CP_MIN_SLOTS and b.n == 1
    assert len(set(a.param_bits.tolist()) | set(b.param_bits.tolist())) == tc.CP_MIN_SLOTS + 1


@pytest.mark.parametrize("name", list(wc.CASES))
def test_wire_case_guard(so, name):
    case = wc.CASES[name]()
    ora = so.OracleEngine(tc.Script("wire").config())
    try:
        R = wc.play(ora, case)
    finally:
        ora.close()
    print(name, wc.guard(case, R))
