"""The packed sorted-event word on the CPU: the stand-alone encode / decode
check (tests/packed_word_check.cpp, built here with the host compiler), and
the validity of the workloads the GPU test relies on
(tests/packed_sorted_cases.py) with the oracle alone and on the host build of
the interpreter (its full-width fallback)."""
import os
import subprocess

import numpy as np
import pytest

from sentinel_amd import abi
from tests import packed_sorted_cases as cases
from tests import workloads

HERE = os.path.dirname(os.path.abspath(__file__))


def test_word_roundtrip(tmp_path):
    exe = str(tmp_path / "packed_word_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-value",
                           "-o", exe, os.path.join(HERE, "packed_word_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout, r.stdout


@pytest.fixture(scope="module")
def built():
    return {name: make() for name, make in cases.CASES.items()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_is_valid_and_escapes(so, built, name):
    """The oracle accepts every event of the workload (so_submit returns 0:
    OracleEngine.submit asserts it), and the workload does need the escape it
    is there for."""
    w = built[name]
    ora = so.OracleEngine(w["cfg"])
    if w.get("status") is not None:
        ora.set_system_status(*w["status"])
    if w.get("system"):
        ora.load_system_rules(list(w["system"]))
    if w.get("flow"):
        ora.load_flow_rules(list(w["flow"]))
    if w.get("param"):
        ora.load_param_rules(list(w["param"]), list(w.get("items", ())))
    outs = [ora.submit(b) for b in w["batches"]]
    assert len(w["batches"]) == 1
    b = w["batches"][0]
    assert np.all(np.diff(b.ts_ms) >= 0)
    if name in cases.FAR_CASES:
        far = (b.ts_ms - b.ts_ms[0]) >= cases.FAR_MS
        assert far.sum() > 100, far.sum()
        if b.entry_ref is not None:
            ex = np.nonzero(((b.flags & abi.EV_EXIT) != 0) & (b.entry_ref >= 0))[0]
            assert far[ex].any(), "no exit past the 16-bit offset"
    if name == "long_single":
        ex = np.nonzero(((b.flags & abi.EV_EXIT) != 0) & (b.entry_ref >= 0))[0]
        gap = b.ts_ms[ex] - b.ts_ms[b.entry_ref[ex]]
        assert (gap < 100).any() and (gap >= 0).all()
    if name == "boundary":
        seg = b.res_id[np.nonzero(far)[0]]
        assert np.intersect1d(seg, b.res_id[~far]).size > 10        # segments that cross the boundary
    if name == "counts":
        for c in cases.ODD_COUNTS:
            assert (b.count == c).sum() > 10, c
        st = outs[0].status
        assert ((st == abi.V_PASS) & (b.count > 255)).any() or ((st == abi.V_BLOCK_FLOW) & (b.count > 255)).any()
    if name == "system_views":
        assert (outs[0].status == abi.V_BLOCK_SYSTEM).sum() > 0, "the SystemRule never fired"


@pytest.fixture(scope="module")
def hs():
    from tests.hostsim import hostsim
    hostsim.lib()
    return hostsim


@pytest.mark.parametrize("heavy_min", [0, 64])
@pytest.mark.parametrize("name", ["long_single", "boundary", "counts", "xflow_long", "param_long"])
def test_case_on_host_build(hs, so, name, heavy_min):
    """The host build of the interpreter (full-width arrays, no words) on the
    same workloads: the accessors' fallback is exact against the oracle."""
    w = cases.CASES[name]()
    w["cfg"].heavy_min_events = heavy_min
    workloads.run(hs.HostSimEngine, so.OracleEngine, w)
