"""The ParamFlow border workloads of tests/param_cases.py on the CPU: every
guard (computed from the batch and the oracle's verdicts and state), the
drift check of the hash and key-packing lines the table cases restate, and
the host build of the interpreter against the oracle in the lane, generic and
xflow contexts (verdicts, waits, rule indices, node rows).  The GPU twin is
tests/test_gpu_param_cases.py.

The host build demotes SM_PARAM segments to the lane walk, so the wave context
runs decide_segment here too; param_run_rule itself, which only the wavefront
walk calls, is checked against param_pass_single by the stand-alone
tests/param_run_check.cpp, plain and under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from sentinel_amd import abi
from tests import param_cases as pc
from tests import workloads

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hs():
    from tests.hostsim import hostsim
    hostsim.lib()
    return hostsim


_built = {}


def case_of(name):
    if name not in _built:
        _built[name] = pc.CASES[name][0]()
    return _built[name]


def run_host(hs, so, w):
    if w.get("host_capacity"):                      # (the host build's table does not grow)
        w = dict(w, cfg=abi.sf_config.from_buffer_copy(w["cfg"]))
        w["cfg"].param_capacity = w["host_capacity"]
    eng = ora = None
    try:
        eng, ora, _ = workloads.run(hs.HostSimEngine, so.OracleEngine, w)
    finally:
        for x in (eng, ora):
            if x is not None:
                x.close()


@pytest.mark.parametrize("name", list(pc.CASES))
def test_guards(so, name):
    """The case sits on its borders: the oracle gives every pinned occurrence
    its designed verdict, the family's own guard holds, and the tail entries
    show the tokens read_param reported."""
    case = case_of(name)
    w = pc.emit(case, "wave")
    ora, st, wait, _ = pc.oracle_run(so, w)
    ora.close()
    pinned = pc.guard_expect(case, st, wait)
    assert pinned >= 2, pinned
    info = pc.CASES[name][1](so, case, st, wait)
    tails = pc.guard_tail(so, case, w)
    if name in ("a_bucket", "c_identity"):
        assert tails >= 2, tails
    print(name, dict(events=len(case["rows"]), pinned=pinned, tails=tails, **info))


@pytest.mark.parametrize("ctx", pc.CONTEXTS)
@pytest.mark.parametrize("name", list(pc.CASES))
def test_case_host_build(hs, so, name, ctx):
    w = pc.emit(case_of(name), ctx)
    lens = [np.bincount(b.res_id).max() for b in w["batches"][:w["main"]]]
    if ctx == "lane":
        assert max(lens) <= pc.PARAM_MIN and w["main"] > 1
    else:
        assert min(lens) > pc.PARAM_MIN and all(w["modes"]) == (ctx in ("wave", "generic"))
    for b in w["batches"]:
        assert np.all(np.diff(b.ts_ms) >= 0)
    run_host(hs, so, w)


@pytest.mark.parametrize("name", list(pc.SINGLE))
def test_single_guard_and_host_build(hs, so, name):
    make, guard = pc.SINGLE[name]
    w = make()
    print(name, guard(so, w))
    run_host(hs, so, w)


@pytest.mark.parametrize("name", list(pc.SYSTEM))
def test_system_guard(so, name):
    make, guard = pc.SYSTEM[name]
    print(name, guard(so, make()))


@pytest.fixture(scope="module")
def run_check(tmp_path_factory):
    """tests/param_run_check.cpp, plain and under ASan + UBSan."""
    d = tmp_path_factory.mktemp("param_run")
    exes = {}
    for kind, flags in (("plain", ["-O2"]),
                        ("sanitized", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exes[kind] = str(d / f"param_run_check_{kind}")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-g", "-std=c++17", "-ffp-contract=off",
                               "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wall", "-Wno-unknown-pragmas",
                               "-Wno-unused-result", "-Wno-unused-value", "-Wno-unused-function", *flags, "-o", exes[kind],
                               os.path.join(HERE, "param_run_check.cpp")])
    return exes


@pytest.mark.parametrize("kind", ["plain", "sanitized"])
def test_param_run_rule_equals_pass_single(run_check, kind):
    r = subprocess.run([run_check[kind]], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout


def test_hash_and_key_lines_match_the_source(run_check):
    """A retune of the table's hash, key packing or probing moves the wrap
    case off the table's end: the restated lines are read back from the source
    text, and the restated functions are compared with the compiled ones."""
    assert pc.source_lines() == dict(PK_RULE=pc.PK_RULE, PARAM_MIN=pc.PARAM_MIN)
    hi = pc.pkey_hi(0, pc.PK_RULE, 0, pc.L)
    vals = pc.wrap_values()
    for lo in (0, 1, int(vals[0]), int(vals[-1]), 2 ** 64 - 1):
        out = subprocess.run([run_check["plain"], "hash", str(hi), str(lo)], capture_output=True, text=True, check=True)
        h, k = (int(x) for x in out.stdout.split())
        assert k == hi and h == int(pc.table_hash(hi, np.array([lo], np.uint64))[0]), (lo, h, k)
    home = pc.table_hash(hi, vals) & np.uint64(pc.WRAP_CAP - 1)
    assert vals.size == pc.WRAP_VALUES and (home >= pc.WRAP_CAP - pc.WRAP_LAST).all()
