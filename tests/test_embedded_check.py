"""The engine's host-compiled embedded token server path (sf_token.h
emb_request, sf_xflow.h xg_event) against the model's case files, under ASan +
UBSan in a stand-alone program (tests/embedded_check.cpp).  The cases are the
mixed traces of tests/embedded_cases.py, whose reachability is asserted on the
model first.  CPU only."""
import os
import subprocess

import pytest

from tests import embedded_cases as ec

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (7, 11)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("embedded") / "embedded_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-value",
                           "-Wno-unused-result", "-o", out, os.path.join(HERE, "embedded_check.cpp")])
    return out


@pytest.mark.parametrize("seed,sample_count", [(s, 2) for s in SEEDS] + [(7, 4)])
def test_embedded_check(so, exe, tmp_path, seed, sample_count):
    """sample_count 4 replays the walk's other instance (NodeWin<16>)."""
    case = ec.random_case(seed)
    config, tabs = ec.cfg(sample_count=sample_count), ec.tables()
    m, outs, _ = ec.run_model(case, tabs, config, with_tail=False)
    ec.reach(m, outs)
    path = tmp_path / "case.txt"
    path.write_text(ec.case_text(config, tabs, case, m, outs))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    n = sum(b.n for b in case["batches"])
    assert r.returncode == 0 and r.stdout.strip() == f"ok {n} {ec.R} 10", r.stdout[-3000:] + r.stderr[-4000:]


def test_unbound_case_is_todays_behaviour(so, exe, tmp_path):
    """No bind: every cluster rule falls back at once and no token state is touched."""
    case = ec.random_case(5, n_entries=900, batches=1, duration_ms=1500)
    config = ec.cfg()
    rules, _, namespaces, crules = ec.tables()
    tabs = (rules, [], namespaces, crules)
    m, outs, _ = ec.run_model(case, tabs, config, with_tail=False)
    assert m.requests == 0
    path = tmp_path / "case.txt"
    path.write_text(ec.case_text(config, tabs, case, m, outs))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-3000:] + r.stderr[-4000:]


def test_cluster_bind_layout(tmp_path):
    """sf_cluster_bind as the Python and Java bindings lay it out equals the C header's."""
    import ctypes as C
    import re

    from sentinel_amd import abi
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sentinel_flow.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(sf_cluster_bind), '
                   'offsetof(sf_cluster_bind, rule_index), offsetof(sf_cluster_bind, flow_id)); return 0; }\n')
    exe = str(tmp_path / "lay")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(os.path.dirname(HERE), "include"), "-o", exe, str(src)])
    size, o_rule, o_flow = map(int, subprocess.check_output([exe]).split())
    assert (C.sizeof(abi.sf_cluster_bind), abi.sf_cluster_bind.rule_index.offset, abi.sf_cluster_bind.flow_id.offset) == \
        (size, o_rule, o_flow)
    java = open(os.path.join(os.path.dirname(HERE), "java", "src", "main", "java", "com", "alibaba", "csp", "sentinel", "gpu",
                             "GpuEngine.java")).read()
    m = re.search(r"CLUSTER_BIND_BYTES = (\d+), CLUSTER_BIND_RULE_INDEX = (\d+), CLUSTER_BIND_FLOW_ID = (\d+);", java)
    assert m and tuple(map(int, m.groups())) == (size, o_rule, o_flow)
    assert 'fn("sf_load_cluster_binds"' in open(os.path.join(os.path.dirname(HERE), "java", "src", "main", "java", "com", "alibaba",
                                                             "csp", "sentinel", "gpu", "SentinelFlowNative.java")).read()
