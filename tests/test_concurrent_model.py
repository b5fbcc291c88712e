"""Cluster concurrency tokens without a GPU: known answers of the reference's
own tests on the sequential model (tests/concurrent_model.py), the chunk
solver of the device walk run on the host wave against a plain serial loop
under ASan + UBSan, and the exports / layouts of the new C-ABI entries."""
import os
import re
import subprocess

import numpy as np

from sentinel_amd import abi
from tests import concurrent_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FUNCTIONS = ("sf_load_concurrent_config", "sf_concurrent_reserve", "sf_request_concurrent", "sf_concurrent_expire",
             "sf_concurrent_now", "sf_read_token", "sf_concurrent_get_stats")
STRUCTS = ("sf_concurrent_config", "sf_concurrent_batch", "sf_concurrent_results", "sf_token_node",
           "sf_concurrent_stats")


def known_answer_batches():
    """ConcurrentClusterFlowCheckerTest.java:61-84: rule 111, GLOBAL, count 10."""
    acquire = cm.make_batch([(cm.A, 111, 1, 0)] * 20, ts=1000)
    release = cm.make_batch([(cm.R, j, 0, 0) for j in range(10)], ts=1001)
    return acquire, release


def test_known_answer_acquire_block_release():
    m = cm.ConcurrentModel()
    m.load_rules([cm.Rule(111, 10.0)])
    rp = cm.Replay(m)
    acquire, release = known_answer_batches()
    st, _ = rp.run(acquire)
    assert st[:10].tolist() == [cm.OK] * 10 and st[10:].tolist() == [cm.BLOCKED] * 10
    ids = rp.model_ids[:10]
    assert all(ids) and len(set(ids)) == 10 and not any(rp.model_ids[10:])
    assert m.now_calls[111] == 10
    st, _ = rp.run(release)
    assert st.tolist() == [cm.RELEASE_OK] * 10
    assert m.now_calls[111] == 0 and not m.tokens


def test_expiry_shape_resource_timeout():
    """ConcurrentClusterFlowCheckerTest.java:115-124: 10 tokens, time-outs 500 /
    1000, the client online, a sweep 3 s later: all go by the resource rule."""
    m = cm.ConcurrentModel()
    m.load_rules([cm.Rule(111, 10.0)])
    m.load_config([(111, 500, 1000)])
    rp = cm.Replay(m)
    rp.run(cm.make_batch([(cm.A, 111, 1, 0)] * 10, ts=1000))
    assert len(m.tokens) == 10 and m.now_calls[111] == 10
    assert rp.expire(1000 + 400, online_clients=[0], n_clients=1) == 0       # 400 - 500 is not > 500
    assert rp.expire(1000 + 3000, online_clients=[0], n_clients=1) == 10
    assert not m.tokens and m.now_calls[111] == 0


def test_model_int_wrap_and_reload():
    m = cm.ConcurrentModel()
    m.load_rules([cm.Rule(1, 1e12), cm.Rule(2, 5.0)])
    assert m.acquire(1, 2 ** 31 - 1, 0, 0)[0] == cm.OK
    assert m.acquire(1, 1, 0, 0)[0] == cm.OK and m.now_calls[1] == -2 ** 31    # int + int wraps, then > double
    _, t2 = m.acquire(2, 3, 0, 0)
    m.load_rules([cm.Rule(1, 1e12)])
    assert m.now_calls == {1: -2 ** 31} and m.release(t2) == cm.NO_RULE_EXISTS and t2 in m.tokens
    m.load_rules([cm.Rule(1, 1e12), cm.Rule(2, 5.0)])
    assert m.now_calls[2] == 0 and m.release(t2) == cm.RELEASE_OK and m.now_calls[2] == -3


def test_chunk_solver_on_the_host_wave(tmp_path):
    """cc_solve_chunk (sf_concur.h) through its plain-loop wave against the
    one-by-one loop on 100,000 random chunks: lengths 1..64, counts 1..5 and
    near INT32_MAX, thresholds 0 .. above INT32_MAX, 0..60 % releases.  Every
    pass mask and final nowCalls agree, and all three outcomes occurred."""
    exe = tmp_path / "concur_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "hostsim", "concur_check.cpp")])
    r = subprocess.run([str(exe), "100000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(zip(r.stdout.split()[0::2], map(int, r.stdout.split()[1::2])))
    assert got["chunks"] == 100000
    assert got["all_pass"] > 0 and got["one_round_all_blocked"] > 0 and got["multi_round"] > 0
    assert got["all_pass"] + got["one_round_all_blocked"] + got["multi_round"] == 100000


def test_exports_and_layouts():
    from sentinel_amd import engine
    L = engine.lib()
    assert [f for f in FUNCTIONS if not hasattr(L, f)] == []
    hdr = open(os.path.join(ROOT, "include", "sentinel_flow.h")).read()
    for f in FUNCTIONS:
        assert re.search(r"^int\s+%s\(" % f, hdr, flags=re.M), f
    for s in STRUCTS:
        assert s in abi.STRUCT_SIZES
    assert abi.STRUCT_SIZES["sf_concurrent_config"] == 24 and abi.STRUCT_SIZES["sf_token_node"] == 32
    assert abi.STRUCT_SIZES["sf_concurrent_stats"] == 56
    assert abi.token_id_shard((3 << 56) | 5) == 2


def test_random_stream_covers_every_status():
    """The generator of the GPU coverage test: each of the four statuses makes
    up at least 5 % of the stream (the GPU test asserts the same)."""
    from tests.test_gpu_concurrent import coverage_case, model_of
    rules, batches = coverage_case()
    rp = cm.Replay(model_of(rules))
    for b in batches:
        rp.run(b)
    st = np.array(rp.status)
    for code in (cm.OK, cm.BLOCKED, cm.RELEASE_OK, cm.ALREADY_RELEASE):
        assert (st == code).mean() >= 0.05, code
