"""SystemRules with a thread, average-RT or load (BBR) check on a resource-sharded
node: the wide kinds of the per-window exchange (sentinel_amd/csrc/sf_sysx.h,
sf_submit_node).

CPU: the product's plan step (sxw_bin, sxw_range, sxw_reduce) on random node
streams under ASan + UBSan (tests/sysx_wide_check.cpp: soundness against
sys_classify on every entry's exact prefix, q, progress, rank order); the
protocol restated over oracle engines (tests/sysx_wide_sim.py) on two and three
ranks -- threads of this process and a gloo world of two processes -- equals
one replay of the whole node batch, every verdict and every rank's ENTRY_NODE
(SystemRuleManager.checkSystem, SystemRuleManager.java:291-348), on the thread,
RT, load and combined rules, the 1-bucket 1500-ms geometry and the borders of
the plan step (tests/sysx_wide_cases.py), each guarded so the test proves it
reaches its border.  GPU: engines deciding their shards through sf_submit_node
(threads, LocalComm) equal the same replay; messages stay within
SF_SYSX_WIDE_MSG_BYTES."""
import functools
import os
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

from sentinel_amd import abi, system_shard
from tests import sysx_wide_cases as cases
from tests import sysx_wide_sim as sim
from tests.test_system_exchange import _rank_cfg, _reference, _threads
from tests.test_system_shard import _load, _merge

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("thread", "rt", "load", "combined", "geom")


# ---------------------------------------------------------------- the plan step alone, under the sanitizers
def test_plan_step_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sysx_wide_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-Wall", "-Wno-unused-result", "-Wno-unused-value",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "sysx_wide_check.cpp")])
    r = subprocess.run([exe, "3000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("3000 trials, 0 failures"), r.stdout[-2000:]


def test_message_size_constant():
    with open(os.path.join(os.path.dirname(HERE), "include", "sentinel_flow.h")) as f:
        h = f.read()
    assert f"#define SF_SYSX_WIDE_MSG_BYTES {abi.SYSX_WIDE_MSG_BYTES}" in h
    assert f"#define SF_SYSX_MSG_BYTES {abi.SYSX_MSG_BYTES} " in h
    assert abi.SYSX_WIDE_MSG_BYTES <= 16384


# ---------------------------------------------------------------- the reference, once per workload
@functools.lru_cache(maxsize=None)
def _case(kind):
    w, batches = cases.workload(kind)
    want, want_en = _reference(w, batches)
    want.setflags(write=False)
    return w, batches, want, want_en


def _check(kind, parts):
    w, batches, want, want_en = _case(kind)
    got = _merge(parts, sum(b.n for b in batches))
    bad = np.nonzero((got != want).any(axis=0))[0]
    assert bad.size == 0, f"{bad.size} verdicts differ; first {bad[0]}: got {got[:, bad[0]]} want {want[:, bad[0]]}"
    assert (want[0] == abi.V_BLOCK_SYSTEM).sum() > 0, "the SystemRule never fired"
    assert (want[0] == abi.V_PASS).sum() > 0
    for p in parts:
        assert p[2] == want_en


def test_combined_rule_fires_each_reason():
    """The combined rule's thresholds (sysx_wide_cases.COMBINED): the QPS, the
    thread and the RT check each block some entry of the reference replay."""
    _, _, want, _ = _case("combined")
    reasons = want[2][want[0] == abi.V_BLOCK_SYSTEM]
    assert {0, 1, 2} <= set(int(x) for x in np.unique(reasons)), np.unique(reasons, return_counts=True)


@pytest.mark.parametrize("kind", ["thread", "rt", "load"])
def test_single_rules_fire_their_reason(kind):
    _, _, want, _ = _case(kind)
    reasons = set(int(x) for x in np.unique(want[2][want[0] == abi.V_BLOCK_SYSTEM]))
    assert reasons == {{"thread": 1, "rt": 2, "load": 3}[kind]}


# ---------------------------------------------------------------- CPU: the protocol over oracle engines
@pytest.fixture(scope="module")
def simlib(tmp_path_factory):
    return sim.build_lib(tmp_path_factory.mktemp("sxw"))


def _sim_rank(libpath, kind, world, rank, comm, log=None):
    from oracle import oracle as so
    w, batches = cases.workload(kind)
    L = sim.load_lib(libpath)
    cfg = _rank_cfg(w, batches, world, rank)
    o = so.OracleEngine(cfg)
    _load(o, w, world, rank)
    rule = sim.sim_rule(w["system"], w["status"])
    assert not L.sxw_c_rule_ok(rule), "a rule of the QPS path"
    pos, cols, off = [], [], 0
    for bi, b in enumerate(batches):
        sel = np.nonzero(b.res_id % world == rank)[0]
        recs = []
        v = sim.submit_node_wide(o, L, b.shard(world, rank), sel + off, comm, rule=rule, S=cfg.sample_count,
                                 interval=cfg.interval_ms, stat_max_rt=cfg.statistic_max_rt, log=recs)
        if log is not None:
            log.extend(dict(r, batch=bi, n_local=int(sel.size)) for r in recs)
        pos.append(sel + off)
        cols.append(np.stack([v.status, v.wait_ms, v.rule_idx]).astype(np.int64))
        off += b.n
    return np.concatenate(pos), np.concatenate(cols, axis=1), abi.node_state_to_dict(o.read_entry_node(),
                                                                                      cfg.sample_count)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("world", [2, 3])
def test_wide_protocol_local_ranks(simlib, kind, world):
    logs = [[] for _ in range(world)]
    parts = _threads(lambda r, c: _sim_rank(simlib, kind, world, r, c, logs[r]), world)
    _check(kind, parts)
    assert len(logs[0]) >= 2 and any(len(x["levels"]) > 1 for x in logs[0])      # rounds, and a refinement
    assert all(len(lg) == len(logs[0]) for lg in logs)                            # the same loop on every rank


def _gloo_worker(rank, world, port, libpath, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, _sim_rank(libpath, "combined", world, rank, system_shard.TorchComm())))
    dist.destroy_process_group()


def test_wide_protocol_gloo_two_ranks(simlib):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, simlib, q)) for r in range(2)]
    for p in procs:
        p.start()
    parts = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    _check("combined", [parts[0], parts[1]])


def _last_bin(level):
    """The next level's range is the last of BINS bins of this one."""
    nb = (level["hi"] - level["lo"] + level["w"] - 1) // level["w"]
    return (level["next"] is not None and level["w"] > 1 and nb == cases.BINS
            and level["next"][0] == level["lo"] + (nb - 1) * level["w"])


def _guard(kind, logs, batches):
    """What the border case must have reached (logs: per rank, one record per round)."""
    r0 = logs[0]
    rounds = range(len(r0))
    if kind == "few":
        return any(x["hi"] - x["lo"] < cases.BINS and x["levels"][0]["w"] == 1 for x in r0)
    if kind == "bins_plus_one":
        return any(x["hi"] - x["lo"] == cases.BINS + 1 and x["levels"][0]["w"] == 2 for x in r0)
    if kind == "last_bin":
        return any(_last_bin(lv) for x in r0 for lv in x["levels"])
    if kind == "same_bin":
        def same(x):
            lv = x["levels"][0]
            return lv["w"] > 1 and any((a - lv["lo"]) // lv["w"] == (b - lv["lo"]) // lv["w"] and a < x["q"]
                                       for a, b in x.get("exit_entry_seq", ()))
        return any(same(x) for lg in logs for x in lg)
    if kind == "earlier_round":
        return any(x.get("exits_earlier_round", 0) > 0 for lg in logs for x in lg)
    if kind == "earlier_batch":
        return any(x["batch"] == 1 and x.get("exits_earlier_batch", 0) > 0 for lg in logs for x in lg)
    if kind == "only_exits":
        return any(sum(lg[k]["local_entries"] for lg in logs) == 0 and sum(lg[k]["local_in_window"] for lg in logs) > 0
                   for k in rounds)
    if kind == "idle_rank":
        return any(min(lg[k]["local_in_window"] for lg in logs) == 0 and max(lg[k]["local_in_window"] for lg in logs) > 0
                   for k in rounds)
    if kind == "empty_batch":
        return any(min(lg[k]["n_local"] for lg in logs) == 0 and max(lg[k]["n_local"] for lg in logs) > 0
                   for k in rounds)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", cases.BORDERS)
def test_wide_protocol_borders(simlib, kind):
    _, batches, _, _ = _case(kind)
    assert sum(b.n for b in batches) <= 400
    logs = [[], []]
    parts = _threads(lambda r, c: _sim_rank(simlib, kind, 2, r, c, logs[r]), 2)
    _check(kind, parts)
    assert len(logs[0]) == len(logs[1])
    assert _guard(kind, logs, batches), f"the case does not reach its border: {kind}"


# ---------------------------------------------------------------- GPU: the product
class _CountingComm:
    def __init__(self, inner):
        self.inner, self.calls, self.largest = inner, 0, 0

    def allgather_bytes(self, x):
        self.calls += 1
        self.largest = max(self.largest, x.nbytes)
        return self.inner.allgather_bytes(x)


def _gpu_rank(kind, world, rank, comm, stats=None):
    from sentinel_amd import engine
    w, batches = cases.workload(kind)
    cfg = _rank_cfg(w, batches, world, rank)
    e = engine.FlowEngine(cfg)
    try:
        _load(e, w, world, rank)
        pos, cols, off = [], [], 0
        for b in batches:
            sel = np.nonzero(b.res_id % world == rank)[0]
            v = e.submit_node(b.shard(world, rank), sel + off, comm)        # the exchange itself: no fallback
            pos.append(sel + off)
            cols.append(np.stack([v.status, v.wait_ms, v.rule_idx]).astype(np.int64))
            off += b.n
        if stats is not None:
            s = e.stats()
            stats.append((int(s.sys_rounds), int(s.sys_exchanges)))
        return np.concatenate(pos), np.concatenate(cols, axis=1), abi.node_state_to_dict(e.read_entry_node(),
                                                                                          cfg.sample_count)
    finally:
        e.close()


def _gpu_node(kind, world):
    comms, stats = [], []

    def rank(r, c):
        cc = _CountingComm(c)
        comms.append(cc)
        return _gpu_rank(kind, world, r, cc, stats)
    parts = _threads(rank, world)
    _check(kind, parts)
    # the exchange ran (no event gather), every message within the wide format's size
    assert len(comms) == world and all(c.calls > 0 and c.largest <= abi.SYSX_WIDE_MSG_BYTES for c in comms)
    assert any(c.largest == abi.SYSX_WIDE_MSG_BYTES for c in comms)
    assert len(set(stats)) == 1 and stats[0][0] >= 1 and stats[0][1] >= stats[0][0]      # one loop on every rank
    return stats[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_wide_two_engines(kind):
    """30,000 events (three pipelined node batches, exits crossing their
    borders) under each wide rule, two engines on one GPU."""
    _, batches, _, _ = _case(kind)
    assert sum(b.n for b in batches) == 30_000 and len(batches) >= 2
    _gpu_node(kind, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", cases.BORDERS)
def test_gpu_wide_borders(kind):
    _gpu_node(kind, 2)


@pytest.mark.gpu
def test_gpu_wide_three_engines():
    _gpu_node("thread", 3)


@pytest.mark.gpu
def test_gpu_wide_pipelined_batches_exits_cross_border():
    """Two node batches; exits of the second close entries of the first (entry_ref -1 with a create time)."""
    _, batches, want, _ = _case("earlier_batch")
    assert len(batches) == 2
    b1 = batches[1]
    x = (b1.flags & (abi.EV_IN | abi.EV_EXIT)) == (abi.EV_IN | abi.EV_EXIT)
    assert (x & (b1.entry_ref == -1)).sum() > 0 and (x & (b1.entry_ref >= 0)).sum() > 0
    _gpu_node("earlier_batch", 2)


@pytest.mark.gpu
def test_gpu_wide_rccl_single_rank():
    """The wide exchange over the engine's RCCL communicator (device buffers,
    ncclAllGather on the engine's stream) on a one-rank node: equal to one
    engine deciding the batches with sf_submit, ENTRY_NODE included."""
    from sentinel_amd import engine
    w, batches = cases.workload("thread")
    c = w["cfg"]
    e, ref = engine.FlowEngine(c), engine.FlowEngine(c)
    try:
        for x in (e, ref):
            _load(x, w)
        e.comm_init(1, 0, engine.comm_unique_id())
        off, fired = 0, 0
        for b in batches:
            got = e.submit_node(b, np.arange(off, off + b.n, dtype=np.int64), None)
            want = ref.submit(b)
            off += b.n
            assert np.array_equal(got.status, want.status) and np.array_equal(got.wait_ms, want.wait_ms)
            assert np.array_equal(got.rule_idx, want.rule_idx)
            fired += int((want.status == abi.V_BLOCK_SYSTEM).sum())
        assert fired > 0
        assert abi.node_state_to_dict(e.read_entry_node()) == abi.node_state_to_dict(ref.read_entry_node())
    finally:
        e.close()
        ref.close()
