"""Cost of the embedded token server's two routes (sf_load_cluster_binds,
DESIGN.md §6g) on one hot cluster-limited resource.

Workload: 4096 resources, each with one cluster-mode rule bound to a GLOBAL
cluster flow rule of its own (no namespace limiter); resource 0 takes half of
the events, the rest a Zipf(1.1) tail; 2^22 entries per batch (acquireCount 1,
no exits) spread over one second, every array in device memory.

Legs, each a child process under its own time limit (the first failure ends
the run), timed by the engine's device events (sf_set_timing: sf_stats
.total_ms and .decide_ms per sf_submit) after warm-up batches:
  wave     the bound rules, k_decide_xcl takes the long segments
  lane     the same, SF_XCL_MIN raised at engine creation so that every
           segment stays on k_decide_x's lane
  unbound  the same rules without binds (local fallback).  As the yardstick
           this leg is run from a checkout of the parent commit
           (--legs unbound --out ...), not on this code.
wave and lane must give identical verdicts (compared through a digest).
Results (median, min, max of each leg) go to --out as JSON.  MEASUREMENT TOOL."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sentinel_amd import abi  # noqa: E402

R, T0 = 4096, 1_700_000_000_000


def batches(n, k, seed=5):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, R) ** 1.1
    p /= p.sum()
    out = []
    for i in range(k):
        res = np.where(rng.random(n) < 0.5, 0, 1 + rng.choice(R - 1, n, p=p)).astype(np.uint32)
        ts = np.sort(rng.integers(0, 1000, n)) + T0 + 1000 * i
        out.append(abi.HostBatch(res, ts, np.ones(n, np.int32), np.zeros(n, np.uint8)))
    return out


def leg(name, n, warmup, repeats):
    from sentinel_amd import engine
    if name == "lane":
        os.environ["SF_XCL_MIN"] = str(1 << 30)
    e = engine.FlowEngine(abi.default_config(max_resources=R, max_batch=n))
    rules = [abi.sf_flow_rule(resource=r, grade=abi.GRADE_QPS, count=2000.0 if r == 0 else 50.0, strategy=0,
                              control_behavior=0, warm_up_period_sec=10, max_queueing_time_ms=500, cluster_mode=1,
                              ref_resource=0xFFFFFFFF, limit_app=0, cluster_fallback=1) for r in range(R)]
    e.load_namespaces([abi.sf_namespace(namespace_id=1, connected_count=1, max_allowed_qps=-1.0)])
    e.load_cluster_rules(flow=[abi.sf_cluster_flow_rule(flow_id=1000 + r, count=2000.0 if r == 0 else 50.0,
                                                        threshold_type=abi.THRESHOLD_GLOBAL, namespace_id=1,
                                                        sample_count=10, window_interval_ms=1000) for r in range(R)])
    e.load_flow_rules(rules)
    if name != "unbound":
        e.load_cluster_binds([(r, 1000 + r) for r in range(R)])
    hbs = batches(n, warmup + repeats)
    dbs = [engine.DeviceBatch(e, hb) for hb in hbs]
    dv = engine.DeviceVerdicts(e, n, with_wait=True, with_rule=True)
    total, decide, h = [], [], hashlib.sha256()
    for i, db in enumerate(dbs):
        e.set_timing(True)                                 # (clears the sums)
        e.submit_device(db, dv)
        s = e.stats()
        h.update(dv.status.numpy().tobytes())
        if i >= warmup:
            total.append(s.total_ms)
            decide.append(s.decide_ms)
    s = e.stats()
    out = {"leg": name, "events": n, "warmup": warmup, "repeats": repeats, "total_ms": stat(total), "decide_ms": stat(decide),
           "digest": h.hexdigest()}
    if hasattr(s, "xcl_chunks_wave"):
        out.update(xcl_chunks_wave=int(s.xcl_chunks_wave), xcl_chunks_serial=int(s.xcl_chunks_serial))
    e.close()
    print(json.dumps(out))


def stat(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="wave,lane")
    ap.add_argument("--leg", default=None, help="(child) run one leg")
    ap.add_argument("--limit", type=int, default=240, help="seconds per leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.events, a.warmup, a.repeats)
    res = {}
    for name in a.legs.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--events", str(a.events),
                            "--warmup", str(a.warmup), "--repeats", str(a.repeats)], capture_output=True, text=True,
                           timeout=a.limit)
        if r.returncode:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"leg {name} failed ({r.returncode}): nothing more is started")
        res[name] = json.loads(r.stdout.strip().split("\n")[-1])
    if "wave" in res and "lane" in res:
        assert res["wave"]["digest"] == res["lane"]["digest"], "the two routes gave different verdicts"
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
