"""What the AuthorityRule mark pass costs, on config 3's traffic (trace.mixed_zipf
+ trace.mixed_rules, HBM-resident batches through sf_submit_async as bench.py
submits them) with a 64-origin Zipf(1.1) origin on every entry
(trace.with_origins), each step the same trace one DURATION_MS later.

  (a) no AuthorityRules: this tree's library against the parent commit's
      (--parent-lib, built from the parent's sources), same box, same session.
      Each variant is a worker process that keeps its engine; the rounds
      alternate the workers (new, parent, rules ..., new, parent, ...), every
      round `--steps` batches from the first enqueue to the sync.  Reported per
      variant: every round, the median, the spread (max - min).  The claim "no
      cost when unused" holds when the two medians differ by less than the
      spreads.
  (b) white / black rules on 1 % and on 100 % of the resources (lists of 1-16
      of the 64 origins): the extra time per batch over the no-rules variant of
      the same library, the share of entries blocked, and sf_authority_mark on
      the same device arrays alone -- the call's wall clock (launch + kernel +
      sync, so an upper bound of the kernel's time) and the bytes per second
      that gives against the 10 B per event the pass moves (res 4, origin 4,
      flags 1 in, 1 out; the auth_of gather not counted).

Prints one JSON line; --out also writes it to a file.  MEASUREMENT TOOL."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DURATION_MS = 4000
RING = 4


def authority_rules(R, frac, seed=5, n_origins=64):
    """(resource, strategy, [origin ids]) on ``frac`` of the resources, the busiest first (Zipf ranks are
    permuted by the trace, so "busiest" is drawn from the batch), black and white alternating."""
    rng = np.random.default_rng(seed)
    k = max(1, int(round(R * frac)))
    res = np.arange(R) if k >= R else rng.choice(R, size=k, replace=False)
    lens = rng.integers(1, 17, res.size)
    out = []
    for i, r in enumerate(res):
        ids = (2 + rng.choice(n_origins, size=int(lens[i]), replace=False)).tolist()
        out.append((int(r), i & 1, ids))
    return out


def worker(a):
    """One variant: builds the trace and the engine, then answers "run" lines with a JSON line each."""
    from sentinel_amd import abi, engine, trace
    hb = trace.with_origins(trace.mixed_zipf(a.resources, a.events, duration_ms=DURATION_MS, seed=3), seed=13)
    rules = trace.mixed_rules(a.resources, seed=3)
    e = engine.FlowEngine(abi.default_config(max_resources=a.resources, max_batch=hb.n))
    e.load_flow_rules(rules)
    info = {"rules_kept": 0}
    if a.rule_frac > 0:
        info["rules_kept"] = e.load_authority_rules(authority_rules(a.resources, a.rule_frac))
    base = engine.DeviceBatch(e, hb)
    ring = [base] + [engine.DeviceBatch.with_ts(e, base, hb.ts_ms) for _ in range(RING - 1)]
    out = engine.DeviceVerdicts(e, hb.n, with_wait=True, with_rule=False)
    step = 0

    def run(steps):
        nonlocal step
        total = 0.0
        for lo in range(0, steps, RING):
            m = min(RING, steps - lo)
            for k in range(m):                                       # (outside the timed stretch)
                ts = np.ascontiguousarray(hb.ts_ms + (step + k) * DURATION_MS)
                engine._check(engine.lib().sf_memcpy(e.h, ring[k].arrays["ts_ms"].ptr, ts.ctypes.data, ts.nbytes, 0))
            e.sync()
            t = time.perf_counter()
            for k in range(m):
                e.submit_device_async(ring[k], out)
            e.sync()
            total += time.perf_counter() - t
            step += m
        return 1e3 * total / steps

    run(a.warmup)
    st = out.status.numpy()
    ent = (hb.flags & abi.EV_EXIT) == 0
    info["blocked_share"] = round(float((st == getattr(abi, "V_BLOCK_AUTHORITY", 10)).sum() / ent.sum()), 5)
    if a.rule_frac > 0:                                              # the mark pass alone, on the batch's arrays
        mo = engine.DeviceArray.empty(e, hb.n, np.uint8)
        arr = base.arrays
        for _ in range(3):
            e.authority_mark_device(arr["res_id"], arr["origin"], arr["flags"], mo)
        us = []
        for _ in range(a.mark_reps):
            t = time.perf_counter()
            e.authority_mark_device(arr["res_id"], arr["origin"], arr["flags"], mo)
            us.append(1e6 * (time.perf_counter() - t))
        info["mark_call_us"] = [round(x, 1) for x in sorted(us)[:: max(1, len(us) // 8)]]
        info["mark_call_us_median"] = round(float(np.median(us)), 1)
        info["mark_bytes_per_s_from_call"] = round(10.0 * hb.n / (float(np.median(us)) * 1e-6))
        mo.free()
    print(json.dumps({"ready": True, "events": int(hb.n), **info}), flush=True)
    for line in sys.stdin:
        if line.strip() != "run":
            break
        print(json.dumps({"ms_per_batch": round(run(a.steps), 4)}), flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1 << 24)
    ap.add_argument("--resources", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=8, help="batches per variant and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mark-reps", type=int, default=40)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libsentinel_flow.so: part (a)")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--rule-frac", type=float, default=0.0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    variants = [("new_no_rules", None, 0.0)]
    if a.parent_lib:
        variants.append(("parent_no_rules", os.path.abspath(a.parent_lib), 0.0))
    variants += [("new_rules_1pct", None, 0.01), ("new_rules_100pct", None, 1.0)]
    procs, info = {}, {}
    try:
        for name, libpath, frac in variants:                         # one at a time: the set-up is not timed
            env = dict(os.environ)
            if libpath:
                env["SENTINEL_FLOW_LIB"] = libpath
            else:
                env.pop("SENTINEL_FLOW_LIB", None)
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--events", str(a.events),
                                  "--resources", str(a.resources), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                  "--mark-reps", str(a.mark_reps), "--rule-frac", str(frac)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
            procs[name] = p
            line = p.stdout.readline()
            if not line:
                raise RuntimeError(f"worker {name} ended before it was ready (exit status {p.wait()})")
            info[name] = json.loads(line)
        ms = {name: [] for name in procs}
        for _ in range(a.rounds):
            for name, p in procs.items():                            # interleaved
                p.stdin.write("run\n")
                p.stdin.flush()
                line = p.stdout.readline()
                if not line:
                    raise RuntimeError(f"worker {name} ended during a round (exit status {p.wait()})")
                ms[name].append(json.loads(line)["ms_per_batch"])
    finally:
        for p in procs.values():
            try:
                p.stdin.close()
            except OSError:
                pass
        for p in procs.values():
            try:
                p.wait(timeout=60)
            except subprocess.TimeoutExpired:
                p.kill()
    res = {"what": "config 3's traffic with a 64-origin Zipf column, HBM-resident batches through sf_submit_async: "
                   "the AuthorityRule mark pass unused, on 1 % and on 100 % of the resources",
           "events": info["new_no_rules"]["events"], "resources": a.resources, "steps_per_round": a.steps,
           "rounds": a.rounds, "warmup_steps": a.warmup, "variants": {}}
    for name in procs:
        x = ms[name]
        res["variants"][name] = {"ms_per_batch_rounds": x, "ms_per_batch": round(float(np.median(x)), 4),
                                 "spread_ms": round(max(x) - min(x), 4),
                                 **{k: v for k, v in info[name].items() if k not in ("ready", "events")}}
    base = res["variants"]["new_no_rules"]["ms_per_batch"]
    for name in ("new_rules_1pct", "new_rules_100pct"):
        res["variants"][name]["extra_ms_per_batch"] = round(res["variants"][name]["ms_per_batch"] - base, 4)
    if a.parent_lib:
        d = base - res["variants"]["parent_no_rules"]["ms_per_batch"]
        sp = max(res["variants"]["new_no_rules"]["spread_ms"], res["variants"]["parent_no_rules"]["spread_ms"])
        res["unused_cost"] = {"new_minus_parent_ms": round(d, 4), "larger_spread_ms": sp,
                              "within_spread": bool(abs(d) <= sp)}
    else:
        res["unused_cost"] = "not measured (no --parent-lib)"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
