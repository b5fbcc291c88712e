"""A ParamFlow batch from page-locked host memory, three ways on one engine:
config 4's traffic (trace.param_zipf: 2^24 events on 1000 resources, one LONG
argument per event drawn Zipf(1.1) over 100M keys, no SystemRule), each step
the same trace one DURATION_MS later.

  soa            sf_submit of the sf_event_batch SoA with host verdicts: the
                 path a batch with arguments had to take before the packed
                 forms carried them (synchronous: copy in, decide, copy back)
  packed         sf_submit_packed_sparse_async, 8-byte words + 9 B per argument,
                 double-buffered as the Java flusher does (enqueue k+1, then
                 sf_sync_packed_sparse of k)
  packed_narrow  the same with 4-byte words and the per-millisecond table

The three alternate round by round on the same engine (its clock only moves
forward), after warm-up steps of each; per path the milliseconds per batch of
every round (the round's wall clock over its batches: for soa the sum of the
calls, for the packed paths first enqueue to last sync, the pipeline's fill
included) and the median of the rounds, and the bytes per event that cross
PCIe in each direction (computed from the arrays, not timed).  --check decides
the first batch on a fresh engine per path and compares every verdict.  Prints
one JSON line; --out also writes it to a file.  MEASUREMENT TOOL."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd import abi, engine, trace  # noqa: E402

DURATION_MS = 4000


def pinned_soa(pin, hb):
    def cp(x):
        return None if x is None else pin.array(x.shape, x.dtype, x)
    return abi.HostBatch(cp(hb.res_id), cp(hb.ts_ms), cp(hb.count), cp(hb.flags), arg_tag=cp(hb.arg_tag),
                         arg_bits=cp(hb.arg_bits))


class Paths:
    """The three submit paths over one engine's pinned arrays; `step` is the engine's clock."""

    def __init__(self, e, hb):
        self.e, self.n = e, hb.n
        self.pin = engine.PinnedArrays(e)
        self.soa = pinned_soa(self.pin, hb)
        self.ts0 = hb.ts_ms.copy()
        self.soa_out = self.pin.verdicts(hb.n)
        self.pb = {"packed": abi.PackedBatch(hb, alloc=self.pin.array),
                   "packed_narrow": abi.PackedBatch(hb, alloc=self.pin.array, narrow=True)}
        self.base = self.pb["packed"].ts_base
        self.pre = hb.n // 64
        self.outs = [self.pin.sparse_verdicts(hb.n, self.pre) for _ in range(2)]
        self.step = 0

    def run_soa(self, steps):
        ts = []
        for _ in range(steps):
            self.soa.ts_ms[...] = self.ts0 + self.step * DURATION_MS       # (outside the timed call)
            self.step += 1
            t = time.perf_counter()
            self.e.submit(self.soa, self.soa_out)
            ts.append(time.perf_counter() - t)
        return 1e3 * float(np.sum(ts)) / steps                             # the mean, as run_packed's

    def run_packed(self, name, steps):
        pb = self.pb[name]
        self.e.sync()
        t = time.perf_counter()
        for k in range(steps):
            pb.ts_base = self.base + self.step * DURATION_MS
            self.step += 1
            self.e.submit_packed_sparse_async(pb, self.outs[k & 1])
            if k:
                self.e.sync_packed_sparse(self.outs[(k - 1) & 1])
        self.e.sync()
        return 1e3 * (time.perf_counter() - t) / steps

    def d2h_bytes(self):
        o = self.outs[0]
        lists = [int(o.counts[0]), int(o.counts[1])]
        return self.n + 8 + 2 * 8 * min(self.pre, self.n) + 8 * sum(max(0, c - self.pre) for c in lists)

    def close(self):
        self.pin.free()


def first_batch_statuses(cfg, rules, hb):
    """Batch 0 decided on a fresh engine by each path: (status, wait, rule) triples."""
    got = {}
    for name in ("soa", "packed", "packed_narrow"):
        e = engine.FlowEngine(cfg)
        e.load_param_rules(rules)
        p = Paths(e, hb)
        if name == "soa":
            e.submit(p.soa, p.soa_out)
            v = p.soa_out
        else:
            e.submit_packed_sparse_async(p.pb[name], p.outs[0])
            e.sync()
            v = p.outs[0].dense()
        got[name] = (v.status.copy(), v.wait_ms.copy(), v.rule_idx.copy())
        p.close()
        e.close()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--resources", type=int, default=1000)
    ap.add_argument("--keys", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=4, help="batches per path and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2, help="untimed batches per path before the rounds")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    rules, hb = trace.param_zipf(a.resources, a.n, a.keys, duration_ms=DURATION_MS, seed=4)
    cap = 1 << int(np.ceil(np.log2(max(2 * hb.n * 4, 1 << 16))))
    cfg = abi.default_config(max_resources=a.resources, max_batch=hb.n, param_capacity=cap)
    res = {"what": "config 4's traffic (ParamFlow, one LONG argument per event, no SystemRule) from page-locked "
                   "host memory: SoA sf_submit against the double-buffered packed forms",
           "events": int(hb.n), "resources": a.resources, "keys": a.keys, "steps_per_round": a.steps,
           "rounds": a.rounds, "warmup_steps": a.warmup}
    if a.check:
        got = first_batch_statuses(cfg, rules, hb)
        res["first_batch_verdicts_equal"] = bool(all(
            all(np.array_equal(x, y) for x, y in zip(got["soa"], got[k])) for k in ("packed", "packed_narrow")))
    e = engine.FlowEngine(cfg)
    e.load_param_rules(rules)
    p = Paths(e, hb)
    try:
        names = ("soa", "packed", "packed_narrow")
        run = {"soa": p.run_soa, "packed": lambda s: p.run_packed("packed", s),
               "packed_narrow": lambda s: p.run_packed("packed_narrow", s)}
        for k in names:
            run[k](a.warmup)
        ms = {k: [] for k in names}
        for _ in range(a.rounds):
            for k in names:
                ms[k].append(round(run[k](a.steps), 3))
        n = hb.n
        slots = hb.arg_tag.shape[0]
        h2d = {"soa": (4 + 8 + 4 + 1 + 9 * slots) * n, "packed": p.pb["packed"].nbytes(),
               "packed_narrow": p.pb["packed_narrow"].nbytes()}
        d2h = {"soa": 7 * n, "packed": p.d2h_bytes(), "packed_narrow": p.d2h_bytes()}
        res["paths"] = {k: {"ms_per_batch_rounds": ms[k], "ms_per_batch": round(float(np.median(ms[k])), 3),
                            "events_per_s": round(n / (float(np.median(ms[k])) / 1e3)),
                            "h2d_bytes_per_event": round(h2d[k] / n, 3),
                            "d2h_bytes_per_event": round(d2h[k] / n, 3)} for k in names}
        res["param_table"] = e.param_table_stats()
    finally:
        p.close()
        e.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
