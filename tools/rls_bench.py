"""Throughput of the batched Envoy rate-limit service (sf_request_rls):
2^22 RateLimitRequests per call with 1-3 descriptors each, drawn Zipf(1.1)
over 1M descriptor rules (GLOBAL, sampleCount 1, 1-s window, as
EnvoyRlsRuleManager loads them), keys of about 30 bytes, hits_addend 1.

Legs, every array in device memory, timed with device events around the
synchronous call, alternated in one process (each leg on an engine of its own,
fed the same batches):
  a  sf_request_rls, string form
  b  sf_request_rls, pre-hashed form
  c  sf_request_tokens on the same flattened descriptor stream (what the
     engine offered for these decisions before sf_request_rls)
  d  leg b with the wave route switched off (SF_RLS_WAVE=0 at engine creation)
Every output of b and d is compared after every call.  The check step decides
a 64k-request prefix of the same generator in both forms and compares every
output (and the sums of a sample of rules) with the model (tests/rls_model.py);
the prefix is the first 64k requests of the timed stream's first call.  With
the default arguments a timing window of leg b is about a third of a second.

This script only drives: each device step is a child process under its own
time limit, and the first failure ends the run.  Results (median and
run-to-run spread of every leg) go to --out as JSON.  MEASUREMENT TOOL."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sentinel_amd import abi  # noqa: E402

SEED = 1
DOMAIN, KEY = "mesh-gateway.prod", "dest_cluster"            # key: 17 + 1 + 12 + 1 + 11 bytes


def java_hash_from(h, raw):
    for b in raw:
        h = (31 * h + b) & 0xFFFFFFFF
    return h


def rule_ids(n_rules):
    """flowId of "DOMAIN|KEY|svc-%07d" for every rule (ASCII keys: one code unit per byte)."""
    h0 = java_hash_from(0, f"{DOMAIN}|{KEY}|svc-".encode())
    h = np.full(n_rules, h0, np.uint32)
    r = np.arange(n_rules)
    for p in range(6, -1, -1):
        h = h * np.uint32(31) + (48 + (r // 10 ** p) % 10).astype(np.uint32)
    return (2 ** 31 - 1) + h.astype(np.int32).astype(np.int64)


def string_table(n_rules):
    vals = np.char.add("svc-", np.char.zfill(np.arange(n_rules).astype(str), 7)).astype("S11")
    data = DOMAIN.encode() + KEY.encode() + vals.tobytes()
    off = np.concatenate([[0, len(DOMAIN), len(DOMAIN) + len(KEY)],
                          len(DOMAIN) + len(KEY) + 11 * np.arange(1, n_rules + 1)]).astype(np.uint32)
    return off, data                                        # string 0 the domain, 1 the key, 2 + r the value of rule r


def gen(rng, n, n_rules, cdf):
    nd = rng.integers(1, 4, n)
    desc_off = np.concatenate([[0], np.cumsum(nd)]).astype(np.uint32)
    rule = np.searchsorted(cdf, rng.random(int(desc_off[-1]))).clip(0, n_rules - 1)
    return desc_off, rule


def call_times(a, step):
    """ts_ms of the requests of call `step`: span_ms of server time per call, evenly spread."""
    return 100_000 + step * a.span_ms + (np.arange(a.n, dtype=np.int64) * a.span_ms) // a.n


def zipf_cdf(n_rules):
    w = 1.0 / np.arange(1, n_rules + 1) ** 1.1
    return np.cumsum(w / w.sum())


def rules_of(ids, count):
    arr = (abi.sf_cluster_flow_rule * len(ids))()
    for i, f in enumerate(ids.tolist()):
        arr[i].flow_id, arr[i].count, arr[i].threshold_type = f, count, abi.THRESHOLD_GLOBAL
        arr[i].namespace_id, arr[i].sample_count, arr[i].window_interval_ms = 0, 1, 1000
    return arr


def load_rules(e, arr):
    from sentinel_amd import engine
    engine._check(engine.lib().sf_load_cluster_rules(e.h, arr, len(arr), None, 0, None, 0))


# ---------------------------------------------------------------- step: check
def step_check(a):
    from oracle import oracle as so
    from sentinel_amd import engine, rls
    from tests import rls_cases as rc
    from tests import rls_model as rm
    n = min(1 << 16, a.n)
    ids = rule_ids(a.rules)
    # the first n requests of the timed stream's first call: same generator, seed and times
    desc_off, rule = gen(np.random.default_rng(SEED), a.n, a.rules, zipf_cdf(a.rules))
    desc_off, rule = desc_off[:n + 1], rule[:int(desc_off[n])]
    ts = call_times(a, 0)[:n]
    reqs = [(DOMAIN, [[(KEY, "svc-%07d" % r)] for r in rule[desc_off[i]:desc_off[i + 1]]], 1, int(ts[i])) for i in range(n)]
    used = np.unique(rule)
    for r in used[:50]:
        assert rm.generate_flow_id(f"{DOMAIN}|{KEY}|svc-{r:07d}") == ids[r]
    flow = [rc.flow_rule(None, a.count, flow_id=int(ids[r])) for r in used]      # the model needs the rules it meets
    nd = int(desc_off[-1])
    m = rm.RlsModel(so, abi.default_config(max_resources=4, max_batch=nd), flow)
    want = m.should_rate_limit(reqs)
    probe = rc.Case("probe", flow[:150] + flow[-50:], [("rls", reqs)])              # the rules whose sums are compared
    want_sums = rc.sums(m, probe)
    arr = rules_of(ids, a.count)
    for prehashed in (False, True):
        e = engine.FlowEngine(abi.default_config(max_resources=4, max_batch=nd))
        load_rules(e, arr)
        got = e.request_rls(rls.pack_requests(reqs, prehashed=prehashed))
        for f in ("overall", "code", "limit", "remaining", "flow_id"):
            assert (getattr(got, f) == getattr(want, f)).all(), (prehashed, f)
        assert rc.sums(e, probe) == want_sums, prehashed
        e.close()
    codes = np.bincount(want.code, minlength=3).tolist()
    print(json.dumps({"checked_requests": n, "checked_descriptors": nd, "rules_touched": int(used.size),
                      "codes_unknown_ok_over": codes}))


# ---------------------------------------------------------------- step: time
class Dev:
    """Arrays of one leg in device memory, alive for the whole run."""

    def __init__(self, e):
        self.e, self.a = e, {}

    def put(self, name, host):
        from sentinel_amd import engine
        self.a[name] = engine.DeviceArray(self.e, np.ascontiguousarray(host))
        return self.a[name].ptr

    def set(self, name, host):
        from sentinel_amd import engine
        host = np.ascontiguousarray(host)
        engine._check(engine.lib().sf_memcpy(self.e.h, self.a[name].ptr, host.ctypes.data, host.nbytes, 0))


def step_time(a):
    import torch
    from sentinel_amd import engine
    L = engine.lib()
    n = a.n
    rng = np.random.default_rng(SEED)
    ids = rule_ids(a.rules)
    cdf = zipf_cdf(a.rules)
    batches = [gen(rng, n, a.rules, cdf) for _ in range(2)]
    nd_max = max(int(b[0][-1]) for b in batches)
    str_off, data = string_table(a.rules)
    arr = rules_of(ids, a.count)
    legs = {}
    for leg in "abcd":
        if leg == "d":
            os.environ["SF_RLS_WAVE"] = "0"
        e = engine.FlowEngine(abi.default_config(max_resources=4, max_batch=nd_max))
        os.environ.pop("SF_RLS_WAVE", None)
        load_rules(e, arr)
        d = Dev(e)
        per_batch = []
        for desc_off, rule in batches:
            nd = int(desc_off[-1])
            k = len(per_batch)
            req_of = np.repeat(np.arange(n), np.diff(desc_off.astype(np.int64)))
            if leg == "c":
                tb = abi.sf_token_batch()
                tb.n, tb.mem = nd, abi.MEM_DEVICE
                tb.flow_id, tb.count = d.put(f"fid{k}", ids[rule]), d.put(f"cnt{k}", np.ones(nd, np.int32))
                tb.flags, tb.ts_ms = d.put(f"fl{k}", np.zeros(nd, np.uint8)), d.put(f"ts{k}", np.zeros(nd, np.int64))
                tr = abi.sf_token_results()
                tr.mem = abi.MEM_DEVICE
                tr.status, tr.remaining, tr.wait_ms = (d.put(f"st{k}", np.zeros(nd, np.int8)),
                                                       d.put(f"rem{k}", np.zeros(nd, np.int32)),
                                                       d.put(f"wt{k}", np.zeros(nd, np.int32)))
                per_batch.append((tb, tr, req_of, nd))
                continue
            b = abi.sf_rls_batch()
            b.n, b.mem = n, abi.MEM_DEVICE
            b.ts_ms, b.hits_addend = d.put(f"ts{k}", np.zeros(n, np.int64)), d.put(f"hits{k}", np.ones(n, np.int32))
            b.desc_off = d.put(f"doff{k}", desc_off)
            if leg == "a":
                b.domain = d.put(f"dom{k}", np.zeros(n, np.uint32))
                b.ent_off = d.put(f"eoff{k}", np.arange(nd + 1, dtype=np.uint32))
                b.ent_key, b.ent_val = d.put(f"ek{k}", np.ones(nd, np.uint32)), d.put(f"ev{k}", (rule + 2).astype(np.uint32))
                if k == 0:
                    d.put("soff", str_off), d.put("bytes", np.frombuffer(data, np.uint8))
                b.str_off, b.bytes, b.n_str = d.a["soff"].ptr, d.a["bytes"].ptr, str_off.size - 1
            else:
                b.desc_flow_id = d.put(f"fid{k}", ids[rule])
            r = abi.sf_rls_results()
            r.mem = abi.MEM_DEVICE
            r.overall, r.code = d.put(f"all{k}", np.zeros(n, np.uint8)), d.put(f"code{k}", np.zeros(nd, np.uint8))
            r.limit, r.remaining = d.put(f"lim{k}", np.zeros(nd, np.int32)), d.put(f"rem{k}", np.zeros(nd, np.int32))
            r.flow_id = d.put(f"ofid{k}", np.zeros(nd, np.int64))
            per_batch.append((b, r, req_of, nd))
        legs[leg] = (e, d, per_batch)

    def call(leg, step):
        """One call of a leg on batch step % 2 at the step's times; returns device milliseconds."""
        e, d, per_batch = legs[leg]
        k = step % 2
        inp, out, req_of, nd = per_batch[k]
        ts = call_times(a, step)
        d.set(f"ts{k}", ts[req_of] if leg == "c" else ts)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        rc = (L.sf_request_tokens if leg == "c" else L.sf_request_rls)(e.h, C.byref(inp), C.byref(out))
        ev1.record()
        engine._check(rc)
        ev1.synchronize()
        return ev0.elapsed_time(ev1), nd

    def same_outputs(step):
        k = step % 2
        for name in (f"all{k}", f"code{k}", f"lim{k}", f"rem{k}", f"ofid{k}"):
            assert (legs["b"][1].a[name].numpy() == legs["d"][1].a[name].numpy()).all(), (step, name)

    step = 0
    for _ in range(a.warmup):
        for leg in "abcd":
            call(leg, step)
        same_outputs(step)
        step += 1
    windows = {leg: [] for leg in "abcd"}                   # (ms, descriptors) of every timing window
    for _ in range(a.windows):
        acc = {leg: [0.0, 0] for leg in "abcd"}
        for _ in range(a.calls):
            for leg in "abcd":                               # alternated: every leg sees the same drift
                ms, nd = call(leg, step)
                acc[leg][0] += ms
                acc[leg][1] += nd
            same_outputs(step)
            step += 1
        for leg in "abcd":
            windows[leg].append(acc[leg])
    res = {"requests_per_call": n, "descriptors_per_call": [p[3] for p in legs["b"][2]], "rules": a.rules,
           "rule_count": a.count, "calls_per_window": a.calls, "windows": a.windows, "span_ms_per_call": a.span_ms,
           "b_equals_d_every_call": True}
    for leg, name in zip("abcd", ("rls_strings", "rls_prehashed", "request_tokens", "rls_prehashed_no_wave")):
        ns = np.array([1e6 * ms / nd for ms, nd in windows[leg]])
        res[name] = {"ns_per_descriptor_median": round(float(np.median(ns)), 3),
                     "ns_per_descriptor_min_max": [round(float(ns.min()), 3), round(float(ns.max()), 3)],
                     "spread_rel": round(float((ns.max() - ns.min()) / np.median(ns)), 4),
                     "window_ms_median": round(float(np.median([ms for ms, _ in windows[leg]])), 2),
                     "descriptors_per_s": round(1e9 / float(np.median(ns)))}
    s = legs["b"][0].rls_stats()
    res["stats_b"] = {f: int(getattr(s, f)) for f, _ in abi.sf_rls_stats._fields_}
    for e, _, _ in legs.values():
        e.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--rules", type=int, default=1_000_000)
    ap.add_argument("--count", type=float, default=2000.0, help="threshold of every rule (per second)")
    ap.add_argument("--span-ms", type=int, default=20, help="server time one call covers")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=8, help="calls of every leg per timing window")
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--step", choices=["check", "time"])
    ap.add_argument("--limit-s", type=int, default=420, help="time limit of each device step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_rls_bench.json"))
    a = ap.parse_args()
    if a.step:
        return {"check": step_check, "time": step_time}[a.step](a)
    out = {"arguments": {k: v for k, v in vars(a).items() if k not in ("step", "out")}}
    for step in ("check", "time"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + sys.argv[1:]
        t0 = time.time()
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit_s)
        except subprocess.TimeoutExpired:
            print(f"step {step}: time limit of {a.limit_s} s", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"step {step} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        out[step] = json.loads(p.stdout.strip().split("\n")[-1])
        out[step]["step_seconds"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
