"""Cost of parsing gateway requests on the device (sf_gateway_args) beside the
submit it feeds: 2^22 requests per call with 1-3 entries each over 1000 routes,
three item rules per route (client IP without pattern, a header matched EXACT,
a cookie matched CONTAINS), values of 8-64 bytes.

Legs, every array in device memory, timed with device events around the
synchronous call, alternated call by call in one process on one engine:
  a  sf_gateway_args: the requests -> the event columns
  b  sf_submit of the batch leg a just wrote
and, once, the one-core rate of the same parser code on the host
(tools/gateway_host.cpp runs sf_gateway.h's gw_entry over the first batch; its
output checksum must equal the device's).  The check step parses a prefix of
the same generator in host memory and compares every column with the model
(tests/gateway_model.py).

This script only drives: each device step is a child process under its own
time limit, and the first failure ends the run.  Results (median and
run-to-run spread of every leg) go to --out as JSON.  MEASUREMENT TOOL."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sentinel_amd import abi, gateway as gw  # noqa: E402

SEED = 1
N_IP, N_HDR, N_COOKIE = 1 << 14, 4096, 8192


def rules_of(R):
    out = []
    for r in range(R):
        name = f"route-{r:04d}"
        out.append(gw.GatewayRule(r, name, count=5, item=gw.ParamItem(gw.PARSE_CLIENT_IP)))
        out.append(gw.GatewayRule(r, name, count=2000, item=gw.ParamItem(gw.PARSE_HEADER, "x-tenant", pattern_of(r), gw.MATCH_EXACT)))
        out.append(gw.GatewayRule(r, name, count=50, item=gw.ParamItem(gw.PARSE_COOKIE, "sid", "sess", gw.MATCH_CONTAINS)))
    return out


def pattern_of(r):
    return f"tenant-header-value-{r:04d}"


def strings(R):
    """The string pool of every batch: [IPs | the routes' header patterns | other header values | cookies]."""
    rng = np.random.default_rng(SEED + 1)
    ips = ["10.%d.%d.%d" % (k >> 12, (k >> 6) & 63, (k & 63) * 4 + 1) for k in range(N_IP)]
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz0123456789"))
    word = lambda n: "".join(rng.choice(letters, n))  # noqa: E731
    hdr = [pattern_of(r) for r in range(R)] + [word(int(rng.integers(8, 65))) for _ in range(N_HDR)]
    cookies = []
    for k in range(N_COOKIE):
        s = word(int(rng.integers(32, 61)))
        if k % 2:
            cut = int(rng.integers(0, len(s)))
            s = s[:cut] + "sess" + s[cut:]
        cookies.append(s)
    return ips + hdr + cookies


def gen(rng, n, R, fields):
    """Arrays of one sf_gateway_batch over the pool (no ts: set per call)."""
    ne = rng.integers(1, 4, n)
    res_off = np.concatenate([[0], np.cumsum(ne)]).astype(np.uint32)
    res_id = rng.integers(0, R, int(res_off[-1])).astype(np.uint32)
    first = res_id[res_off[:-1]]
    hdr = np.where(rng.random(n) < 0.5, N_IP + first, N_IP + R + rng.integers(0, N_HDR, n))
    val_str = np.stack([rng.integers(0, N_IP, n), hdr, N_IP + R + N_HDR + rng.integers(0, N_COOKIE, n)], 1)
    return dict(count=np.ones(n, np.int32), flags=np.full(n, abi.EV_IN, np.uint8), res_off=res_off, res_id=res_id,
                res_mode=np.zeros(res_id.size, np.int32), val_off=(3 * np.arange(n + 1)).astype(np.uint32),
                val_field=np.tile(np.array(fields, np.uint32), n), val_str=val_str.astype(np.uint32).ravel(),
                val_flags=np.zeros(3 * n, np.uint8), ev_index=res_off[:-1].copy())


def call_times(a, step):
    return 100_000 + step * a.span_ms + (np.arange(a.n, dtype=np.int64) * a.span_ms) // a.n


def table_of(a):
    t = gw.RuleTable(rules_of(a.routes))
    fields = [t.fields[(gw.PARSE_CLIENT_IP, None)], t.fields[(gw.PARSE_HEADER, "x-tenant")], t.fields[(gw.PARSE_COOKIE, "sid")]]
    return t, fields


# ---------------------------------------------------------------- step: check
def step_check(a):
    from sentinel_amd import engine
    from tests import gateway_model as gm
    n = min(4096, a.n)
    t, fields = table_of(a)
    pool = strings(a.routes)
    g = gen(np.random.default_rng(SEED), a.n, a.routes, fields)
    ne = int(g["res_off"][n])
    str_off, data = abi.string_table(pool)
    ts = call_times(a, 0)[:n]
    hb = abi.HostGatewayBatch(ts_ms=ts, count=g["count"][:n], flags=g["flags"][:n], res_off=g["res_off"][:n + 1],
                              res_id=g["res_id"][:ne], res_mode=g["res_mode"][:ne], val_off=g["val_off"][:n + 1],
                              val_field=g["val_field"][:3 * n], val_str=g["val_str"][:3 * n], val_flags=g["val_flags"][:3 * n],
                              str_off=str_off, data=data, ev_index=g["ev_index"][:n])
    reqs = []
    for i in range(n):
        v = g["val_str"][3 * i:3 * i + 3]
        reqs.append(dict(ts_ms=int(ts[i]), entries=[(int(r), 0) for r in g["res_id"][g["res_off"][i]:g["res_off"][i + 1]]],
                         client_ip=pool[v[0]], headers={"x-tenant": pool[v[1]]}, cookies={"sid": pool[v[2]]}))
    ev = abi.HostGatewayEvents(ne)
    want = gm.columns(gm.Converted(t.rules), reqs, hb.ev_index, ev)
    e = engine.FlowEngine(abi.default_config(max_resources=a.routes, max_batch=ne))
    t.load(e)
    e.gateway_args(hb, ev)
    for c, _ in ev.COLUMNS:
        assert (getattr(ev, c) == getattr(want, c)).all(), c
    e.close()
    nm = int((want.arg_bits == gm.bits_of("$NM")).sum())
    print(json.dumps({"checked_requests": n, "checked_entries": ne, "not_match_slots": nm}))


# ---------------------------------------------------------------- step: time
def host_rate(a, t, g, ts, str_off, data):
    """gw_entry on one core over the batch; returns the program's JSON."""
    from sentinel_amd import engine
    _, _, _, desc = engine.gateway_convert(t.c_rules, t.patterns)
    poff, pdata = abi.string_table(t.patterns)
    slot_t = np.dtype([("field_id", "<u4"), ("parse", "<i4"), ("match", "<i4"), ("pat_off", "<u4"), ("pat_len", "<u4")])
    desc_t = np.dtype([("n_slots", "<u4"), ("n_item", "<u4"), ("gate", "<i4"), ("pad", "<u4"), ("slot", slot_t, (4,))])
    dd = np.zeros(len(desc), desc_t)
    of = np.full(a.routes, 0xFFFFFFFF, np.uint32)
    for k, d in enumerate(desc):
        of[d.resource] = k
        dd[k]["n_slots"], dd[k]["n_item"], dd[k]["gate"] = d.n_slots, d.n_item_slots, d.mode_gate
        for s in range(d.n_item_slots):
            x = d.slot[s]
            plen = 0 if x.pattern == abi.GW_NONE else int(poff[x.pattern + 1] - poff[x.pattern])
            dd[k]["slot"][s] = (x.field_id, x.parse_strategy, x.match_strategy, int(poff[x.pattern]) if plen else 0, plen)
    arrays = [ts, g["count"], g["flags"], g["res_off"], g["res_id"], g["res_mode"], g["val_off"], g["val_field"], g["val_str"],
              str_off, data, g["ev_index"], of, dd, pdata]
    head = np.array([a.n, g["res_id"].size, g["val_field"].size, str_off.size - 1, data.size, a.routes, len(desc), pdata.size],
                    np.uint32)
    with tempfile.TemporaryDirectory() as d:
        path, exe = os.path.join(d, "batch.bin"), os.path.join(d, "gateway_host")
        with open(path, "wb") as f:
            for x in [head] + arrays:
                raw = np.ascontiguousarray(x).tobytes()
                f.write(raw + b"\0" * (-len(raw) % 8))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "gateway_host.cpp")])
        return json.loads(subprocess.run([exe, path, "3"], capture_output=True, text=True, check=True).stdout)


def step_time(a):
    import torch
    from sentinel_amd import engine
    L = engine.lib()
    t, fields = table_of(a)
    rng = np.random.default_rng(SEED)
    batches = [gen(rng, a.n, a.routes, fields) for _ in range(2)]
    str_off, data = abi.string_table(strings(a.routes))
    ne_max = max(g["res_id"].size for g in batches)
    e = engine.FlowEngine(abi.default_config(max_resources=a.routes, max_batch=ne_max, param_capacity=1 << 24))
    t.load(e)
    put = lambda x: engine.DeviceArray(e, np.ascontiguousarray(x))  # noqa: E731
    d_soff, d_data = put(str_off), put(data)
    per = []
    for g in batches:
        ne = g["res_id"].size
        dev = {k: put(v) for k, v in g.items()}
        dev["ts_ms"] = put(np.zeros(a.n, np.int64))
        gb = abi.sf_gateway_batch()
        gb.n, gb.mem, gb.n_str = a.n, abi.MEM_DEVICE, str_off.size - 1
        for k, v in dev.items():
            setattr(gb, k, v.ptr)
        gb.str_off, gb.bytes = d_soff.ptr, d_data.ptr
        cols = {c: engine.DeviceArray.empty(e, (abi.SF_MAX_ARGS, ne) if c.startswith("arg_") else (ne,), dt)
                for c, dt in abi.HostGatewayEvents.COLUMNS}
        go = abi.sf_gateway_events()
        go.mem, go.n_total = abi.MEM_DEVICE, ne
        eb = abi.sf_event_batch()
        eb.n, eb.mem, eb.arg_slots = ne, abi.MEM_DEVICE, abi.SF_MAX_ARGS
        for c, v in cols.items():
            setattr(go, c, v.ptr)
            setattr(eb, c, v.ptr)
        verd = engine.DeviceVerdicts(e, ne, with_wait=True, with_rule=True)
        per.append((gb, go, eb, verd, dev, cols, ne))

    def timed(fn, *args):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        rc = fn(*args)
        ev1.record()
        engine._check(rc)
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    def call(step):
        gb, go, eb, verd, dev, _, ne = per[step % 2]
        ts = call_times(a, step)
        engine._check(L.sf_memcpy(e.h, dev["ts_ms"].ptr, ts.ctypes.data, ts.nbytes, 0))
        v = verd.c_struct()
        ms_a = timed(L.sf_gateway_args, e.h, C.byref(gb), C.byref(go))       # alternated call by call
        ms_b = timed(L.sf_submit, e.h, C.byref(eb), C.byref(v))
        return ms_a, ms_b, ne

    step = 0
    for _ in range(a.warmup):
        call(step)
        step += 1
    # the first batch's columns as the device wrote them, for the host program's checksum
    _, _, _, verd, _, cols, ne0 = per[0]
    call(step); step += 1
    call(step); step += 1                                  # (step is even again: the last call of batch 0 is two back)
    bits, tag = cols["arg_bits"].numpy().ravel(), cols["arg_tag"].numpy().ravel()
    k = np.arange(1, bits.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        checksum = int((bits * k).sum(dtype=np.uint64) + tag.sum(dtype=np.uint64)
                       + (cols["n_args"].numpy().astype(np.uint64) * np.uint64(31)).sum(dtype=np.uint64)
                       + cols["res_id"].numpy().sum(dtype=np.uint64))
    status = np.bincount(per[1][3].status.numpy(), minlength=8).tolist()
    windows = []
    for _ in range(a.windows):
        acc = [0.0, 0.0, 0]
        for _ in range(a.calls):
            ms_a, ms_b, ne = call(step)
            acc[0] += ms_a; acc[1] += ms_b; acc[2] += ne
            step += 1
        windows.append(acc)
    res = {"requests_per_call": a.n, "entries_per_call": [p[6] for p in per], "routes": a.routes, "rules": 3 * a.routes,
           "calls_per_window": a.calls, "windows": a.windows, "span_ms_per_call": a.span_ms,
           "string_pool": {"strings": int(str_off.size - 1), "bytes": int(data.size)}, "verdicts_last_call": status}
    for i, name in enumerate(("gateway_args", "submit")):
        ns = np.array([1e6 * w[i] / w[2] for w in windows])
        res[name] = {"ns_per_entry_median": round(float(np.median(ns)), 3),
                     "ns_per_entry_min_max": [round(float(ns.min()), 3), round(float(ns.max()), 3)],
                     "spread_rel": round(float((ns.max() - ns.min()) / np.median(ns)), 4),
                     "window_ms_median": round(float(np.median([w[i] for w in windows])), 2)}
    res["args_share_of_submit"] = round(res["gateway_args"]["ns_per_entry_median"] / res["submit"]["ns_per_entry_median"], 4)
    e.close()
    host = host_rate(a, t, batches[0], call_times(a, 0), str_off, data)
    assert host["checksum"] == checksum, (host["checksum"], checksum)
    res["host_one_core"] = {"ns_per_entry_best_of_3": host["ns_per_entry_best"], "outputs_equal_device": True}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--routes", type=int, default=1000)
    ap.add_argument("--span-ms", type=int, default=1000, help="gateway time one call covers")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=4, help="calls of every leg per timing window")
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--step", choices=["check", "time"])
    ap.add_argument("--limit-s", type=int, default=420, help="time limit of each device step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_gateway_bench.json"))
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
