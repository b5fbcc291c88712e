"""Throughput of the cluster concurrency tokens (sf_request_concurrent):
batches of 2^22 requests over 10,000 flowIds drawn Zipf(1.1), a threshold per
flowId at about half the concurrency its requests offer, 40 % of every batch
releases of the previous batch's tokens (a request that got none: its id is 0,
ALREADY_RELEASE).  Host arrays in, host arrays out: the time of one call as a
TokenService front-end sees it.

Prints one JSON line: milliseconds per batch, decisions per second, the chunk
solver's counters, and the same request count through sf_request_tokens (flow
requests of the same flowIds) for scale.  --flows 1 is the worst case of the
walk: one flowId, one wavefront's serial chain of chunks.  --check replays a
2^18-request run of the same generator (4 batches of 2^16) on the sequential
model of the reference (tests/concurrent_model.py) and compares every status,
nowCalls and the live tokens.  --tokens-only times sf_request_tokens alone.
MEASUREMENT TOOL."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd import abi, engine  # noqa: E402

RELEASE_SHARE = 0.4


def flows(n_flow, batch_n):
    ids = np.arange(1, n_flow + 1, dtype=np.int64)
    w = 1.0 / np.arange(1, n_flow + 1) ** 1.1
    w /= w.sum()
    # a flowId's acquires per batch x the mean count 2 is the concurrency it offers; the threshold is half
    thr = np.maximum(1.0, np.floor(batch_n * (1 - RELEASE_SHARE) * w * 2 * 0.5))
    return ids, w, thr


def rules_of(ids, thr):
    return [abi.sf_cluster_flow_rule(int(f), float(c), abi.THRESHOLD_GLOBAL, 0, 10, 1000) for f, c in zip(ids, thr)]


def gen_batch(rng, n, ids, w, prev_tokens, ts):
    """prev_tokens: token_id of the previous batch's acquires (0: got none), or None."""
    op = np.zeros(n, np.uint8)
    rid = ids[np.searchsorted(np.cumsum(w), rng.random(n)).clip(0, ids.size - 1)]
    if prev_tokens is not None:
        n_rel = min(int(n * RELEASE_SHARE), prev_tokens.size)
        pos = rng.permutation(n)[:n_rel]
        op[pos] = abi.CC_RELEASE
        rid[pos] = rng.permutation(prev_tokens)[:n_rel]
    return abi.HostConcurrentBatch(op, rid, rng.integers(1, 4, n), rng.integers(0, 64, n), np.full(n, ts, np.int64))


def time_tokens(e, ids, w, n, steps, warmup, rng):
    ts = []
    for k in range(warmup + steps):
        rid = ids[np.searchsorted(np.cumsum(w), rng.random(n)).clip(0, ids.size - 1)]
        b = abi.HostTokenBatch(rid, rng.integers(1, 4, n), np.zeros(n, np.uint8), np.full(n, 1000 + 10 * k, np.int64))
        t0 = time.perf_counter()
        e.request_tokens(b)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[warmup:]) * 1e3)


def check(n_flow):
    """Exact against the model on 2^18 requests of the generator."""
    from tests import concurrent_model as cm
    n, rng = 1 << 16, np.random.default_rng(7)
    ids, w, thr = flows(n_flow, n)
    e = engine.FlowEngine(abi.default_config(max_resources=4, max_batch=n))
    e.load_cluster_rules(flow=rules_of(ids, thr))
    m = cm.ConcurrentModel()
    m.load_rules([cm.Rule(int(f), float(c)) for f, c in zip(ids, thr)])
    prev, prev_m = None, None
    for k in range(4):
        b = gen_batch(rng, n, ids, w, prev, 1000 + k)
        got = e.request_concurrent(b)
        want = np.zeros(n, np.int8)
        mid = np.zeros(n, np.int64)
        back = dict(zip(prev.tolist(), prev_m.tolist())) if prev is not None else {}
        for i in range(n):
            if b.op[i] == abi.CC_ACQUIRE:
                want[i], mid[i] = m.acquire(int(b.id[i]), int(b.count[i]), int(b.client[i]), int(b.ts_ms[i]))
            else:
                want[i] = m.release(back.get(int(b.id[i]), 0))
        assert (got.status == want).all(), f"batch {k}: {(got.status != want).sum()} statuses differ"
        acq = b.op == abi.CC_ACQUIRE
        prev, prev_m = got.token_id[acq], mid[acq]
        assert e.concurrent_stats().live_tokens == len(m.tokens)
    for f in ids[:200].tolist() + ids[-50:].tolist():
        assert e.concurrent_now(f) == m.now_calls[f], f
    e.close()
    return 4 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--flows", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--tokens-only", action="store_true")
    ap.add_argument("--no-tokens", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ids, w, thr = flows(a.flows, a.n)
    e = engine.FlowEngine(abi.default_config(max_resources=4, max_batch=a.n))
    e.load_cluster_rules(flow=rules_of(ids, thr))
    res = {"requests_per_batch": a.n, "flow_ids": a.flows, "steps": a.steps}
    if not a.tokens_only:
        if a.check:
            res["checked_requests_exact"] = check(a.flows)
        e.concurrent_reserve(2 * a.n)
        ts, prev, mix = [], None, None
        for k in range(a.warmup + a.steps):
            b = gen_batch(rng, a.n, ids, w, prev, 1000 + k)
            t0 = time.perf_counter()
            got = e.request_concurrent(b)
            ts.append(time.perf_counter() - t0)
            prev = got.token_id[b.op == abi.CC_ACQUIRE]
            mix = {int(c): round(float((got.status == c).mean()), 4) for c in np.unique(got.status)}
        ms = float(np.median(ts[a.warmup:]) * 1e3)
        s = e.concurrent_stats()
        res.update(ms_per_batch=round(ms, 3), decisions_per_s=round(a.n / ms * 1e3), status_share_last_batch=mix,
                   chunks=s.chunks, chunks_all_pass=s.chunks_all_pass, rounds=s.rounds, live_tokens=s.live_tokens,
                   pool_capacity=s.pool_capacity, pool_grows=s.pool_grows)
    if not a.no_tokens:
        tms = time_tokens(e, ids, w, a.n, a.steps, a.warmup, rng)
        res.update(request_tokens_ms_per_batch=round(tms, 3), request_tokens_per_s=round(a.n / tms * 1e3))
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
