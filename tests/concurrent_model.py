"""TEST-ONLY: a sequential restatement of the reference's cluster concurrency
tokens, and a driver that replays one op stream on it and on the engine.

Reference (CS = sentinel-cluster/sentinel-cluster-server-default/src/main/java/
com/alibaba/csp/sentinel/cluster):
  DefaultTokenService.requestConcurrentToken      CS/flow/DefaultTokenService.java:66-93
  ConcurrentClusterFlowChecker                    CS/flow/ConcurrentClusterFlowChecker.java:36-101
  ClusterFlowRuleManager.applyClusterFlowRule     CS/flow/rule/ClusterFlowRuleManager.java:271-375
  RegularExpireStrategy.clearToken                CS/flow/statistic/concurrent/expire/RegularExpireStrategy.java:94-136
  FlowRuleUtil (time-outs > 0)                    sentinel-core .../flow/FlowRuleUtil.java:195

Declared divergences: the model issues its own ids (the
reference draws UUIDs); the sweep looks at every live token (the reference at
1000 keys for 800 ms); a token whose rule is gone is kept by the resource
time-out check (the reference throws there and ends the run) while the
client-offline check still removes it; the clock is the request's ts_ms and
the sweep's now_ms.
"""
from dataclasses import dataclass

import numpy as np

OK, BLOCKED, NO_RULE_EXISTS, BAD_REQUEST, RELEASE_OK, ALREADY_RELEASE = 0, 1, 3, -4, 6, 7
AVG_LOCAL, GLOBAL = 0, 1        # ClusterRuleConstant.FLOW_THRESHOLD_*
CLIENT_NONE = 0xFFFFFFFF
DEFAULT_TIMEOUT = 2000          # ClusterFlowConfig: resourceTimeout, clientOfflineTime


def jint(v: int) -> int:
    """Java int: wrap to 32 bits."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


@dataclass
class Rule:
    flow_id: int
    count: float
    threshold_type: int = GLOBAL
    namespace_id: int = 0


@dataclass
class Node:                      # TokenCacheNode
    flow_id: int
    count: int
    client: int
    client_deadline: int
    resource_deadline: int


class ConcurrentModel:
    def __init__(self):
        self.rules = {}          # flowId -> Rule (ClusterFlowRuleManager.FLOW_RULES)
        self.connected = {}      # namespace id -> ConnectionManager.getConnectedCount
        self.cfg = {}            # flowId -> (resourceTimeout, clientOfflineTime)
        self.now_calls = {}      # CurrentConcurrencyManager
        self.tokens = {}         # TokenCacheNodeManager
        self.next_id = 1

    def load_namespaces(self, ns):
        self.connected = {int(k): int(v) for k, v in ns}

    def load_config(self, cfg):
        for _, rt, cot in cfg:
            assert rt > 0 and cot > 0                            # FlowRuleUtil.java:195
        self.cfg = {int(f): (int(rt), int(cot)) for f, rt, cot in cfg}

    def load_rules(self, rules):
        """applyClusterFlowRule :271-375: nowCalls of a flowId that stays loaded
        is kept, of one that goes is dropped; stored tokens are untouched."""
        new = {}
        for r in rules:
            if r.flow_id > 0:
                new.setdefault(r.flow_id, r)
        self.now_calls = {f: self.now_calls.get(f, 0) for f in new}
        self.rules = new

    def threshold(self, r: Rule) -> float:                       # calcGlobalThreshold :36-46
        if r.threshold_type == GLOBAL:
            return float(r.count)
        return float(r.count) * self.connected.get(r.namespace_id, 0)

    def timeouts(self, flow_id):
        return self.cfg.get(flow_id, (DEFAULT_TIMEOUT, DEFAULT_TIMEOUT))

    def acquire(self, flow_id, count, client, ts):
        if client == CLIENT_NONE or flow_id <= 0 or count <= 0:  # notValidRequest :91-93
            return BAD_REQUEST, 0
        r = self.rules.get(flow_id)
        if r is None:                                            # :72-75
            return NO_RULE_EXISTS, 0
        if jint(self.now_calls[flow_id] + count) > self.threshold(r):     # :57-68, int + int > double
            return BLOCKED, 0
        self.now_calls[flow_id] = jint(self.now_calls[flow_id] + count)   # :70
        rt, cot = self.timeouts(flow_id)
        tid = self.next_id
        self.next_id += 1
        self.tokens[tid] = Node(flow_id, count, client, ts + cot, ts + rt)   # generateTokenCacheNode :74-75
        return OK, tid

    def release(self, tid):
        node = self.tokens.get(tid)
        if node is None:                                         # :82-86
            return ALREADY_RELEASE
        if node.flow_id not in self.rules:                       # :87-91 (the token stays)
            return NO_RULE_EXISTS
        del self.tokens[tid]
        self.now_calls[node.flow_id] = jint(self.now_calls[node.flow_id] - node.count)   # :96-98
        return RELEASE_OK

    def expire(self, now, online) -> int:
        """clearToken :94-136 over every live token; online: set of client ids."""
        removed = 0
        for tid in list(self.tokens):
            node = self.tokens[tid]
            rm = node.client not in online and node.client_deadline - now < 0       # :110-114
            if not rm and node.flow_id in self.rules:                                # :118-122 (rule gone: kept)
                rm = now - node.resource_deadline > self.timeouts(node.flow_id)[0]
            if rm:
                del self.tokens[tid]                                                 # removeToken :126-136
                if node.flow_id in self.now_calls:
                    self.now_calls[node.flow_id] = jint(self.now_calls[node.flow_id] - node.count)
                removed += 1
        return removed


# ---------------------------------------------------------------- op streams
# One request: kind A (acquire), R (release the token of request #ref of the
# whole stream; id 0 if that request got none) or X (release of the raw id
# `ref`, the same number on both sides).
A, R, X = 0, 1, 2


@dataclass
class Batch:
    kind: np.ndarray             # [n] A / R / X
    ref: np.ndarray              # [n] A: flow id; R: request number; X: raw token id
    count: np.ndarray            # [n]
    client: np.ndarray           # [n]
    ts: np.ndarray               # [n]

    @property
    def n(self):
        return len(self.kind)


def make_batch(rows, ts=0):
    """rows: (kind, ref, count, client) or (kind, ref, count, client, ts)."""
    rows = [tuple(r) + (ts,) if len(r) == 4 else tuple(r) for r in rows]
    k, ref, c, cl, t = zip(*rows) if rows else ((), (), (), (), ())
    return Batch(np.array(k, np.int64), np.array(ref, np.int64), np.array(c, np.int64), np.array(cl, np.int64),
                 np.array(t, np.int64))


class Replay:
    """Feeds batches to the model and (when given) the engine and compares
    every status, the id translation, nowCalls of every flowId and the
    live-token count after every batch."""

    def __init__(self, model: ConcurrentModel, engine=None):
        self.model, self.engine = model, engine
        self.model_ids, self.engine_ids = [], []     # per request number: the token it got, or 0
        self.status = []                             # model statuses of the whole stream

    def run(self, b: Batch):
        m = self.model
        st = np.zeros(b.n, np.int8)
        base = len(self.model_ids)
        ids = [0] * b.n
        for i in range(b.n):
            k, ref = int(b.kind[i]), int(b.ref[i])
            if k == A:
                st[i], ids[i] = m.acquire(ref, int(b.count[i]), int(b.client[i]), int(b.ts[i]))
            else:
                assert k == X or ref < base, "a release names a token of an earlier call"
                st[i] = m.release(self.model_ids[ref] if k == R else ref)
        self.model_ids += ids
        self.status += st.tolist()
        if self.engine is None:
            self.engine_ids += [0] * b.n
            return st, None
        from sentinel_amd import abi
        eid = np.array([ref if k == A else (self.engine_ids[ref] if k == R else ref)
                        for k, ref in zip(b.kind.tolist(), b.ref.tolist())], np.int64)
        hb = abi.HostConcurrentBatch(np.where(b.kind == A, abi.CC_ACQUIRE, abi.CC_RELEASE), eid, b.count, b.client, b.ts)
        got = self.engine.request_concurrent(hb)
        self.engine_ids += got.token_id.tolist()
        bad = np.nonzero(got.status != st)[0]
        assert bad.size == 0, f"status differs at {bad[:8]}: got {got.status[bad[:8]]} want {st[bad[:8]]}"
        assert ((got.token_id != 0) == (st == OK)).all(), "token_id is non-zero exactly for an OK acquire"
        self.check_state()
        return st, got

    def check_state(self):
        live = [t for t in self.engine_ids if t != 0]
        assert len(set(live)) == len(live), "token ids are distinct"
        for f, want in self.model.now_calls.items():
            assert self.engine.concurrent_now(f) == want, f"nowCalls of flowId {f}"
        assert self.engine.concurrent_stats().live_tokens == len(self.model.tokens)

    def expire(self, now, online_clients, n_clients):
        want = self.model.expire(now, set(online_clients))
        if self.engine is not None:
            on = np.zeros(n_clients, np.uint8)
            on[np.array(list(online_clients), np.int64)] = 1
            assert self.engine.concurrent_expire(now, on) == want
            self.check_state()
        return want


def random_stream(rng, flow_ids, n_batches, batch_n, release_share=0.4, dup_share=0.05, counts=(1, 3), weights=None,
                  n_clients=8, ts0=1000):
    """Batches of acquires on `flow_ids` (drawn with `weights`) and releases of
    earlier batches' requests: of requests not yet released by the stream (so
    most hold a token if they passed), with some repeated (`dup_share`)."""
    out, pool, done, base = [], [], [], 0
    for k in range(n_batches):
        kind = np.full(batch_n, A, np.int64)
        ref = rng.choice(flow_ids, batch_n, p=weights).astype(np.int64)
        n_rel = min(int(batch_n * release_share), len(pool)) if pool else 0
        pos = np.sort(rng.choice(batch_n, n_rel, replace=False)) if n_rel else np.zeros(0, np.int64)
        take = rng.permutation(len(pool))[:n_rel]
        targets = [pool[j] for j in take]
        n_dup = int(n_rel * dup_share)
        if n_dup and (done or targets):
            src = done + targets
            for q in rng.choice(n_rel, n_dup, replace=False):
                targets[q] = src[int(rng.integers(len(src)))]
        kind[pos] = R
        ref[pos] = targets
        keep = set(range(len(pool))) - set(take.tolist())
        done += [pool[j] for j in take]
        pool = [pool[j] for j in sorted(keep)] + [base + i for i in range(batch_n) if kind[i] == A]
        out.append(Batch(kind, ref, rng.integers(counts[0], counts[1] + 1, batch_n).astype(np.int64),
                         rng.integers(0, n_clients, batch_n).astype(np.int64),
                         np.full(batch_n, ts0 + k, np.int64)))
        base += batch_n
    return out
