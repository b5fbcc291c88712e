"""Envoy rate-limit service front-end helpers: what a gRPC front-end does
before and after sf_request_rls.  It keeps gRPC and protobuf; the engine gets
the strings (or the flow ids) of a batch of RateLimitRequests.

Reference: sentinel-cluster/sentinel-cluster-server-envoy-rls (RLS below),
RLS/rule/EnvoyRlsRuleManager.java:85-98 and
RLS/rule/EnvoySentinelRuleConverter.java:53-74."""
import numpy as np

from . import abi, engine

SEPARATOR = "|"


def generate_key(domain, entries) -> str:
    """EnvoySentinelRuleConverter.generateKey: domain, then "|key|value" per entry."""
    return domain + "".join(SEPARATOR + k + SEPARATOR + v for k, v in entries)


def _utf8(s) -> bytes:
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8", "surrogatepass")


def pack_requests(requests, prehashed=False) -> abi.HostRlsBatch:
    """``requests``: (domain, [[(key, value), ...], ...], hits_addend, ts_ms)
    per RateLimitRequest, in arrival order; strings are str, or bytes for raw
    (possibly ill-formed) UTF-8.  prehashed=True hashes every key on the host
    (engine.rls_flow_id) and builds the flow-id form; every string must then
    be well-formed."""
    ts = [r[3] for r in requests]
    hits = [r[2] for r in requests]
    desc_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in requests])]).astype(np.uint32)
    if prehashed:
        fid = [engine.rls_flow_id(_utf8(r[0]) + b"".join(b"|" + _utf8(k) + b"|" + _utf8(v) for k, v in d))
               for r in requests for d in r[1]]
        return abi.HostRlsBatch(ts, hits, desc_off, desc_flow_id=np.asarray(fid, np.int64))
    index, chunks, str_off = {}, [], [0]

    def intern(s):
        raw = bytes(_utf8(s))
        i = index.get(raw)
        if i is None:
            i = index[raw] = len(chunks)
            chunks.append(raw)
            str_off.append(str_off[-1] + len(raw))
        return i

    domain = [intern(r[0]) for r in requests]
    ent_off, ent_key, ent_val = [0], [], []
    for r in requests:
        for d in r[1]:
            for k, v in d:
                ent_key.append(intern(k))
                ent_val.append(intern(v))
            ent_off.append(len(ent_key))
    return abi.HostRlsBatch(ts, hits, desc_off, domain=domain, ent_off=ent_off, ent_key=ent_key, ent_val=ent_val,
                            str_off=str_off, data=b"".join(chunks))


def rules_from_descriptors(domain, descriptors, namespace_id=0):
    """``descriptors``: ([(key, value), ...], count) per EnvoyRlsRule
    ResourceDescriptor.  Returns the sf_cluster_flow_rule list
    EnvoySentinelRuleConverter.toSentinelFlowRule makes: GLOBAL threshold,
    sampleCount 1, a 1000-ms window."""
    return [abi.sf_cluster_flow_rule(flow_id=engine.rls_flow_id(generate_key(domain, entries)), count=float(count),
                                     threshold_type=abi.THRESHOLD_GLOBAL, namespace_id=namespace_id, sample_count=1,
                                     window_interval_ms=1000)
            for entries, count in descriptors]
