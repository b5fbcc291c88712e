"""GPU parity of the cluster concurrency tokens (sf_request_concurrent,
sf_concurrent_expire) against the sequential model of the reference
(tests/concurrent_model.py): every status, the id translation, nowCalls of
every flowId and the live-token count after every batch.
Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from sentinel_amd import abi
from tests import concurrent_model as cm
from tests.test_concurrent_model import known_answer_batches

gpu = pytest.mark.gpu
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def eng_mod():
    from sentinel_amd import engine
    engine.lib()
    return engine


def model_of(rules, ns=(), cfg=()):
    m = cm.ConcurrentModel()
    m.load_namespaces(ns)
    m.load_config(cfg)
    m.load_rules(rules)
    return m


def load_engine_rules(e, rules, param_ids=()):
    e.load_cluster_rules(flow=[abi.sf_cluster_flow_rule(r.flow_id, r.count, r.threshold_type, r.namespace_id, 10, 1000)
                               for r in rules],
                         param=[abi.sf_cluster_param_rule(p, 5.0, abi.THRESHOLD_GLOBAL, 0, 10, 1000, 0, 0)
                                for p in param_ids])


def pair(eng_mod, rules, ns=(), cfg=(), param_ids=(), shard_count=1, shard_index=0):
    """An engine and a model loaded alike, behind one Replay."""
    e = eng_mod.FlowEngine(abi.default_config(max_resources=4, max_batch=1 << 12, shard_count=shard_count,
                                              shard_index=shard_index))
    e.load_namespaces([abi.sf_namespace(k, v, -1.0) for k, v in ns])
    load_engine_rules(e, rules, param_ids)
    if cfg:
        e.load_concurrent_config(cfg)
    return e, cm.Replay(model_of(rules, ns, cfg), e)


# ---------------------------------------------------------------- cases built on the CPU
def chunk_edges_case():
    """7 flowIds; flowId 101 has segments of 1, 63, 64, 65 and 197 requests (its
    acquires plus the releases that remove one of its tokens) over 5 batches;
    counts 1..3, thresholds 3..40, releases of earlier batches' tokens."""
    rng = np.random.default_rng(11)
    thr = {101: 40.0, 102: 3.0, 103: 7.0, 104: 12.0, 105: 20.0, 106: 33.0, 107: 40.0}
    rules = [cm.Rule(f, c) for f, c in thr.items()]
    rp = cm.Replay(model_of(rules))                           # a scratch model tells which tokens are held
    batches = []
    for k, seg in enumerate((1, 63, 64, 65, 197)):
        held = {}                                             # flowId -> request numbers holding a token
        for j, t in enumerate(rp.model_ids):
            if t in rp.model.tokens:
                held.setdefault(rp.model.tokens[t].flow_id, []).append(j)
        rows = []
        rel = held.get(101, [])[:min(len(held.get(101, [])), seg // 3)]
        rows += [(cm.R, j, 0, 0) for j in rel]
        rows += [(cm.A, 101, int(rng.integers(1, 4)), int(rng.integers(0, 4))) for _ in range(seg - len(rel))]
        for f in range(102, 108):
            rows += [(cm.R, j, 0, 0) for j in held.get(f, [])[::2]]
            rows += [(cm.A, f, int(rng.integers(1, 4)), int(rng.integers(0, 4))) for _ in range(int(rng.integers(5, 40)))]
        rows = [rows[i] for i in rng.permutation(len(rows))]
        b = cm.make_batch(rows, ts=1000 + k)
        rp.run(b)
        batches.append(b)
    return rules, batches


def coverage_case():
    """12 flowIds under skewed load, thresholds at about half the offered
    concurrency, 40 % releases with some repeated: every status is frequent and
    the hot flowIds' chunks mix passes, blocks and releases."""
    rng = np.random.default_rng(5)
    flow_ids = np.arange(201, 213)
    w = 1.0 / np.arange(1, 13) ** 1.1
    w /= w.sum()
    batch_n, n_batches = 3000, 6
    # offered concurrency of a flowId per batch: its acquires x mean count 2; the threshold is half of it
    rules = [cm.Rule(int(f), max(3.0, float(int(batch_n * 0.6 * p * 2 * 0.5)))) for f, p in zip(flow_ids, w)]
    batches = cm.random_stream(rng, flow_ids, n_batches, batch_n, release_share=0.4, dup_share=0.1, weights=w)
    return rules, batches


# ---------------------------------------------------------------- tests
@gpu
def test_known_answer(eng_mod):
    e, rp = pair(eng_mod, [cm.Rule(111, 10.0)])
    acquire, release = known_answer_batches()
    st, got = rp.run(acquire)
    assert got.status.tolist() == [cm.OK] * 10 + [cm.BLOCKED] * 10
    assert len(set(got.token_id[:10].tolist())) == 10 and (got.token_id[:10] != 0).all() and (got.token_id[10:] == 0).all()
    node = e.read_token(got.token_id[3])
    assert (node.flow_id, node.count, node.client, node.client_deadline_ms, node.resource_deadline_ms) == \
        (111, 1, 0, 3000, 3000)
    st, got = rp.run(release)
    assert got.status.tolist() == [cm.RELEASE_OK] * 10
    assert e.concurrent_now(111) == 0 and e.concurrent_stats().live_tokens == 0
    with pytest.raises(eng_mod.EngineError):
        e.read_token(rp.engine_ids[3])
    with pytest.raises(eng_mod.EngineError):
        e.concurrent_now(112)


@gpu
def test_chunk_edges(eng_mod):
    rules, batches = chunk_edges_case()
    e, rp = pair(eng_mod, rules)
    for b in batches:
        rp.run(b)
    st = np.array(rp.status)
    assert (st == cm.OK).any() and (st == cm.BLOCKED).any() and (st == cm.RELEASE_OK).any()
    assert e.concurrent_stats().chunks >= 9 + 6 * 5              # flowId 101: 1, 1, 1, 2 and 4 chunks; the others >= 1 a batch


@gpu
def test_buffers_regrow(eng_mod):
    """Batches of 3, 300 and 3 requests on one engine: the work set and the
    staging buffer are built, grown and reused by a smaller batch."""
    e, rp = pair(eng_mod, [cm.Rule(1, 120.0), cm.Rule(2, 7.0)])
    rng = np.random.default_rng(3)
    for k, n in enumerate((3, 300, 3)):
        rows = [(cm.A, int(rng.integers(1, 3)), int(rng.integers(1, 4)), int(rng.integers(0, 4))) for _ in range(n)]
        rp.run(cm.make_batch(rows, ts=1000 + k))
    st = np.array(rp.status)
    assert (st == cm.OK).sum() > 20 and (st == cm.BLOCKED).sum() > 20


@gpu
def test_malformed_releases(eng_mod):
    e, rp = pair(eng_mod, [cm.Rule(1, 100.0)])
    rp.run(cm.make_batch([(cm.A, 1, 1, 0)] * 4, ts=10))                      # requests 0..3 hold tokens
    never = (1 << 56) | (5 << 28) | 2                                       # a generation no slot has reached
    far = (1 << 56) | 0x0FFFFFFF                                            # a slot out of range
    st, got = rp.run(cm.make_batch([(cm.R, 0, 0, 0), (cm.R, 0, 0, 0), (cm.R, 0, 0, 0), (cm.X, never, 0, 0),
                                    (cm.X, far, 0, 0), (cm.X, 0, 0, 0), (cm.R, 1, 0, 0)], ts=11))
    assert got.status.tolist() == [cm.RELEASE_OK] + [cm.ALREADY_RELEASE] * 5 + [cm.RELEASE_OK]
    # a stale generation: the freed slots are used again, the old ids stay dead
    old = [rp.engine_ids[0], rp.engine_ids[1]]
    st, got = rp.run(cm.make_batch([(cm.A, 1, 1, 0)] * 2, ts=12))            # requests 11, 12
    slots = lambda ids: sorted(int(t) & 0x0FFFFFFF for t in ids)
    assert slots(got.token_id) == slots(old) and not set(got.token_id.tolist()) & set(old)
    st, got = rp.run(cm.make_batch([(cm.R, 0, 0, 0), (cm.R, 1, 0, 0), (cm.R, 11, 0, 0)], ts=13))
    assert got.status.tolist() == [cm.ALREADY_RELEASE, cm.ALREADY_RELEASE, cm.RELEASE_OK]


@gpu
def test_request_validation(eng_mod):
    e, rp = pair(eng_mod, [cm.Rule(1, 100.0)], param_ids=[9])
    st, got = rp.run(cm.make_batch([(cm.A, 1, 1, cm.CLIENT_NONE), (cm.A, 0, 1, 0), (cm.A, -5, 1, 0), (cm.A, 1, 0, 0),
                                    (cm.A, 1, -1, 0), (cm.A, 9, 1, 0), (cm.A, 77, 1, 0), (cm.A, 1, 1, 0)], ts=5))
    assert got.status.tolist() == [cm.BAD_REQUEST] * 5 + [cm.NO_RULE_EXISTS] * 2 + [cm.OK]


@gpu
def test_coverage_stream(eng_mod):
    rules, batches = coverage_case()
    e, rp = pair(eng_mod, rules)
    for b in batches:
        rp.run(b)
    st = np.array(rp.status)                                      # the model's results
    for code in (cm.OK, cm.BLOCKED, cm.RELEASE_OK, cm.ALREADY_RELEASE):
        assert (st == code).mean() >= 0.05, code
    s = e.concurrent_stats()
    assert s.chunks_all_pass < s.chunks and s.rounds > s.chunks, (s.chunks, s.chunks_all_pass, s.rounds)


@gpu
def test_thresholds(eng_mod):
    rules = [cm.Rule(1, 4.0, cm.AVG_LOCAL, 7), cm.Rule(2, 4.0, cm.AVG_LOCAL, 8), cm.Rule(3, 1e12)]
    e, rp = pair(eng_mod, rules, ns=[(7, 3)])
    st, got = rp.run(cm.make_batch([(cm.A, 1, 5, 0)] * 3 + [(cm.A, 2, 1, 0)] * 3, ts=1))
    assert got.status.tolist() == [cm.OK, cm.OK, cm.BLOCKED] + [cm.BLOCKED] * 3       # 4 * 3 = 12; namespace 8: 0
    # Java int: INT32_MAX + 1 wraps to INT32_MIN, which is not > 1e12
    st, got = rp.run(cm.make_batch([(cm.A, 3, INT32_MAX, 0), (cm.A, 3, 1, 0), (cm.A, 3, 1, 0)], ts=2))
    assert got.status.tolist() == [cm.OK] * 3 and e.concurrent_now(3) == -2 ** 31 + 1


@gpu
def test_reload(eng_mod):
    a, b_ = cm.Rule(1, 10.0), cm.Rule(2, 10.0)
    e, rp = pair(eng_mod, [a, b_])
    rp.run(cm.make_batch([(cm.A, 1, 2, 0), (cm.A, 2, 3, 0), (cm.A, 1, 1, 0)], ts=1))
    for rules in ([a], [a, b_]):
        load_engine_rules(e, rules)
        rp.model.load_rules(rules)
        rp.check_state()
        if len(rules) == 1:
            assert e.concurrent_now(1) == 3
            st, got = rp.run(cm.make_batch([(cm.R, 1, 0, 0), (cm.R, 1, 0, 0)], ts=2))
            assert got.status.tolist() == [cm.NO_RULE_EXISTS] * 2 and e.concurrent_stats().live_tokens == 3
    assert e.concurrent_now(2) == 0
    st, got = rp.run(cm.make_batch([(cm.R, 1, 0, 0)], ts=3))
    assert got.status.tolist() == [cm.RELEASE_OK] and e.concurrent_now(2) == -3


@gpu
def test_expiry(eng_mod):
    rules = [cm.Rule(1, 100.0), cm.Rule(2, 100.0)]
    cfg = [(1, 500, 1000), (2, 500, 1000)]
    e, rp = pair(eng_mod, rules, cfg=cfg)
    # request 0: client 0 goes offline; 1: online, old; 2: online, fresh (acquired late); 3: its rule goes, online
    rp.run(cm.make_batch([(cm.A, 1, 1, 0, 1000), (cm.A, 1, 2, 1, 1000), (cm.A, 2, 4, 1, 1000)]))
    rp.run(cm.make_batch([(cm.A, 1, 3, 1, 2400)]))
    load_engine_rules(e, rules[:1])
    rp.model.load_rules(rules[:1])
    assert rp.expire(1900, online_clients=[0, 1], n_clients=2) == 0       # 1900 - 1500 is not > 500
    # 2500: client 0 is offline and past 1000 + 1000; request 1 is past 1500 + 500; request 3 is fresh
    # (2500 - 2900 < 0); request 2 has no rule and an online client
    assert rp.expire(2500, online_clients=[1], n_clients=2) == 2
    assert e.concurrent_now(1) == 3 and e.concurrent_stats().live_tokens == 2
    for j, live in enumerate((False, False, True, True)):
        if live:
            e.read_token(rp.engine_ids[j])
        else:
            with pytest.raises(eng_mod.EngineError):
                e.read_token(rp.engine_ids[j])
    # a time-out changed after the acquire applies to the second term only: the stored deadline stays
    # 2400 + 500 = 2900, and 2950 - 2900 = 50 > 40
    e.load_concurrent_config([(1, 40, 1000)])
    rp.model.load_config([(1, 40, 1000)])
    assert e.read_token(rp.engine_ids[3]).resource_deadline_ms == 2900
    assert rp.expire(2950, online_clients=[1], n_clients=2) == 1
    assert e.concurrent_stats().expired == 3
    # the client-offline branch still removes the token whose rule is gone
    assert rp.expire(2950, online_clients=[], n_clients=2) == 1
    assert e.concurrent_stats().live_tokens == 0
    with pytest.raises(eng_mod.EngineError):
        e.load_concurrent_config([(1, 0, 1000)])


@gpu
def test_pool_growth(eng_mod):
    e, rp = pair(eng_mod, [cm.Rule(1, 1e6)])
    e.concurrent_reserve(64)
    assert e.concurrent_stats().pool_capacity == 64
    for k in range(10):
        rp.run(cm.make_batch([(cm.A, 1, 1, 0)] * 100, ts=k))
    s = e.concurrent_stats()
    assert s.pool_grows > 0 and s.live_tokens == 1000 and s.pool_capacity >= 1000
    st, got = rp.run(cm.make_batch([(cm.R, j, 0, 0) for j in range(1000)], ts=20))
    assert (got.status == cm.RELEASE_OK).all() and e.concurrent_now(1) == 0


@gpu
def test_two_shards(eng_mod):
    rules = [cm.Rule(10, 5.0), cm.Rule(11, 5.0)]                  # owners: flow_id % 2
    ids = {}
    for shard in (0, 1):
        e, rp = pair(eng_mod, rules, shard_count=2, shard_index=shard)
        st, got = rp.run(cm.make_batch([(cm.A, 10 + shard, 1, 0)] * 2, ts=1))
        assert [abi.token_id_shard(t) for t in got.token_id] == [shard, shard]
        ids[shard] = int(got.token_id[0])
        with pytest.raises(eng_mod.EngineError) as ei:
            e.request_concurrent(abi.HostConcurrentBatch([abi.CC_ACQUIRE], [10 + (1 - shard)], [1], [0], [2]))
        assert ei.value.code == abi.SF_ERR_INVALID
        if shard == 1:
            with pytest.raises(eng_mod.EngineError) as ei:
                e.request_concurrent(abi.HostConcurrentBatch([abi.CC_RELEASE], [ids[0]], [0], [0], [3]))
            assert ei.value.code == abi.SF_ERR_INVALID
            st, got = rp.run(cm.make_batch([(cm.R, 0, 0, 0)], ts=4))
            assert got.status.tolist() == [cm.RELEASE_OK]
