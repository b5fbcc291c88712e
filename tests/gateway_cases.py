"""Border workloads of the API-gateway flow rules (sf_load_gateway_rules,
sf_gateway_args), shared by the CPU checks (tests/test_gateway_model.py: each
workload sits on its borders, judged from the model and the oracle alone) and
the GPU parity suite (tests/test_gpu_gateway.py).

A case: rules (gateway.GatewayRule, in Set iteration order), prules / items
(ordinary ParamFlowRules), and batches of requests, in-batch exits, late exits
(of an entry of an earlier batch) and unrelated events.  build() lays every
batch out (gateway.layout), and computes with the model (tests/gateway_model.py)
the columns sf_gateway_args must produce and the rule list of the oracle."""
import numpy as np

from sentinel_amd import abi, gateway as gw, trace
from tests import gateway_model as gm

T0 = trace.T0
ROUTE, API = gw.RESOURCE_MODE_ROUTE_ID, gw.RESOURCE_MODE_CUSTOM_API_NAME
R = 16                                   # resources of every case
LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65)
EXACT_P = "abcdefgh"                      # L = 8: values of 7, 8 and 9 bytes around it
UTF_P = "é€\U0001F600"          # a 2-, a 3- and a 4-byte sequence


def item(parse, name=None, pattern=None, match=gw.MATCH_EXACT):
    return gw.ParamItem(parse, name, pattern, match)


def rule(res, name=None, **kw):
    return gw.GatewayRule(res, name or f"route_{res}", **kw)


def req(ts, entries, **kw):
    return dict(ts_ms=T0 + ts, entries=list(entries), **kw)


# ---- strings: every length and match border on one resource ----------------------------------
STR_HEADER = ["abcdefg", EXACT_P, "abcdefghi", "$NM", "", "Abcdefgh"]
STR_PARAM = ["aabxx", "xxaab", "aaab", "aa", "xaaxb", "aab", "ab"]      # CONTAINS "aab": first / last position, overlap, too short
STR_COOKIE = ["x" * n if n != 3 else "$NM" for n in LENGTHS]            # no pattern: the value as is (a literal "$NM" too)
STR_HOST = ["x" + UTF_P + "y", UTF_P, "é€\U0001F601", "è€\U0001F600", "é€", "y" + UTF_P,
            "é₭\U0001F600"]


def strings(seed=5, n=420):
    rules = [rule(0, count=5, item=item(gw.PARSE_HEADER, "h", EXACT_P, gw.MATCH_EXACT)),
             rule(0, count=4, item=item(gw.PARSE_URL_PARAM, "p", "aab", gw.MATCH_CONTAINS)),
             rule(0, count=3, burst=1, item=item(gw.PARSE_COOKIE, "c")),
             rule(0, count=6, item=item(gw.PARSE_HOST, None, UTF_P, gw.MATCH_CONTAINS))]
    rng = np.random.default_rng(seed)
    most = max(len(STR_HEADER), len(STR_PARAM), len(STR_COOKIE), len(STR_HOST))
    reqs = []
    for k in range(n):
        pick = (lambda pool: pool[k % len(pool)]) if k < most else (lambda pool: pool[int(rng.integers(0, len(pool)))])
        reqs.append(req(k * 2, [(0, ROUTE)], headers={"h": pick(STR_HEADER)}, params={"p": pick(STR_PARAM)},
                        cookies={"c": pick(STR_COOKIE)}, host=pick(STR_HOST)))
    # the last string of the table: a value no request had before, matched at its last bytes
    reqs.append(req(n * 2, [(0, ROUTE)], headers={"h": EXACT_P}, params={"p": "last_value_aab"}, cookies={"c": "x"},
                    host=UTF_P))
    return dict(name="strings", rules=rules, batches=[dict(requests=reqs)], item_rules={0: [0, 1, 2, 3]})


# ---- rules: every row of the semantics table ---------------------------------------------------
def rule_rows(seed=6):
    rng = np.random.default_rng(seed)
    rules = [
        # 1: only rules without item, one of them a CUSTOM_API_NAME rule: "$D" whatever the entry's mode
        rule(1, count=3), rule(1, count=5, resource_mode=API, control_behavior=2, max_queueing_timeout_ms=100),
        # 2: item rules of two modes (predSet has both): no entry gets arguments, the rule without item passes too
        rule(2, count=1, item=item(gw.PARSE_CLIENT_IP)), rule(2, count=1, resource_mode=API, item=item(gw.PARSE_HOST)),
        rule(2, count=1),
        # 3: one route-mode item rule: an API-mode entry gets no arguments
        rule(3, count=2, item=item(gw.PARSE_HEADER, "h", "Wow", gw.MATCH_EXACT)),
        # 4: PREFIX and strategy 7 always give the value; parse strategy 9 gives null
        rule(4, count=2, item=item(gw.PARSE_HEADER, "h", "ab", gw.MATCH_PREFIX)),
        rule(4, count=3, item=item(gw.PARSE_URL_PARAM, "p", "zz", 7)),
        rule(4, count=1, item=item(9, None)),
        # 5: a null pattern against an empty one (the empty one still has the "$NM" hot item)
        rule(5, count=2, item=item(gw.PARSE_HEADER, "h")), rule(5, count=3, item=item(gw.PARSE_HEADER, "h2", "")),
        # 6: two regex rules on one URL parameter: two field ids, two flags
        rule(6, count=2, resource_mode=API, item=item(gw.PARSE_URL_PARAM, "p", r"\d+", gw.MATCH_REGEX)),
        rule(6, count=3, resource_mode=API, item=item(gw.PARSE_URL_PARAM, "p", r"[a-z0-9]+", gw.MATCH_REGEX)),
        # 7: a gateway item rule, a rule without item and (below) an ordinary param rule on slot 0
        rule(7, count=4, item=item(gw.PARSE_CLIENT_IP)), rule(7, count=9),
        # 9: RATE_LIMITER with burst and a 2 s interval
        rule(9, count=8, interval_sec=2, burst=3, control_behavior=2, max_queueing_timeout_ms=300,
             item=item(gw.PARSE_COOKIE, "c")),
        # 11: a rule ParamFlowRuleUtil.isValidRule drops (it keeps slot 0), beside a valid one on slot 1
        rule(11, count=1, max_queueing_timeout_ms=-1, item=item(gw.PARSE_CLIENT_IP)),
        rule(11, count=2, item=item(gw.PARSE_HEADER, "h")),
        # invalid rules: dropped, no slot
        rule(11, count=-1.0, item=item(gw.PARSE_HOST)), rule(12, count=1, item=item(gw.PARSE_COOKIE, " ")),
        rule(12, count=1, interval_sec=0),
    ]
    hot_ip = "10.0.0.1"
    prules = [abi.sf_param_rule(resource=7, grade=abi.GRADE_QPS, param_idx=0, count=6.0, duration_in_sec=1,
                                item_offset=0, item_count=1)]
    items = [abi.sf_hot_item(tag=abi.TAG_STRING, count=1, bits=gm.bits_of(hot_ip))]
    ips = [hot_ip, "10.0.0.2", "10.0.0.3"]
    hs = ["Wow", "Wow_foo", "abx", "zz", "q"]
    ps = ["23", "some233", "abc", "ABC", "zzz"]
    reqs = []
    for k in range(700):
        u = int(rng.integers(0, 12))
        kw = dict(client_ip=ips[int(rng.integers(0, 3))], host="h.test", headers={"h": hs[int(rng.integers(0, 5))]},
                  params={"p": ps[int(rng.integers(0, 5))]}, cookies={"c": "ck%d" % rng.integers(0, 2)})
        if rng.random() < 0.3:
            kw["headers"]["h2"] = hs[int(rng.integers(0, 5))]
        if u == 0:
            kw = {}                                            # a request without values
        if u == 1:
            kw.pop("client_ip")
        if u == 2:                                             # four entries: a route and three API names
            ent = [(3, ROUTE), (6, API), (7, ROUTE), (10, ROUTE)]
        else:
            r = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12]))
            ent = [(r, API if (r == 6 or rng.random() < 0.25) else ROUTE)]
        reqs.append(req(k * 3, ent, count=int(rng.integers(1, 3)),
                        flags=abi.EV_IN | (abi.EV_PRIO if rng.random() < 0.1 else 0), **kw))
    return dict(name="rule_rows", rules=rules, prules=prules, items=items, batches=[dict(requests=reqs)],
                item_rules={3: [0], 4: [0, 1], 5: [0, 1], 6: [0, 1], 7: [0], 9: [0]})


# ---- THREAD grade: exits of this batch through exit_pos, exits one batch later ----------------
def threads(seed=7):
    rng = np.random.default_rng(seed)
    rules = [rule(8, grade=abi.GRADE_THREAD, count=2, item=item(gw.PARSE_CLIENT_IP)),
             rule(8, grade=abi.GRADE_THREAD, count=5)]
    ips = ["1.1.1.1", "2.2.2.2", "3.3.3.3"]
    b0, b1, exits0, late = [], [], [], []
    for k in range(240):
        b0.append(req(k * 4, [(8, ROUTE)], client_ip=ips[int(rng.integers(0, 3))]))
        u = rng.random()
        if u < 0.8:
            exits0.append((T0 + k * 4 + int(rng.integers(1, 9)), k, 0, abi.EV_ERROR if rng.random() < 0.2 else 0))
        elif u < 0.9:
            late.append((T0 + 1000 + int(rng.integers(0, 400)), 0, k, 0))
    for k in range(160):
        b1.append(req(1000 + k * 3, [(8, ROUTE)], client_ip=ips[int(rng.integers(0, 3))]))
    # (resource, paramIdx, tag, bits) whose thread count is compared after every batch
    touched = [(8, 0, abi.TAG_STRING, gm.bits_of(ip)) for ip in ips] + [(8, 1, abi.TAG_STRING, gm.bits_of(gm.D))]
    return dict(name="threads", rules=rules, batches=[dict(requests=b0, exits=exits0), dict(requests=b1, late=late)],
                item_rules={8: [0]}, touched=touched)


# ---- layout: request counts around the block size, gaps, duplicates -----------------------------
LAYOUT_N = (0, 1, 63, 64, 65, 257)


def layout(n, seed=8):
    rng = np.random.default_rng(seed + n)
    rules = [rule(0, count=3, item=item(gw.PARSE_CLIENT_IP)),
             rule(0, count=4, item=item(gw.PARSE_HEADER, "h", "Wow", gw.MATCH_EXACT)),
             rule(0, count=5, item=item(gw.PARSE_COOKIE, "c", "ar", gw.MATCH_CONTAINS)),
             rule(1, count=2, resource_mode=API), rule(2, count=2, resource_mode=API, item=item(gw.PARSE_CLIENT_IP)),
             rule(3, count=3, resource_mode=API, item=item(gw.PARSE_HOST))]
    reqs, extra = [], []
    for k in range(n):
        kw = dict(client_ip="9.9.9.%d" % rng.integers(0, 3), host="host%d" % rng.integers(0, 2),
                  headers={"h": ["Wow", "wow"][int(rng.integers(0, 2))]}, cookies={"c": ["bar", "baz"][int(rng.integers(0, 2))]})
        if k % 7 == 3:
            kw = {}
        ent = [(0, ROUTE), (1, API), (2, API), (3, API)] if k % 5 == 0 else [(0, ROUTE)]
        reqs.append(req(k * 5, ent, **kw))
    for k in range(max(3, n // 3)):                              # unrelated events in the gaps, with arguments of their own
        extra.append(dict(ts_ms=T0 + k * 13 + 1, res_id=13, count=1, flags=abi.EV_IN, n_args=1,
                          arg_tag=[abi.TAG_LONG, 0, 0, 0], arg_bits=[k % 4, 0, 0, 0]))
    prules = [abi.sf_param_rule(resource=13, grade=abi.GRADE_QPS, param_idx=0, count=2.0, duration_in_sec=1)]
    return dict(name=f"layout{n}", rules=rules, prules=prules, batches=[dict(requests=reqs, extra=extra)],
                item_rules={0: [0, 1, 2]} if n >= 257 else {})


def build(case):
    """table, converted model, per batch (HostGatewayBatch, HostGatewayEvents as given to the engine, the model's
    columns, create_ts), the oracle's rules and the workload dict of workloads.run."""
    table = gw.RuleTable(case["rules"])
    conv = gm.Converted(case["rules"])
    built = []
    for b in case["batches"]:
        extra = list(b.get("extra", ()))
        for ts, j, qi, k in b.get("late", ()):                 # the EXIT of an entry of batch j: its arguments were kept
            hb, _, want, _ = built[j]
            p = int(hb.ev_index[qi]) + k
            extra.append(dict(ts_ms=ts, res_id=int(want.res_id[p]), count=int(want.count[p]), flags=abi.EV_EXIT | abi.EV_IN,
                              create_ts=int(want.ts_ms[p]), n_args=int(want.n_args[p]), arg_tag=want.arg_tag[:, p].copy(),
                              arg_bits=want.arg_bits[:, p].copy()))
        hb, ev, create_ts = gw.layout(table, b["requests"], b.get("exits", ()), extra)
        want = gm.columns(conv, b["requests"], hb.ev_index, ev)
        built.append((hb, ev, want, create_ts))
    prules, items = gm.combined_rules(conv, case.get("prules", ()), case.get("items", ()))
    n_max = max([16] + [ev.n_total for _, ev, _, _ in built])
    w = dict(cfg=abi.default_config(max_resources=R, max_batch=n_max, param_capacity=1 << 12), param=prules, items=items,
             batches=[want.batch(ct) for _, _, want, ct in built], nodes=list(range(R)))
    return dict(table=table, conv=conv, built=built, w=w, case=case)


def duplicate_field(hb: abi.HostGatewayBatch):
    """hb with a second item of an already present field id appended to every
    request that has values: the first one must still be used."""
    arr = {name: getattr(hb, name) for name in hb.ARRAYS}
    strings = [bytes(hb.data[hb.str_off[k]:hb.str_off[k + 1]]) for k in range(hb.n_str)] + [b"duplicate!"]
    vf, vs, vl, off = [], [], [], [0]
    for i in range(hb.n):
        lo, hi = int(hb.val_off[i]), int(hb.val_off[i + 1])
        vf += list(hb.val_field[lo:hi]); vs += list(hb.val_str[lo:hi]); vl += list(hb.val_flags[lo:hi])
        if hi > lo:
            vf.append(int(hb.val_field[lo])); vs.append(hb.n_str); vl.append(abi.GW_NOMATCH)
        off.append(len(vf))
    arr["str_off"], arr["data"] = abi.string_table(strings)
    arr.update(val_off=off, val_field=vf, val_str=vs, val_flags=vl)
    return abi.HostGatewayBatch(**arr)


def distinct_bits(built):
    """Within a case distinct strings have distinct bits (the declared divergence does not occur)."""
    seen = {}
    for hb, _, _, _ in built:
        for k in range(hb.n_str):
            s = bytes(hb.data[hb.str_off[k]:hb.str_off[k + 1]])
            assert seen.setdefault(gm.fnv(s), s) == s, (s, seen[gm.fnv(s)])
    for s in (b"$NM", b"$D"):
        assert seen.setdefault(gm.fnv(s), s) == s


def guard_decisions(built, outs):
    """From the oracle's verdicts: the rule of every listed item slot of the
    listed resources blocks some entry, entries of the resource pass, and some
    entry is blocked by a later rule after an earlier one consumed.  outs: the
    oracle's HostVerdicts per batch."""
    case, conv = built["case"], built["conv"]
    later = False
    for res, slots in case["item_rules"].items():
        lst = [p for p in conv.prules if p.resource == res]
        want = {k for k, p in enumerate(lst) if p.param_idx in slots}
        assert len(want) == len(slots)
        blocked, passed = set(), 0
        for b, v in zip(built["w"]["batches"], outs):
            sel = (b.res_id == res) & ((b.flags & abi.EV_EXIT) == 0)
            passed += int(np.isin(v.status[sel], abi.PASSED).sum())
            blocked |= set(int(x) for x in v.rule_idx[sel & (v.status == abi.V_BLOCK_PARAM)])
        assert passed, f"{case['name']}: no entry of resource {res} passes"
        assert want <= blocked, f"{case['name']}: resource {res}: rules {sorted(want - blocked)} never block"
        later |= any(k > 0 for k in blocked)
    assert later or not case["item_rules"], f"{case['name']}: no entry is blocked by a later rule"
