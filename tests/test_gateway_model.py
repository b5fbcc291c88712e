"""API-gateway flow rules on the CPU: the model (tests/gateway_model.py) pinned
to the reference's own test cases, restated as inputs and expected values;
sf_gateway_convert (host only) against the model on those cases and on seeded
random rule sets; the engine's host-compilable parser code
(sentinel_amd/csrc/sf_gateway.h) against the model in a stand-alone program
under ASan + UBSan (tests/gateway_check.cpp); and the guards of every GPU
workload (tests/gateway_cases.py) on the model and the oracle alone.  Reference
tests are under sentinel-adapter/sentinel-api-gateway-adapter-common/src/test/
java/com/alibaba/csp/sentinel/adapter/gateway/common/."""
import os
import subprocess

import numpy as np
import pytest

from sentinel_amd import abi, gateway as gw
from tests import gateway_cases as gc
from tests import gateway_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
ROUTE, API = gw.RESOURCE_MODE_ROUTE_ID, gw.RESOURCE_MODE_CUSTOM_API_NAME
G, I = gw.GatewayRule, gw.ParamItem


# ---- known answers -------------------------------------------------------------------------------
def test_constants():
    assert gm.bits_of("") == 0xcbf29ce484222325 and gm.bits_of("a") == 0xaf63dc4c8601ec8c      # FNV-1a 64 test vectors
    assert gm.ro.java_string_hash("$NM") == 37091
    assert gm.ro.java_string_hash("java.lang.String") == 1195259493
    assert gw.java_hash("ahas_route") == gm.ro.java_string_hash("ahas_route")


def test_converter_apply_to_param_rule():
    """GatewayRuleConverterTest.testConvertAndApplyToParamRule (:46): the fields carried over."""
    c = gm.Converted([G(0, "routeId1", count=2, interval_sec=2, burst=2, item=I(gw.PARSE_CLIENT_IP))])
    p, = c.prules
    assert (p.resource, p.count, p.control_behavior, p.duration_in_sec, p.burst_count, p.param_idx) == (0, 2.0, 0, 2, 2, 0)
    assert p.max_queueing_time_ms == 500 and p.item_count == 0 and c.slot_of_rule() == [0]


def manager_rules():
    """GatewayRuleManagerTest.testLoadAndGetGatewayRules (:38-72)."""
    return [G(0, "ahas_route", count=500, interval_sec=1),
            G(0, "ahas_route", count=20, interval_sec=2, burst=5, item=I(gw.PARSE_CLIENT_IP)),
            G(1, "complex_route_ZZZ", count=10, interval_sec=1, control_behavior=2, max_queueing_timeout_ms=600,
              item=I(gw.PARSE_HEADER, "X-Sentinel-Flag"))]


def test_manager_load_and_get():
    c = gm.Converted(manager_rules())
    assert c.slot_of_rule() == [1, 0, 0]                   # rule2 and rule3 have index 0; the rule without item comes after
    assert sorted(p.param_idx for p in c.prules if p.resource == 0) == [0, 1]
    assert c.by_res[0] == [0, 1]                           # getRulesForResource holds rule1 and rule2


def validity_rules():
    """GatewayRuleManagerTest.testIsValidRule (:74+): bad1..bad4, good1..good3."""
    return [(G(0, None), False), (G(0, "abc", interval_sec=0), False),
            (G(0, "abc", item=I(gw.PARSE_URL_PARAM)), False),
            (G(0, "abc", item=I(gw.PARSE_URL_PARAM, "p", "def", -1)), False),
            (G(0, "abc"), True), (G(0, "abc", item=I(0)), True),
            (G(0, "abc", item=I(gw.PARSE_CLIENT_IP, "Origin", "def", 2)), True)]


def test_is_valid_rule():
    for r, want in validity_rules():
        assert gm.valid_rule(r) == want, r


REQ = dict(client_ip="66.77.88.99", host="hello.test.sentinel", headers={"X-Sentinel-Flag": "Sentinel"},
           params={"p": "17"}, cookies={"myCookie": "Sentinel-Foo"})


def test_parser_no_param_item():
    """GatewayParamParserTest.testParseParametersNoParamItem (:61)."""
    c = gm.Converted([G(0, "my_test_route_A", count=5, interval_sec=1),
                      G(0, "my_test_route_A", count=10, control_behavior=2, max_queueing_timeout_ms=1000)])
    assert c.parse(0, ROUTE, {}) == ["$D"]


def items_rules():
    """GatewayParamParserTest.testParseParametersWithItems (:85)."""
    a = "my_test_route_A"
    return [G(0, a, count=2, interval_sec=2, burst=2, item=I(gw.PARSE_CLIENT_IP)),
            G(0, a, count=10, interval_sec=1, control_behavior=2, max_queueing_timeout_ms=600,
              item=I(gw.PARSE_HEADER, "X-Sentinel-Flag")),
            G(0, a, count=20, interval_sec=1, burst=5, item=I(gw.PARSE_URL_PARAM, "p")),
            G(0, a, count=120, interval_sec=10, burst=30, item=I(gw.PARSE_HOST)),
            G(0, a, count=50, interval_sec=30, item=I(gw.PARSE_COOKIE, "myCookie")),
            G(0, a, count=10, interval_sec=10),
            G(1, "my_test_route_B", resource_mode=API, count=5, interval_sec=1, item=I(gw.PARSE_URL_PARAM, "p"))]


def test_parser_with_items():
    c = gm.Converted(items_rules())
    # 5 with parameters, 1 normal flow with the generated constant
    assert c.parse(0, ROUTE, REQ) == ["66.77.88.99", "Sentinel", "17", "hello.test.sentinel", "Sentinel-Foo", "$D"]
    assert c.parse(1, ROUTE, REQ) == []
    assert c.parse(1, API, dict(REQ, params={"p": "fs"})) == ["fs"]


def test_parser_empty_pattern():
    """GatewayParamParserTest.testParseParametersWithEmptyItemPattern (:190): an empty pattern takes no effect."""
    c = gm.Converted([G(0, "my_test_route_DS(*H", count=10, interval_sec=2, item=I(gw.PARSE_HEADER, "X-Sentinel-Flag", "", 0))])
    assert c.parse(0, ROUTE, dict(headers={"X-Sentinel-Flag": "Sent1nel"})) == ["Sent1nel"]
    assert c.prules[0].item_count == 1                      # (a non-null pattern still gets the "$NM" item)


def matching_rules():
    """GatewayParamParserTest.testParseParametersWithItemPatternMatching (:219)."""
    return [G(0, "my_test_route_F&@", count=10, interval_sec=1, control_behavior=2, max_queueing_timeout_ms=600,
              item=I(gw.PARSE_HEADER, "X-Sentinel-Flag", "Wow", gw.MATCH_EXACT)),
            G(0, "my_test_route_F&@", count=20, interval_sec=1, burst=5, item=I(gw.PARSE_URL_PARAM, "p", "warn", gw.MATCH_CONTAINS)),
            G(1, "my_test_route_E5K", resource_mode=API, count=5, interval_sec=1,
              item=I(gw.PARSE_URL_PARAM, "p", r"\d+", gw.MATCH_REGEX))]


def test_parser_pattern_matching():
    c = gm.Converted(matching_rules())
    q = lambda h, p: dict(headers={"X-Sentinel-Flag": h}, params={"p": p})  # noqa: E731
    assert c.parse(0, ROUTE, q("Wow", "warn")) == ["Wow", "warn"]
    assert c.parse(0, ROUTE, q("Wow_foo", "warn_foo")) == ["$NM", "warn_foo"]
    assert c.parse(0, ROUTE, q("foo", "foo")) == ["$NM", "$NM"]
    assert c.parse(1, API, q("foo", "23")) == ["23"]
    assert c.parse(1, API, q("foo", "some233")) == ["$NM"]
    # REGEX through the flag: the front-end table evaluates the regex, the value's flag carries the answer
    t = gw.RuleTable(matching_rules())
    fid = t.c_rules[2].field_id
    assert [(f, fl) for f, _, fl in t.items_of(q("foo", "some233")) if f == fid] == [(fid, abi.GW_NOMATCH)]
    assert [(f, fl) for f, _, fl in t.items_of(q("foo", "23")) if f == fid] == [(fid, 0)]


# ---- sf_gateway_convert against the model ----------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from sentinel_amd import engine
    engine.lib()
    return engine


def rule_tuple(p):
    return (p.resource, p.grade, p.param_idx, p.control_behavior, p.count, p.max_queueing_time_ms, p.burst_count,
            p.duration_in_sec, p.item_count, p.item_offset if p.item_count else 0)


def convert_both(engine, rules):
    """The engine's conversion and the model's, as comparable values (or the error each raises)."""
    t = gw.RuleTable(rules)
    try:
        pr, it, slot, desc = engine.gateway_convert(t.c_rules, t.patterns)
        got = ([rule_tuple(p) for p in pr], [(x.tag, x.count, x.bits) for x in it], slot.tolist(),
               {d.resource: (d.n_slots, d.n_item_slots, d.mode_gate,
                             [(d.slot[a].parse_strategy, d.slot[a].match_strategy,
                               None if d.slot[a].pattern == abi.GW_NONE else t.patterns[d.slot[a].pattern], d.slot[a].field_id)
                              for a in range(d.n_item_slots)]) for d in desc})
    except engine.EngineError as e:
        got = e.code
    try:
        c = gm.Converted(rules)
        descs = {}
        for res in c.by_res:
            n_slots, n_item, gate, slots = c.desc(res)
            if n_slots > abi.SF_MAX_ARGS:
                raise OverflowError
            descs[res] = (n_slots, n_item, gate, [(pa, ma, pt, t.c_rules[i].field_id) for pa, ma, pt, i in slots])
        per = {}
        for p in c.prules:
            per[p.resource] = per.get(p.resource, 0) + 1
        if max(per.values(), default=0) > abi.SF_MAX_RULES_PER_RESOURCE:
            raise OverflowError
        want = ([rule_tuple(p) for p in c.prules], [(x.tag, x.count, x.bits) for x in c.items], c.slot_of_rule(), descs)
    except gm.Unsupported:
        want = abi.SF_ERR_UNSUPPORTED
    except OverflowError:
        want = abi.SF_ERR_CAPACITY
    return got, want


def test_convert_reference_cases(engine):
    for rules in (manager_rules(), matching_rules(), [r for r, _ in validity_rules() if r.name is not None]):
        got, want = convert_both(engine, rules)
        assert got == want and not isinstance(got, int)
    got, want = convert_both(engine, items_rules())        # six slots: more than SF_MAX_ARGS
    assert got == want == abi.SF_ERR_CAPACITY


def random_rules(rng, n, n_res, max_items):
    rules, per = [], {}
    for _ in range(n):
        res = int(rng.integers(0, n_res))
        kw = dict(resource_mode=int(rng.choice([0, 0, 0, 1])), grade=int(rng.choice([1, 1, 0])),
                  count=float(rng.choice([-1, 0, 1, 2, 5, 10])), interval_sec=int(rng.choice([0, 1, 1, 2])),
                  control_behavior=int(rng.choice([0, 0, 2])), burst=int(rng.choice([0, 0, 3])),
                  max_queueing_timeout_ms=int(rng.choice([-1, 0, 500])))
        it = None
        if rng.random() < 0.5 and per.get(res, 0) < max_items:
            parse = int(rng.choice([-1, 0, 1, 2, 3, 4, 9]))
            it = I(parse, rng.choice([None, " ", "f", "g"]), rng.choice([None, "", "pat", "x"]), int(rng.choice([-1, 0, 1, 2, 3, 7])))
            per[res] = per.get(res, 0) + 1
        rules.append(G(res, f"res-{res}", item=it, **kw))
    return rules


@pytest.mark.parametrize("seed", range(40))
def test_convert_random(engine, seed):
    """Seeded rule sets: equal rules without item, resources at 4 and 5 slots, mixed modes, invalid rules, and more
    than 12 converted rules so that the global HashSet resizes."""
    rng = np.random.default_rng(100 + seed)
    rules = random_rules(rng, int(rng.choice([6, 20, 40])), int(rng.choice([2, 5, 9])), int(rng.choice([3, 3, 4, 5])))
    got, want = convert_both(engine, rules)
    assert got == want


def test_convert_random_reaches_its_cases(engine):
    kinds = set()
    for seed in range(40):
        rng = np.random.default_rng(100 + seed)
        rules = random_rules(rng, int(rng.choice([6, 20, 40])), int(rng.choice([2, 5, 9])), int(rng.choice([3, 3, 4, 5])))
        got, _ = convert_both(engine, rules)
        if isinstance(got, int):
            kinds.add(got)
            continue
        pr, _, slot, desc = got
        kinds.add("ok")
        if len(pr) > 12:
            kinds.add("resize")
        if any(d[0] == 4 for d in desc.values()):
            kinds.add("4 slots")
        if any(d[2] == abi.GW_GATE_NEVER for d in desc.values()):
            kinds.add("mixed modes")
        valid_non = [i for i, r in enumerate(rules) if r.item is None and gm.valid_rule(r)]
        if len({(rules[i].resource, slot[i]) for i in valid_non}) < len(valid_non) and \
                len([p for p in pr]) < len([s for s in slot if s >= 0]):
            kinds.add("collapsed")
    assert {"ok", "resize", "4 slots", "mixed modes", "collapsed", abi.SF_ERR_CAPACITY} <= kinds, kinds


def test_string_bits(engine):
    for s in ("", "a", "$NM", "$D", "é€\U0001F600", "x" * 65):
        assert engine.gateway_string_bits(s) == gm.bits_of(s)


# ---- the parser code under the sanitizers -----------------------------------------------------------
def _hex(s: bytes) -> str:
    return s.hex() or "-"


def _check_lines():
    rng = np.random.default_rng(77)
    alphabet = ["a", "b", "aa", "ab", "$", "N", "M", "é", "€", "\U0001F600", "è", "x"]
    cases = []
    for _ in range(4000):
        v = "".join(rng.choice(alphabet, size=int(rng.integers(0, 7))))
        p = "".join(rng.choice(alphabet[:4] + alphabet[7:10], size=int(rng.integers(0, 4))))
        if rng.random() < 0.3 and v:
            a = int(rng.integers(0, len(v)))
            p = v[a:a + int(rng.integers(1, 4))]
        cases.append((int(rng.choice([-1, 0, 1, 2, 3, 4, 5])), int(rng.choice([0, 1, 2, 3, 7])), int(rng.integers(0, 2)),
                      int(rng.random() < 0.9), p, v))
    borders = [(2, 0, EX, v) for EX in (gc.EXACT_P,) for v in gc.STR_HEADER]
    borders += [(3, 3, "aab", v) for v in gc.STR_PARAM] + [(1, 3, gc.UTF_P, v) for v in gc.STR_HOST]
    borders += [(4, 0, "", v) for v in gc.STR_COOKIE] + [(4, 3, "x" * 65, "x" * n) for n in (63, 64, 65)]
    borders += [(2, 1, "ab", "zz"), (2, 7, "ab", "zz"), (2, 3, "NM", "$NM"), (2, 0, "$NM", "$NM")]
    cases += [(pa, ma, 0, 1, p, v) for pa, ma, p, v in borders]
    lines = []
    for parse, match, flags, present, p, v in cases:
        it = I(parse, "f", p, match)
        if not present or parse < 0 or parse > 4:
            want = None
        elif not p:
            want = v
        elif match == 0:
            want = v if v == p else "$NM"
        elif match == 3:
            want = v if p in v else "$NM"
        elif match == 2:
            want = "$NM" if flags & abi.GW_NOMATCH else v
        else:
            want = v
        if match != 2 and present and 0 <= parse <= 4:          # the model's parser agrees with this restatement
            key = {0: "client_ip", 1: "host"}.get(parse)
            q = {key: v} if key else {{2: "headers", 3: "params", 4: "cookies"}[parse]: {"f": v}}
            assert gm.parse_internal(it, q) == want
        tag, bits = gm.arg(want)
        lines.append(f"{parse} {match} {flags} {present} {_hex(p.encode())} {_hex(v.encode())} {tag} {bits:016x}\n")
    return lines


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("gateway")
    lines = _check_lines()
    (d / "cases.txt").write_text("".join(lines))
    exe = str(d / "gateway_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, os.path.join(HERE, "gateway_check.cpp")])
    return len(lines), lines, subprocess.run([exe, str(d / "cases.txt")], capture_output=True, text=True)


def test_parser_under_sanitizers(check_output):
    n, lines, r = check_output
    nm = f"{gm.bits_of('$NM'):016x}"
    assert sum(l.split()[7] == nm for l in lines) > 500 and sum(l.split()[6] == "0" for l in lines) > 300
    assert r.returncode == 0 and r.stdout.strip() == f"ok {n}", r.stdout[-2000:] + r.stderr[-4000:]


# ---- the GPU workloads sit on their borders ----------------------------------------------------------
CASES = {"strings": gc.strings, "rule_rows": gc.rule_rows, "threads": gc.threads,
         **{f"layout{n}": (lambda n=n: gc.layout(n)) for n in gc.LAYOUT_N}}


@pytest.fixture(scope="module")
def built():
    return {name: gc.build(make()) for name, make in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_case_guards(so, built, name):
    b = built[name]
    gc.distinct_bits(b["built"])
    w = b["w"]
    ora = so.OracleEngine(w["cfg"])
    ora.load_param_rules(w["param"], w["items"])
    gc.guard_decisions(b, [ora.submit(x) for x in w["batches"]])


def test_strings_borders(built):
    hb, _, want, _ = built["strings"]["built"][0]
    lens = {int(hb.str_off[k + 1] - hb.str_off[k]) for k in range(hb.n_str)}
    assert set(gc.LENGTHS) <= lens
    L = len(gc.EXACT_P)
    assert {L - 1, L, L + 1} <= {len(v) for v in gc.STR_HEADER}
    assert gc.STR_PARAM[0].startswith("aab") and gc.STR_PARAM[1].endswith("aab") and "aab" in "aaab" and len("aa") < 3
    assert [len(c.encode()) for c in gc.UTF_P] == [2, 3, 4]
    # the last string of the table is a value, and it is matched at its last bytes
    last = bytes(hb.data[hb.str_off[-2]:hb.str_off[-1]])
    assert int(hb.str_off[-1]) == hb.data.size and last.endswith(b"aab") and int(hb.val_str[-3:].max()) == hb.n_str - 1
    nm, conv = gm.bits_of("$NM"), built["strings"]["conv"]
    for slot in range(4):                                   # every item slot sees values, "$NM" from a failed match included
        col = want.arg_bits[slot][want.n_args == 4]
        assert (col == nm).any() and (col != nm).any(), slot
    assert "$NM" in gc.STR_COOKIE and "$NM" in gc.STR_HEADER  # a literal "$NM" value
    assert conv.desc(0)[:3] == (4, 4, ROUTE)


def test_rule_rows_reach_every_row(built):
    b = built["rule_rows"]
    conv, (hb, ev, want, _) = b["conv"], b["built"][0]
    d = {r: conv.desc(r) for r in range(gc.R)}
    assert d[1][:3] == (1, 0, abi.GW_GATE_ANY) and d[2][:3] == (3, 2, abi.GW_GATE_NEVER) and d[10][0] == 0
    assert d[11][:2] == (2, 2) and [p.param_idx for p in conv.prules if p.resource == 11] == [1]
    assert d[12][0] == 0 and d[7][:3] == (2, 1, ROUTE)
    ent = (want.flags & abi.EV_EXIT) == 0
    res, na = want.res_id, want.n_args
    mode = np.zeros(ev.n_total, np.int32)
    for i in range(hb.n):
        k = int(hb.res_off[i + 1] - hb.res_off[i])
        mode[hb.ev_index[i]:hb.ev_index[i] + k] = hb.res_mode[hb.res_off[i]:hb.res_off[i + 1]]
    assert (na[ent & (res == 1)] == 1).all() and {0, 1} <= set(mode[res == 1].tolist())        # "$D" whatever the mode
    assert (want.arg_bits[0][res == 1] == gm.bits_of("$D")).all()
    assert (na[res == 2] == 0).all() and (na[res == 10] == 0).all()
    assert set(na[(res == 3) & (mode == API)].tolist()) == {0} and set(na[(res == 3) & (mode == ROUTE)].tolist()) == {1}
    r4 = res == 4
    assert (want.arg_tag[2][r4 & (na == 3)] == abi.TAG_NULL).all()                             # parse strategy 9
    nm = gm.bits_of("$NM")
    has = want.arg_tag[0][r4 & (na == 3)] == abi.TAG_STRING
    assert has.any() and not (want.arg_bits[0][r4] == nm).any() and not (want.arg_bits[1][r4] == nm).any()   # PREFIX, 7
    assert (want.arg_tag[0][res == 5] == abi.TAG_NULL).any()                                   # an absent item
    r6 = (res == 6) & (na == 2)
    a, c = want.arg_bits[0][r6] == nm, want.arg_bits[1][r6] == nm
    assert (a & ~c).any() and (a & c).any() and (~a & ~c).any()                                # the two flags differ
    assert (np.diff(hb.res_off) == 4).any() and (np.diff(hb.val_off) == 0).any()               # 4 entries; no values
    assert (want.flags & abi.EV_PRIO).any() and (want.count == 2).any()
    w = b["w"]
    hot = [p for p in w["param"] if p.resource == 7][-1]
    assert w["items"][hot.item_offset].bits == gm.bits_of("10.0.0.1") and hot.item_count == 1
    assert (want.arg_bits[0][res == 7] == gm.bits_of("10.0.0.1")).any()


def test_threads_and_layout_borders(built):
    (hb0, ev0, want0, _), (hb1, ev1, want1, ct1) = built["threads"]["built"]
    assert ev0.exit_pos.size > 50 and ev1.exit_pos.size == 0
    late = ((want1.flags & abi.EV_EXIT) != 0) & (ev1.entry_ref == -1)
    assert late.sum() > 10 and (want1.n_args[late] == 2).all() and (ct1[late] > 0).all()
    p = ev0.exit_pos
    assert (want0.arg_bits[:, p] == want0.arg_bits[:, ev0.entry_ref[p]]).all() and (want0.n_args[p] == 2).all()
    assert [built[f"layout{n}"]["built"][0][0].n for n in gc.LAYOUT_N] == list(gc.LAYOUT_N)
    hb, ev, want, _ = built["layout65"]["built"][0]
    assert set(np.diff(hb.res_off).tolist()) == {1, 4} and (np.diff(hb.val_off) == 0).any()
    gaps = np.ones(ev.n_total, bool)
    for i in range(hb.n):
        gaps[hb.ev_index[i]:hb.ev_index[i] + int(hb.res_off[i + 1] - hb.res_off[i])] = False
    assert gaps.sum() >= 3 and (want.res_id[gaps] == 13).all() and (want.arg_tag[0][gaps] == abi.TAG_LONG).all()
    dup = gc.duplicate_field(hb)
    assert dup.val_field.size > hb.val_field.size and dup.n_str == hb.n_str + 1
