"""AuthorityRule on the CPU: the string model (tests/authority_model.py) pinned
with the reference's own test cases, and the engine's host-compilable table
code (sentinel_amd/csrc/sf_authority.h: the loader's builder and the mark
kernel's predicate) against that model in a stand-alone program under ASan +
UBSan (tests/authority_check.cpp).  Reference paths are under
sentinel-core/src/{main,test}/java/com/alibaba/csp/sentinel/slots/block/authority/."""
import os
import subprocess

import numpy as np
import pytest

from tests import authority_model as am
from tests.authority_model import AUTHORITY_BLACK as BLACK, AUTHORITY_WHITE as WHITE, AuthorityRule

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- AuthorityRuleCheckerTest.java:24-58 testPassCheck (origin "appA")
def test_pass_check_reference_cases():
    origin = "appA"
    rule_a = AuthorityRule("testPassCheck", origin + ",appB", WHITE)    # :30-34
    rule_b = AuthorityRule("testPassCheck", "appB", WHITE)              # :35-39
    rule_c = AuthorityRule("testPassCheck", origin, BLACK)              # :40-44
    rule_d = AuthorityRule("testPassCheck", "appC", BLACK)              # :45-49
    assert am.pass_check(rule_a, origin)                                # :51
    assert not am.pass_check(rule_b, origin)                            # :52
    assert not am.pass_check(rule_c, origin)                            # :53
    assert am.pass_check(rule_d, origin)                                # :54


# ---- AuthoritySlotTest.java
def test_slot_no_exception_cases():
    """:25-52 testCheckAuthorityNoExceptionItemsSuccess: a white list holding the origin, then a black list without it."""
    m = am.AuthorityRuleManager()
    res = "testCheckAuthorityNoExceptionItemsSuccess"
    m.load_rules([AuthorityRule(res, "appA,appB", WHITE)])              # :32-38
    assert not m.blocks(res, "appA")                                    # :39
    m.load_rules([AuthorityRule(res, "appD", BLACK)])                   # :41-47
    assert not m.blocks(res, "appA")                                    # :48


def test_slot_black_fail():
    """:54-72 testCheckAuthorityNoExceptionItemsBlackFail expects AuthorityException."""
    m = am.AuthorityRuleManager()
    res = "testCheckAuthorityNoExceptionItemsBlackFail"
    m.load_rules([AuthorityRule(res, "appA,appC", BLACK)])              # :61-67
    assert m.blocks(res, "appA")                                        # :68


def test_slot_white_fail_untrimmed():
    """:74-92 testCheckAuthorityNoExceptionItemsWhiteFail: "appB, appE" is split without trimming."""
    m = am.AuthorityRuleManager()
    res = "testCheckAuthorityNoExceptionItemsWhiteFail"
    m.load_rules([AuthorityRule(res, "appB, appE", WHITE)])             # :81-87
    assert m.blocks(res, "appA")                                        # :88
    assert m.blocks(res, "appE") and not m.blocks(res, " appE") and not m.blocks(res, "appB")


# ---- AuthorityRuleManagerTest.java
def test_manager_load_rules():
    """:25-42 testLoadRules: one valid rule is kept; a load of one invalid rule leaves none."""
    m = am.AuthorityRuleManager()
    rule = AuthorityRule("testLoadRules", "a,b", WHITE)                 # :29-32
    m.load_rules([rule])                                                # :33
    assert m.get_rules() == [rule]                                      # :35-37
    m.load_rules([AuthorityRule()])                                     # :39
    assert m.get_rules() == []                                          # :40-41


def test_manager_is_valid_rule():
    """:44-57 testIsValidRule."""
    assert not am.is_valid_rule(AuthorityRule())                        # ruleA :53
    assert not am.is_valid_rule(None)                                   # ruleB :54
    assert not am.is_valid_rule(AuthorityRule(resource="abc"))          # ruleC :55
    assert am.is_valid_rule(AuthorityRule(resource="bcd", limit_app="abc"))   # ruleD :56
    assert not am.is_valid_rule(AuthorityRule("r", "a", -1))            # AuthorityRuleManager.java:149 strategy >= 0
    assert not am.is_valid_rule(AuthorityRule("r", "  ", WHITE))        # isNotBlank(limitApp)
    assert not am.is_valid_rule(AuthorityRule(" ", "a", WHITE))         # isBlank(resource)


def test_manager_redundant_rule_is_ignored():
    """AuthorityRuleManager.java:125-135: the first valid rule of a resource is kept, a later one does not replace it."""
    m = am.AuthorityRuleManager()
    m.load_rules([AuthorityRule("r", "a", -3), AuthorityRule("r", "appA", BLACK), AuthorityRule("r", "appB", BLACK)])
    assert [r.limit_app for r in m.get_rules()] == ["appA"]
    assert m.blocks("r", "appA") and not m.blocks("r", "appB")


def test_manager_load_null_clears():
    """AuthorityRuleManager.java:111-113 (AuthoritySlotTest.java:124 setUp: loadRules(null))."""
    m = am.AuthorityRuleManager()
    m.load_rules([AuthorityRule("r", "appA", BLACK)])
    assert m.blocks("r", "appA")
    m.load_rules(None)
    assert m.get_rules() == [] and not m.blocks("r", "appA")
    m.load_rules([AuthorityRule("r", "appA", BLACK)])
    m.load_rules([])
    assert not m.blocks("r", "appA")


def test_edge_cases():
    black, white = AuthorityRule("r", "appA,appB", BLACK), AuthorityRule("r", "appA,appB", WHITE)
    for rule in (black, white):                                         # AuthorityRuleChecker.java:36 an empty origin passes
        assert am.pass_check(rule, "") and am.pass_check(rule, None)
    # an origin that is a substring of an app: indexOf finds it (:42), the exact match does not (:49-54)
    assert am.pass_check(black, "app") and not am.pass_check(white, "app")
    # an origin that contains a comma never equals a piece of the split
    assert am.pass_check(black, "appA,appB") and not am.pass_check(white, "appA,appB")
    # a strategy that is neither list kind blocks nothing (:61-70) and is valid (:149)
    other = AuthorityRule("r", "appA", 2)
    assert am.is_valid_rule(other) and am.pass_check(other, "appA") and am.pass_check(other, "appZ")


def test_tables_of_a_rule_list():
    """What a caller hands to the engine: pieces interned like origins, no trimming."""
    it = am.Interner()
    t = am.to_tables([AuthorityRule("res3", "appB, appE,default", WHITE), AuthorityRule("res4", " ", BLACK), None,
                      AuthorityRule(None, "x", BLACK)], lambda s: int(s[3:]), it)
    assert t[0] == (3, WHITE, [it.id("appB"), it.id(" appE"), 0]) and it.id(" appE") != it.id("appE")
    assert t[1] == (4, BLACK, []) and t[2] == (0xFFFFFFFF, BLACK, [it.id("x")])


# ---------------------------------------------------------------- sf_authority.h under the sanitizers
def _res_id(name):
    return int(name[3:])


def _case(name, rules, pair_res, pair_origins, R, sc=1, si=0, it=None):
    """One case of tests/authority_check.cpp from a string rule list: the
    expectation of every (resource, origin) pair comes from the model."""
    it = it or am.Interner()
    mgr = am.AuthorityRuleManager()
    mgr.load_rules(rules)
    tab = am.to_tables(rules, _res_id, it)
    apps, lines = [], []
    for res, strategy, ids in tab:
        lines.append(f"{res} {strategy} {len(apps)} {len(ids)}")
        apps += ids
    kept = sum(1 for r in mgr.get_rules() if _res_id(r.resource) % sc == si)
    pairs = []
    for r in pair_res:
        for o in pair_origins:
            local = r % sc == si and r // sc < R
            pairs.append((r, it.id(o), int(local and mgr.blocks(f"res{r}", o))))
    return _emit(name, R, sc, si, apps, lines, 0, kept, pairs)


def _emit(name, R, sc, si, apps, rule_lines, rc, kept, pairs):
    out = [f"case {name}", f"cfg {R} {sc} {si}", "apps %d %s" % (len(apps), " ".join(map(str, apps))),
           f"rules {len(rule_lines)}"] + rule_lines + [f"expect {rc} {kept}", f"pairs {len(pairs)}"]
    out += ["%d %d %d" % p for p in pairs]
    return "\n".join(out) + "\n", sum(p[2] for p in pairs)


def _cases():
    rng = np.random.default_rng(12)
    out = []
    # list lengths 0 (a blank limitApp: invalid), 1, 2, 3, 8, 9 (the linear / bisection border), 64, 1000,
    # black and white, on row 0, the last row and between; origins in and out of each list
    lens = [0, 1, 2, 3, 8, 9, 64, 1000]
    R = 2 * len(lens)
    rules, origins = [], ["", "default", "other", "app", "zzz", "a,b"]
    for k, n in enumerate(lens):
        names = [f"app{k}_{j}" for j in range(n)]
        rng.shuffle(names)
        for strategy, res in ((BLACK, k), (WHITE, R - 1 - k)):
            rules.append(AuthorityRule(f"res{res}", ",".join(names) if n else " ", strategy))
        origins += names[:3] + names[-2:] + ([names[n // 2]] if n else [])
    out.append(_case("list_lengths", rules, range(R), origins, R))
    # duplicate ids inside a list, the strings "default" / "other" (ids 0 and 1) as list members
    out.append(_case("duplicates", [AuthorityRule("res0", "appA,appB,appA,appA,appB", BLACK),
                                    AuthorityRule("res1", "default,other,default", WHITE),
                                    AuthorityRule("res2", "appA," * 12 + "appC", WHITE)],
                     range(4), ["appA", "appB", "appC", "default", "other", ""], 4))
    # first-wins: an invalid rule first, then the kept one, then conflicting later rules; strategy 2; a blank resource
    out.append(_case("first_wins", [AuthorityRule("res1", "appA", -1), AuthorityRule("res1", "appA", BLACK),
                                    AuthorityRule("res1", "appB", BLACK), AuthorityRule("res1", "appA", WHITE),
                                    AuthorityRule("res2", "appA", 2), AuthorityRule("res2", "appA", BLACK),
                                    AuthorityRule(None, "appA", BLACK), AuthorityRule("res0", "appB, appE", WHITE)],
                     range(3), ["appA", "appB", "appE", " appE", ""], 3))
    # shard_count 2 / index 1: foreign rules dropped, rows = res / 2; resources beyond the rows
    srules = [AuthorityRule(f"res{r}", "appA,appB", BLACK if r % 3 else WHITE) for r in range(0, 12)]
    out.append(_case("shard_1_of_2", srules, list(range(14)) + [999, 0xFFFFFFFE], ["appA", "appC", ""], 6, 2, 1))
    out.append(_case("shard_0_of_2", srules, list(range(14)), ["appA", "appC", ""], 6, 2, 0))
    # origin id 0, the largest interned id and SF_ORIGIN_NONE; resources out of range
    it = am.Interner()
    it.names[0xFFFFFFFE] = "the-last-one"
    it.ids["the-last-one"] = 0xFFFFFFFE
    out.append(_case("id_extremes", [AuthorityRule("res0", "default,the-last-one", BLACK),
                                     AuthorityRule("res4", "the-last-one", WHITE)],
                     [0, 4, 5, 6, 0x7FFFFFFF, 0xFFFFFFFF], ["default", "the-last-one", "", "other"], 5, it=it))
    out.append(_case("no_rules", [], range(3), ["appA", ""], 3))
    out.append(_case("only_invalid", [AuthorityRule("res0", "", BLACK), AuthorityRule("res1", "a", -1)], range(3),
                     ["a", ""], 3))
    # malformed ranges: refused before anything is read, whatever else the rule says
    for name, line in [("range_past_apps", "0 1 2 5"), ("range_wraps_u32", "0 1 4294967295 2"),
                       ("range_of_invalid_rule", "0 -1 3 1"), ("range_of_foreign_rule", "1 1 0 4")]:
        out.append(_emit(name, 4, 2, 0, [5, 6, 7], ["0 1 0 1", line], -1, 0, []))
    out.append(_emit("range_ok_when_empty", 4, 1, 0, [5, 6, 7], ["0 1 4000000000 0", "1 1 1 2"], 0, 1,
                     [(1, 6, 1), (1, 5, 0), (0, 5, 0)]))
    out.append(_emit("rule_beyond_rows", 4, 1, 0, [5], ["4 1 0 1"], -1, 0, []))
    return out


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("authority")
    cases = _cases()
    assert sum(c[1] for c in cases) > 50, "the model must block in the cases"
    (d / "cases.txt").write_text("".join(c[0] for c in cases))
    exe = str(d / "authority_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(HERE, "authority_check.cpp")])
    r = subprocess.run([exe, str(d / "cases.txt")], capture_output=True, text=True)
    return len(cases), r


def test_tables_and_predicate_under_sanitizers(check_output):
    n, r = check_output
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f"{n} cases, ") and " 0 failures" in r.stdout, r.stdout
