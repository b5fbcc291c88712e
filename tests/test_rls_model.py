"""Envoy rate-limit service on the CPU: the string model (tests/rls_model.py)
pinned with known answers and the reference's own test cases; the engine's
host-compilable key code (sentinel_amd/csrc/sf_rls.h) against the model in a
stand-alone program under ASan + UBSan (tests/rls_check.cpp); the guards of
every GPU workload (tests/rls_cases.py) on the model alone.  Reference tests
are under sentinel-cluster/sentinel-cluster-server-envoy-rls/src/test/java/
com/alibaba/csp/sentinel/cluster/server/envoy/rls/."""
import os
import re
import subprocess

import numpy as np
import pytest

from sentinel_amd import abi, rls
from tests import rls_cases as rc
from tests import rls_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- known answers
def test_java_hash_known_answers():
    assert rm.java_hash("hello") == 99162322
    assert rm.generate_flow_id("hello") == 2246645969
    assert rm.java_hash("polygenelubricants") == -2 ** 31              # Integer.MIN_VALUE
    assert rm.generate_flow_id("polygenelubricants") == -1             # an id <= 0 has no rule
    assert rm.java_hash("") == 0
    assert rm.generate_flow_id("") == -1 != rm.INT_MAX                 # by blankness, not Integer.MAX_VALUE + 0
    assert rm.java_hash("\U0001F600") == 1772899                       # D83D DE00: two code units
    assert rm.generate_flow_id("testConvertToSentinelFlowRules|k1|v1") == 3990326333


def test_is_blank_is_java_whitespace():
    for cp in (0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F, 0x20, 0x1680, 0x2000, 0x2006, 0x2008, 0x200A,
               0x2028, 0x2029, 0x205F, 0x3000):
        assert rm.is_blank(chr(cp)), hex(cp)
    # the no-break spaces, U+180E (Java 11+), NEL, and the neighbours of the ranges
    for cp in (0x00A0, 0x2007, 0x202F, 0x180E, 0x85, 0x08, 0x0E, 0x1B, 0x21, 0x200B, 0x2027, 0x202A, 0x3001, 0xFEFF):
        assert not rm.is_blank(chr(cp)), hex(cp)
    assert rm.is_blank("") and rm.is_blank(" \t　") and not rm.is_blank("  x ") and not rm.is_blank("|")


def test_converter_keys():
    """EnvoySentinelRuleConverterTest.java:58 and :65."""
    domain = "testConvertToSentinelFlowRules"
    k1 = rm.generate_key(domain, [("k1", "v1")])
    k2 = rm.generate_key(domain, [("k2", "v2"), ("k3", "v3")])
    assert k1 == domain + "|k1|v1" and k2 == domain + "|k2|v2|k3|v3"
    assert rm.generate_key(domain, []) == domain
    rules = rls.rules_from_descriptors(domain, [([("k1", "v1")], 10), ([("k2", "v2"), ("k3", "v3")], 20)], namespace_id=3)
    assert [(r.flow_id, r.count) for r in rules] == [(rm.generate_flow_id(k1), 10.0), (rm.generate_flow_id(k2), 20.0)]
    assert all((r.threshold_type, r.sample_count, r.window_interval_ms, r.namespace_id) == (abi.THRESHOLD_GLOBAL, 1, 1000, 3)
               for r in rules)
    assert rls.generate_key(domain, [("k1", "v1")]) == k1


D1, D2 = [("rk1", "rv1")], [("rk2", "rv2"), ("rk3", "rv3")]


def _service(so, domain, c1, c2):
    flow = [rc.flow_rule(rm.generate_key(domain, D1), c1), rc.flow_rule(rm.generate_key(domain, D2), c2)]
    return rm.RlsModel(so, abi.default_config(max_resources=4, max_batch=16), flow)


def test_should_rate_limit_pass(so):
    """SentinelEnvoyRlsServiceImplTest.java:30-66 on real rules: both descriptors have room."""
    domain = "testShouldRateLimitPass"
    r = _service(so, domain, 5, 5).should_rate_limit([(domain, [D1, D2], 1, 1000)])
    assert r.overall.tolist() == [abi.RLS_OK] and r.code.tolist() == [abi.RLS_OK, abi.RLS_OK]      # :63-65
    assert r.limit.tolist() == [5, 5] and r.remaining.tolist() == [4, 4]


def test_should_rate_limit_partial_block(so):
    """SentinelEnvoyRlsServiceImplTest.java:69-108 on real rules: counts 0 and 1
    make the first descriptor block and the second pass."""
    domain = "testShouldRatePartialBlock"
    r = _service(so, domain, 0, 1).should_rate_limit([(domain, [D1, D2], 1, 1000)])
    assert r.overall.tolist() == [abi.RLS_OVER_LIMIT] and len(r.code) == 2                          # :102-103
    assert r.code.tolist() == [abi.RLS_OVER_LIMIT, abi.RLS_OK]                                      # :104-107
    assert r.limit.tolist() == [0, 1] and r.remaining.tolist() == [0, 0]


def test_should_rate_limit_edges(so):
    domain = "edges"
    m = _service(so, domain, 2.5, 1)
    reqs = [(domain, [D1], -1, 1000),                      # onError: nothing checked
            (domain, [], 1, 1000),                         # no descriptors: OK, no statuses
            (domain, [D1, [("no", "rule")], D1, D1], 0, 1000),   # hits 0 counts as 1; no short-circuit
            (domain, [D2], 2, 1001)]
    r = m.should_rate_limit(reqs)
    assert r.overall.tolist() == [abi.RLS_ERROR, abi.RLS_OK, abi.RLS_OVER_LIMIT, abi.RLS_OVER_LIMIT]
    assert r.code.tolist() == [abi.RLS_UNKNOWN, abi.RLS_OK, abi.RLS_OK, abi.RLS_OK, abi.RLS_OVER_LIMIT, abi.RLS_OVER_LIMIT]
    assert r.limit.tolist() == [-1, 2, -1, 2, 2, 1] and r.remaining.tolist() == [0, 1, 0, 0, 0, 0]
    fid = m.flow[0].flow_id
    assert m.cluster_sum(fid, 0, 1001) == 2 and m.cluster_sum(fid, 1, 1001) == 1    # PASS 2, BLOCK 1: the error request left nothing


# ---------------------------------------------------------------- sf_rls.h under the sanitizers
def _case_line(raw: bytes) -> str:
    s = rm.well_formed(raw)
    if s is None:
        return "%s 0 0 0 0 0\n" % (raw.hex() or "-")
    return "%s 1 %d %d %d %d\n" % (raw.hex() or "-", rm.is_blank(s), rm.java_hash(s), rm.generate_flow_id(s),
                                   rm.java_hash("ab|" + s))


def _check_cases():
    rng = np.random.default_rng(99)
    raws = [b"hello", b"polygenelubricants", b"", "\U0001F600".encode(), b"testConvertToSentinelFlowRules|k1|v1"]
    raws += list(rc.ILL_FORMED.values())
    raws += [chr(cp).encode() for cp in sorted(rm.WHITESPACE)] + [" \t　 ".encode()]
    raws += [chr(cp).encode() for cp in (0xA0, 0x2007, 0x202F, 0x180E, 0x85, 0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000,
                                         0xFFFF, 0x10000, 0x10FFFF)]
    raws += [a + "x".encode() + b for a in [c.encode() for c in rc.CODE_POINTS] for b in [c.encode() for c in rc.CODE_POINTS]]
    # 2,000 seeded random strings: raw bytes (mostly ill-formed), and well-formed text with a damaged byte now and then
    for k in range(2000):
        n = int(rng.integers(0, 24))
        if k % 2:
            raws.append(bytes(rng.integers(0, 256, n, dtype=np.uint8)))
        else:
            cps = rng.choice([0x20, 0x41, 0x7C, 0xE9, 0x20AC, 0x3000, 0x1F600, 0x10FFFF, 0x9, 0x2003], n)
            raw = bytearray("".join(chr(int(c)) for c in cps).encode())
            if raw and rng.random() < 0.3:
                raw[int(rng.integers(0, len(raw)))] = int(rng.integers(0x80, 0x100))
            raws.append(bytes(raw))
    return raws


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("rls")
    raws = _check_cases()
    lines = [_case_line(r) for r in raws]
    n_bad = sum(l.split()[1] == "0" for l in lines)
    assert n_bad > 500 and len(lines) - n_bad > 500, "the cases must hold many strings of either kind"
    assert all(_case_line(r).split()[1] == "0" for r in rc.ILL_FORMED.values())
    (d / "cases.txt").write_text("".join(lines))
    exe = str(d / "rls_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, os.path.join(HERE, "rls_check.cpp")])
    return len(lines), subprocess.run([exe, str(d / "cases.txt")], capture_output=True, text=True)


def test_keys_under_sanitizers(check_output):
    n, r = check_output
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(f"{n} cases, 0 failures"), r.stdout[-2000:]


def test_library_flow_id_matches_model():
    """sf_rls_flow_id (host only, no GPU) is the same code behind the C ABI."""
    from sentinel_amd import engine
    for raw in _check_cases()[:120]:
        s = rm.well_formed(raw)
        if s is None:
            with pytest.raises(ValueError):
                engine.rls_flow_id(raw)
        else:
            assert engine.rls_flow_id(raw) == rm.generate_flow_id(s) == engine.rls_flow_id(s)


# ---------------------------------------------------------------- constants and workload guards
def test_constants_follow_the_header():
    hdr = rc.header_constants()
    assert (hdr["RLS_CHUNK"], hdr["RLS_T"], hdr["RLS_LANE_T"]) == (rc.CHUNK, rc.BLOCK, rc.LANE_T)
    assert hdr["RLS_WAVE_MIN"] == rc.WAVE_MIN >= 2 * rc.CHUNK          # the border cases need whole chunks below it
    assert rc.BORDER_LENGTHS == [1, 63, 64, 65, rc.WAVE_MIN - 1, rc.WAVE_MIN, rc.WAVE_MIN + 1, 4 * rc.WAVE_MIN + 17]
    assert rc.FIRST_BLOCK == [0, 31, 63, 64]
    src = open(rc.RLS_HEADER).read()
    table = re.search(r"Character\.isWhitespace.*?\n//\s+([0-9A-F, -]+)\n", src, re.S).group(1)
    cps = set()
    for part in table.replace(" ", "").split(","):
        lo, _, hi = part.partition("-")
        cps |= set(range(int(lo, 16), int(hi or lo, 16) + 1))
    assert cps == set(rm.WHITESPACE)


def test_pack_requests_layout():
    b = rls.pack_requests([("d", [[("k", "v")], []], 1, 5), ("d", [], 0, 6), ("é", [[("k", "€")]], 2, 7)])
    assert (b.n, b.n_desc, b.n_str) == (3, 3, 5)
    assert b.desc_off.tolist() == [0, 2, 2, 3] and b.ent_off.tolist() == [0, 1, 1, 2]
    assert b.domain.tolist() == [0, 0, 1] and b.ent_key.tolist() == [2, 2] and b.ent_val.tolist() == [3, 4]
    assert bytes(b.data) == "dékv€".encode() and b.str_off.tolist() == [0, 1, 3, 4, 5, 8]    # domains first


def test_guard_mixed(so):
    case = rc.mixed()
    rc.guard_mixed(case, rc.reference(case, so))


@pytest.mark.parametrize("L", rc.BORDER_LENGTHS)
def test_guard_wave_border(so, L):
    case = rc.wave_border(L)
    ref = rc.reference(case, so)
    rc.guard_border(case, ref, L)
    if L > rc.FIRST_BLOCK[-1]:
        for k, p in enumerate(rc.FIRST_BLOCK):             # descriptor p is the first blocked one of rule k
            code = ref.results[k].code
            assert code[p] == abi.RLS_OVER_LIMIT and (code[:p] == abi.RLS_OK).all(), (k, p)
    if L >= 3 * rc.CHUNK:                                   # the first bucket boundary is inside the chunk [128, 192)
        ts = np.array([t for _, d, _, t in case.calls[0][1] for _ in d])
        b = int(np.argmax(ts // 1000 != ts[0] // 1000))
        assert 2 * rc.CHUNK < b < 3 * rc.CHUNK - 1, b


def test_guard_old_window(so):
    case = rc.old_window()
    rc.guard_old_window(case, rc.reference(case, so))


def test_guard_strings(so):
    case = rc.strings()
    rc.guard_strings(case, rc.reference(case, so))
    assert len(case.calls[0][1]) < rc.BLOCK


def test_guard_shared(so):
    case = rc.shared()
    rc.guard_shared(case, rc.reference(case, so), so)
