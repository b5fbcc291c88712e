"""The gateway part of the Java shim (java/.../GatewayRuleTable.java), statically
as tests/test_java_shim.py does for the rest: its Panama FFM layouts equal the C
structs of include/sentinel_flow.h (field offsets and sizes by gcc), every write
goes through a named field of the right width, and its downcalls exist."""
import re
import subprocess

import pytest

from tests import javashim as j
from tests.test_abi import HEADER, declared_functions

C_STRUCT = {"GATEWAY_RULE": "sf_gateway_rule", "GATEWAY_BATCH": "sf_gateway_batch", "GATEWAY_EVENTS": "sf_gateway_events"}


def layouts():
    src = j.source("GatewayRuleTable.java")
    out = {}
    for m in re.finditer(r"static final StructLayout (\w+) = MemoryLayout\.structLayout\((.*?)\);", src, re.S):
        off, fields = 0, []
        for item in re.finditer(r"(\w+)\.withName\(\"(\w+)\"\)|MemoryLayout\.paddingLayout\((\d+)\)", m.group(2)):
            if item.group(3):
                off += int(item.group(3))
                continue
            sz = j.SIZES[item.group(1)]
            assert off % sz == 0, (m.group(1), item.group(2))
            fields.append((item.group(2), off, sz))
            off += sz
        out[m.group(1)] = (off, fields)
    return out


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    lines = []
    for jl, cs in C_STRUCT.items():
        lines.append('printf("%s - %%zu 0\\n", sizeof(%s));' % (cs, cs))
        for f, _, _ in layouts()[jl][1]:
            lines.append('printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cs, f, cs, f, cs, f))
    d = tmp_path_factory.mktemp("jgw")
    (d / "off.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){\n%s\nreturn 0;}\n'
                             % (HEADER, "\n".join(lines)))
    subprocess.check_call(["gcc", "-o", str(d / "off"), str(d / "off.c")])
    out = {}
    for l in subprocess.check_output([str(d / "off")]).decode().split("\n"):
        if l.strip():
            s, f, a, b = l.split()
            ent = out.setdefault(s, [0, {}])
            if f == "-":
                ent[0] = int(a)
            else:
                ent[1][f] = (int(a), int(b))
    return out


def test_layouts_match_the_c_structs(c_layout):
    lay = layouts()
    assert set(lay) == set(C_STRUCT)
    src = open(HEADER).read()
    for jl, (size, fields) in lay.items():
        cs = C_STRUCT[jl]
        csize, cf = c_layout[cs]
        assert size == csize, f"{jl}: FFM layout {size} B, sizeof({cs}) {csize} B"
        for f, off, sz in fields:
            assert cf[f] == (off, sz), f"{jl}.{f}: Java ({off}, {sz}) vs C {cf[f]}"
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cs, cs), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for part in re.findall(r"[\w\s\*]+?([\w\s\*,]+);", body) for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", part)]
        assert set(names) == {f for f, _, _ in fields}, (jl, sorted(set(names) ^ {f for f, _, _ in fields}))


def test_writes_and_downcalls():
    src = j.source("GatewayRuleTable.java")
    fields = {f: sz for f, _, sz in layouts()["GATEWAY_RULE"][1]}
    writes = re.findall(r"s\.set\((\w+), o\(\"(\w+)\"\)", src)
    assert len(writes) >= 15
    for t, f in writes:
        assert j.SIZES[t] == fields[f], (f, t)
    assert {f for _, f in writes} == set(fields) - {"pad"}
    fns = set(declared_functions())
    assert {"sf_load_gateway_rules", "sf_gateway_args", "sf_gateway_string_bits"} <= set(j.downcalls()) & fns
    assert "LOAD_GATEWAY.invokeExact(engine, table, n, strOff, bytes," in src
    assert "for (GatewayFlowRule r : conf)" in src           # the Set's iteration order, not a sorted copy
