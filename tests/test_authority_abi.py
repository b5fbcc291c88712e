"""The AuthorityRule additions to the C ABI (include/sentinel_flow.h) and their
mirrors: sentinel_amd/abi.py by gcc's offsetof / sizeof, the Java shim
statically (no JDK here; tests/javashim.py reads the sources).  No GPU."""
import ctypes as C
import re
import subprocess

from sentinel_amd import abi, system_shard
from tests import javashim as j
from tests.test_abi import HEADER, declared_functions

FIELDS = ["resource", "strategy", "app_off", "app_cnt"]


def _c_layout(tmp_path):
    lines = ['printf("- %zu 0\\n", sizeof(sf_authority_rule));']
    lines += ['printf("%s %%zu %%zu\\n", offsetof(sf_authority_rule, %s), sizeof(((sf_authority_rule*)0)->%s));'
              % (f, f, f) for f in FIELDS]
    prog = tmp_path / "auth.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){\n%s\nreturn 0;}\n'
                    % (HEADER, "\n".join(lines)))
    exe = tmp_path / "auth"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    rows = [l.split() for l in subprocess.check_output([str(exe)]).decode().split("\n") if l.strip()]
    return int(rows[0][1]), {r[0]: (int(r[1]), int(r[2])) for r in rows[1:]}


def _header_constants():
    src = open(HEADER).read()
    return {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define (SF_\w+)\s+(-?0x[0-9a-fA-F]+u?|-?\d+)", src)}


def test_header_declares_the_authority_calls():
    fns = declared_functions()
    assert "sf_load_authority_rules" in fns and "sf_authority_mark" in fns
    hdr = _header_constants()
    assert (hdr["SF_AUTHORITY_WHITE"], hdr["SF_AUTHORITY_BLACK"], hdr["SF_V_BLOCK_AUTHORITY"]) == (0, 1, 10)
    assert hdr["SF_ABI_VERSION"] == abi.SF_ABI_VERSION == 2          # additions do not move the version


def test_python_struct_and_constants(tmp_path):
    size, fields = _c_layout(tmp_path)
    assert [f for f, _ in abi.sf_authority_rule._fields_] == FIELDS
    assert C.sizeof(abi.sf_authority_rule) == size == abi.STRUCT_SIZES["sf_authority_rule"]
    for f in FIELDS:
        d = getattr(abi.sf_authority_rule, f)
        assert (d.offset, d.size) == fields[f], f
    hdr = _header_constants()
    assert abi.V_BLOCK_AUTHORITY == hdr["SF_V_BLOCK_AUTHORITY"]
    assert (abi.AUTHORITY_WHITE, abi.AUTHORITY_BLACK) == (hdr["SF_AUTHORITY_WHITE"], hdr["SF_AUTHORITY_BLACK"])
    assert abi.V_BLOCK_AUTHORITY in system_shard._BLOCKED and abi.V_BLOCK_OTHER in system_shard._BLOCKED
    assert abi.V_BLOCK_AUTHORITY not in abi.PASSED


def test_python_loader_tables():
    arr, apps = abi.authority_tables([(7, abi.AUTHORITY_BLACK, [3, 2]), (9, abi.AUTHORITY_WHITE, []), (1, 2, [5])])
    assert [(r.resource, r.strategy, r.app_off, r.app_cnt) for r in arr] == [(7, 1, 0, 2), (9, 0, 2, 0), (1, 2, 2, 1)]
    assert apps.dtype.itemsize == 4 and apps.tolist() == [3, 2, 5]


def test_python_binding_declares_the_symbols():
    from sentinel_amd import engine
    L = engine.lib()
    assert len(L.sf_load_authority_rules.argtypes) == 6 and len(L.sf_authority_mark.argtypes) == 7
    assert hasattr(engine.FlowEngine, "load_authority_rules") and hasattr(engine.FlowEngine, "authority_mark")


def _java_layout():
    src = j.source("AuthorityRuleTable.java")
    m = re.search(r"static final StructLayout AUTHORITY_RULE = MemoryLayout\.structLayout\((.*?)\);", src, re.S)
    off, fields = 0, []
    for t, f in re.findall(r"(\w+)\.withName\(\"(\w+)\"\)", m.group(1)):
        fields.append((f, off, j.SIZES[t]))
        off += j.SIZES[t]
    assert "paddingLayout" not in m.group(1)
    return off, fields


def test_java_layout_constants_and_symbols(tmp_path):
    size, fields = _c_layout(tmp_path)
    jsize, jfields = _java_layout()
    assert jsize == size
    assert [f for f, _, _ in jfields] == FIELDS
    for f, off, sz in jfields:
        assert fields[f] == (off, sz), f
    hdr = _header_constants()
    consts = j.constants()
    for k in ("V_BLOCK_AUTHORITY", "AUTHORITY_WHITE", "AUTHORITY_BLACK"):
        assert consts[k] == hdr["SF_" + k], k
    assert {"sf_load_authority_rules", "sf_authority_mark"} <= set(j.downcalls())
    native = j.source("SentinelFlowNative.java")
    # (engine, rules, n, apps, n_apps, n_loaded) and (engine, res, origin, flags, n, mem, out)
    assert re.search(r'fn\("sf_load_authority_rules",\s*FunctionDescriptor\.of\(JAVA_INT, ADDRESS, ADDRESS, JAVA_INT, '
                     r'ADDRESS, JAVA_INT, ADDRESS\)\)', native)
    assert re.search(r'fn\("sf_authority_mark",\s*FunctionDescriptor\.of\(JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, '
                     r'JAVA_INT, JAVA_INT, ADDRESS\)\)', native)
    table = j.source("AuthorityRuleTable.java")
    assert 'getLimitApp().split(",")' in table and ".trim()" not in table      # split like passCheck: no trimming
    assert "LOAD_AUTHORITY.invokeExact" in table


def test_gpu_flow_slot_keeps_its_own_authority_check():
    """Both routes stay: the shim's slot still runs the reference AuthoritySlot and flags EV_BLOCKED."""
    slot = j.source("GpuFlowSlot.java")
    assert "authority.entry(" in slot and "EV_BLOCKED" in slot and "catch (AuthorityException" in slot
