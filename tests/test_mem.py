"""Who owns device memory (sentinel_amd/csrc/sf_mem.h, sf_worksets.h), checked
on the host: tests/mem_check.cpp runs the pool, the grow-only buffer, the
work-set growth functions, the layout cursor and the staging plan (StagePlan,
with memcpy as its copy) on a malloc backend that fails the k-th allocation, under the address and undefined-behaviour sanitizers (the
leak check at exit included).  Nothing is loaded into Python; the kernel headers
the work sets come from are compiled as host code, like tests/hostsim."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pool_growbuf_worksets_and_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mem_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(HERE, "mem_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
