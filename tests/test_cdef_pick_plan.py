"""The integer rules of the frame-level CDEF strength pick (csrc/cdef_pick_plan.h: the greedy schedule, the buffer
layouts, the settle checkpoint's policy and index arithmetic, the RD choice, the parameter conversion, the environment
switches) against the CPU oracle's svt_search_one_dual and finish_cdef_search -- checked by
tests/cdef_pick_plan_check.cpp, a plain C++17 program linked with oracle/cdef_oracle.c: the header has no HIP in it, so a
wrong rule shows here and not only as a pick that differs after a GPU run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
CC = next((c for c in (os.environ.get("CC"), "gcc", "cc", "clang") if c and shutil.which(c)), None)
WARN = ["-O1", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.skipif(CXX is None or CC is None, reason="no host C and C++ compilers")
def test_cdef_pick_plan_against_oracle(tmp_path):
    obj, exe = str(tmp_path / "cdef_oracle.o"), str(tmp_path / "cdef_pick_plan_check")
    subprocess.run([CC, "-std=c11"] + WARN + ["-c", os.path.join(ROOT, "oracle", "cdef_oracle.c"), "-o", obj],
                   check=True, capture_output=True, text=True)
    subprocess.run([CXX, "-std=c++17"] + WARN + ["-o", exe, os.path.join(ROOT, "tests", "cdef_pick_plan_check.cpp"), obj],
                   check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SVTGPU_")}  # the program checks the knobs' defaults
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("cdef_pick_plan_check ok"), r.stderr[-4000:]
