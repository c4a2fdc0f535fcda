"""The integer rules of the deblocking level search (csrc/dlf_levels.h: the bisection state machine, the device plan's
init and step, the trial and apply level tables, the picked levels, the environment switches) against the CPU oracle's
search_filter_level loop and lf_info_init -- checked by tests/dlf_levels_check.cpp, a plain C++17 program linked with
oracle/dlf_oracle.c: the header has no HIP in it, so a wrong decision shows here and not only as a pipeline golden
that differs after a GPU run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
CC = next((c for c in (os.environ.get("CC"), "gcc", "cc", "clang") if c and shutil.which(c)), None)
WARN = ["-O1", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.skipif(CXX is None or CC is None, reason="no host C and C++ compilers")
def test_dlf_levels_against_oracle(tmp_path):
    obj, exe = str(tmp_path / "dlf_oracle.o"), str(tmp_path / "dlf_levels_check")
    subprocess.run([CC, "-std=c11"] + WARN + ["-c", os.path.join(ROOT, "oracle", "dlf_oracle.c"), "-o", obj],
                   check=True, capture_output=True, text=True)
    subprocess.run([CXX, "-std=c++17"] + WARN + ["-o", exe, os.path.join(ROOT, "tests", "dlf_levels_check.cpp"), obj],
                   check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SVTGPU_")}  # the program checks the knobs' defaults
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("dlf_levels_check ok"), r.stderr[-4000:]
