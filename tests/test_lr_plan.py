"""The host plan of the loop-restoration search (csrc/lr_plan.h: units and tiles, the routing of every unit to the big
or small instance of the two resident descents, the buffer layout, the environment knobs) holds its invariants on the
frames the GPU tests and the bench search -- checked by tests/lr_plan_check.cpp, a plain C++17 program: the planner has
no HIP in it, and a wrong plan would not fail a comparison on the device but leave a workgroup waiting for a partner."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_lr_plan_invariants(tmp_path):
    exe = str(tmp_path / "lr_plan_check")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "lr_plan_check.cpp")], check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SVTGPU_")}  # the program checks the knobs' defaults
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("lr_plan_check ok"), r.stderr[-4000:]
