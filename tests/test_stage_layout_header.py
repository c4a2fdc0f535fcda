"""csrc/stage_layout.h compiles alone with g++ (no HIP headers, no library) and keeps its promises: the grown capacity
covers the need in whole 4 KiB pages and is monotone, and carved regions are 256-aligned, start at 0 and never overlap
(tests/stage_layout_check.cpp)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles_alone_and_keeps_its_layout_rules():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "stage_layout_check")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "stage_layout_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stdout.startswith("stage_layout_check ok: 4014 needs, 3000 size lists"), res.stdout
