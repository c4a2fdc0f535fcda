"""csrc/interintra_plan.h compiles alone with g++ (no HIP headers, no library) and its rules hold: every validation
boundary, the DC division, the edge preparation (tests/interintra_plan_check.cpp).  The mask tables the program prints --
the smooth masks of all 10 plane sizes x 4 modes and the wedge masks of both planes -- are held to interintra_cases here."""
import os
import subprocess
import tempfile

import numpy as np

import interintra_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "interintra_plan_check.cpp")


def test_header_compiles_alone_and_its_rules_hold():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "interintra_plan_check")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stderr.startswith("interintra_plan_check ok: 7 sizes, 10 plane sizes, 40 smooth masks"), res.stderr
    lines, k, smooth, wedge = res.stdout.splitlines(), 0, {}, {}
    while k < len(lines):
        head = lines[k].split()
        key = tuple(int(v) for v in head[1:])
        rows = key[1] >> (key[3] if head[0] == "W" else 0)
        (smooth if head[0] == "S" else wedge)[key] = np.array([[int(v) for v in ln.split()] for ln in lines[k + 1:k + 1 + rows]])
        k += 1 + rows
    assert sorted(smooth) == sorted((w, h, m) for (w, h) in ic.PLANE_SIZES for m in range(4)) and len(smooth) == 40
    for (w, h, m), got in smooth.items():
        np.testing.assert_array_equal(got, ic.smooth_mask(m, w, h), err_msg="smooth %dx%d mode %d" % (w, h, m))
    assert sorted(wedge) == sorted((w, h, i, ss) for (w, h) in ic.SIZES for i in range(16) for ss in range(2))
    for (w, h, i, ss), got in wedge.items():
        np.testing.assert_array_equal(got, ic.wedge_mask_plane(w, h, i, ss), err_msg="wedge %dx%d index %d ss %d" % (w, h, i, ss))
