"""csrc/obmc_plan.h compiles alone with g++ (no HIP headers, no library) and its rules hold: masks, blend, the split MV
clamp, the list validation's boundary cases, the exact cover of a block's plane by items and of the blended samples by
passes (tests/obmc_plan_check.cpp).  The geometry table the program prints is held to obmc_pred_cases here."""
import os
import subprocess
import tempfile

import obmc_pred_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "obmc_plan_check.cpp")


def test_header_compiles_alone_and_its_rules_hold():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "obmc_plan_check")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stderr.startswith("obmc_plan_check ok: 17 sizes, "), res.stderr
    rows = [tuple(int(v) for v in line.split()) for line in res.stdout.splitlines()]
    want = [(w, h, p, d, int(oc.skip_plane(w, h, int(p > 0), d)), oc.pred_depth(h if d == 0 else w, int(p > 0)),
             oc.blend_depth(h if d == 0 else w, int(p > 0))) for (w, h) in oc.SIZES for p in range(3) for d in range(2)]
    assert rows == want and len(rows) == 17 * 3 * 2
    # the four cases where the predicted and the blended depth differ
    assert {(w, h, d) for (w, h, p, d, skip, pd, bd) in rows if p == 1 and not skip and pd != bd} == \
        {(32, 8, 0), (8, 8, 1), (8, 16, 1), (8, 32, 1)}
