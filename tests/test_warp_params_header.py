"""csrc/warp_params.h compiles alone with g++ (no HIP headers, no library) and gives the reference's shear parameters on
every shear record of tests/golden/warp.bin (tests/warp_params_check.cpp)."""
import os
import subprocess
import tempfile

import warp_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles_alone_and_matches_the_shear_records():
    g = wc.fixture()
    with tempfile.TemporaryDirectory() as td:
        exe, rec = os.path.join(td, "warp_params_check"), os.path.join(td, "records.txt")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "warp_params_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        with open(rec, "w") as f:
            for mat, out in zip(g["shear_in"], g["shear_out"]):
                f.write(" ".join(str(int(v)) for v in list(mat) + list(out)) + "\n")
        res = subprocess.run([exe, rec], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stdout.startswith("warp_params_check ok: %d shear records" % len(g["shear_in"])), res.stdout
