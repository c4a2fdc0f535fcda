"""csrc/pred_plan.h compiles alone with g++ (no HIP headers, no library) and its rules hold: the size rule, the wave items
against the LDS budget and an exact cover, the plane checks' boundary cases, the MV clamp, the metadata layout
(tests/pred_plan_check.cpp).  The tables the program writes out are held to compound_cases here."""
import os
import re
import subprocess
import tempfile

import compound_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pred_plan_check.cpp")


def test_the_programs_tables_are_the_fixtures():
    text = open(SRC).read()
    sizes = re.search(r"kSizes\[17\]\[2\] = \{(.*?)\};", text, re.S).group(1)
    assert [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+)\}", sizes)] == cc.SIZES
    tiling = re.search(r"kTiling\[23\]\[4\] = \{(.*?)\};", text, re.S).group(1)
    assert [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+), (\d+), (\d+)\}", tiling)] == \
        [(b["x"], b["y"], b["w"], b["h"]) for b in cc.batch_cases()[0]["blocks"]]


def test_header_compiles_alone_and_its_rules_hold():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "pred_plan_check")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stdout.startswith("pred_plan_check ok: 17 sizes, "), res.stdout
