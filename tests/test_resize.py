"""The frame resizer without a GPU: the numpy restatement (tests/resize_cases.py) against every record of the reference's
fixture, bit-exact; svtgpu_resize_plan and the library's tables against what the reference's C recorded; the ABI."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import resize_cases as rc
import svtgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
S = os.path.join(REF, "Source")
REF_OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
LIB_DIR = os.path.dirname(svtgpu.LIB_PATH)
INC = ["-I" + os.path.join(S, d) for d in
       ("API", "Lib/Common/Codec", "Lib/Common/C_DEFAULT", "Lib/Encoder/Codec", "Lib/Encoder/C_DEFAULT",
        "Lib/Encoder/Globals", "Lib/Common/ASM_AVX2", "Lib/Encoder/ASM_AVX2", "Lib/Common/ASM_SSE2",
        "Lib/Common/ASM_SSE4_1")] + \
      ["-I" + os.path.join(REF, "third_party/aom/inc"), "-I" + os.path.join(REF, "third_party/cpuinfo/include"),
       "-I" + REF, "-I" + os.path.join(ROOT, "include")]
STRICT = ["-DARCH_X86_64=1", "-Werror=incompatible-pointer-types", "-Werror=discarded-qualifiers"]
PLANES = list(rc.plane_cases())
FRAMES = list(rc.frame_cases())


def test_fixture_covers_the_paths():
    g = rc.fixture()
    plans = {(c["in_w"], c["out_w"]): rc.plan(c["in_w"], c["out_w"]) for c in PLANES}
    plans.update({(c["in_h"], c["out_h"]): rc.plan(c["in_h"], c["out_h"]) for c in PLANES})
    assert {p[2] for p in plans.values()} == {-1, 0, 1, 2, 3, 4}  # every table, and resizes that end on a halving
    for a, b in (("in_w", "out_w"), ("in_h", "out_h")):             # every table in each direction
        assert {rc.plan(c[a], c[b])[2] for c in PLANES} == {-1, 0, 1, 2, 3, 4}, a
    assert {0, 1, 2, 3} <= {p[0] for p in plans.values()}           # zero to three halving steps
    assert any(p[0] >= 2 and p[2] >= 0 for p in plans.values())     # several steps, then an interpolation
    assert any(i % 2 and p[0] for (i, o), p in plans.items())       # an odd length halved (symodd)
    assert [int(v) for v in g["scaled"][:, 1]] == [78, 70, 64, 59, 54, 50, 47, 44, 66]  # denominators 9..17 of 88
    # tile seams of the device kernels, one sample either side, in both directions
    assert {2 * rc.TILE_W - 1, 2 * rc.TILE_W + 1} <= {c["out_w"] for c in PLANES}
    assert {150 * rc.TILE_ROWS - 1, 150 * rc.TILE_ROWS + 1} <= {c["out_h"] for c in PLANES}
    assert len(FRAMES) >= 2 and {c["bd"] for c in FRAMES} == {8, 10}


def test_an_extreme_record_clips_at_both_ends():
    """The generator counted the horizontal stage's sums outside [0, max]; the restatement finds the same counts."""
    seen = 0
    for c in PLANES:
        lo, hi = c["clipped"]
        if not (lo and hi):
            continue
        s = rc.resize_1d(c["src"].astype(np.int64), c["out_w"], c["bd"], clip_last=False)
        assert (int((s < 0).sum()), int((s > (1 << c["bd"]) - 1).sum())) == (lo, hi), c["name"]
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("i", range(len(PLANES)))
def test_restatement_matches_plane_records(i):
    c = PLANES[i]
    np.testing.assert_array_equal(rc.resize_plane(c["src"], c["out_w"], c["out_h"], c["bd"]), c["out"], err_msg=c["name"])


@pytest.mark.parametrize("i", range(len(FRAMES)))
def test_restatement_matches_frame_records(i):
    c = FRAMES[i]
    got = rc.resize_frame(c["src"], c["src_w"], c["src_h"], c["dst_w"], c["dst_h"], c["bd"])
    for p in range(3):
        np.testing.assert_array_equal(got[p], c["out"][p], err_msg="%s plane %d" % (c["name"], p))


def test_abi_version_and_symbols():
    L = svtgpu.lib()
    assert L.svtgpu_abi_version() >= 11
    for n in ("svtgpu_resize_plan", "svtgpu_resize_filter", "svtgpu_resize_half_filters", "svtgpu_resize_plane",
              "svtgpu_resize_frame", "svtgpu_av1_resize_plane", "svtgpu_av1_highbd_resize_plane"):
        assert hasattr(L, n) and n in svtgpu.declared_symbols(), n


def test_plan_matches_recorded_steps_delta_and_offset():
    rows = rc.fixture()["plan"]
    assert len(rows) >= 40
    for row in rows:
        i, o, steps, n, idx, delta, offset = (int(v) for v in row)
        if o > 2 * i:
            continue
        assert svtgpu.resize_plan(i, o) == (steps, n, idx, delta, offset), (i, o)
        assert rc.plan(i, o) == (steps, n, idx, delta, offset), (i, o)


def test_tables_match_the_reference():
    g = rc.fixture()
    for k in range(5):
        np.testing.assert_array_equal(svtgpu.resize_filter(k), g["filters"][k], err_msg="table %d" % k)
    e, o = svtgpu.resize_half_filters()
    np.testing.assert_array_equal(e, g["half_filters"][0])
    np.testing.assert_array_equal(o, g["half_filters"][1])
    # the normative table is the one the superres fixture recorded
    import superres_cases as sc
    np.testing.assert_array_equal(svtgpu.resize_filter(4), sc.fixture()["filter"])


def test_host_only_entries_refuse_bad_arguments():
    L = svtgpu.lib()
    v = [ctypes.c_int32(7) for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    for i, o in [(0, 4), (4, 0), (-1, 4), (65537, 4), (4, 65537), (4, 9), (1, 3)]:
        assert L.svtgpu_resize_plan(i, o, *refs) == -1, (i, o)
        with pytest.raises(svtgpu.SvtGpuError):
            svtgpu.resize_plan(i, o)
    for k in range(4):
        a = list(refs)
        a[k] = None
        assert L.svtgpu_resize_plan(88, 66, *a) == -1
    assert [x.value for x in v] == [7, 7, 7, 7]  # nothing written
    assert L.svtgpu_resize_plan(4, 8, *refs) == 0 and L.svtgpu_resize_plan(65536, 1, *refs) == 0
    buf = np.zeros((64, 8), np.int16)
    for k in (-1, 5, 6):
        assert L.svtgpu_resize_filter(k, svtgpu.ptr(buf)) == -1
    assert L.svtgpu_resize_filter(0, None) == -1 and not buf.any()
    h = np.zeros(4, np.int16)
    assert L.svtgpu_resize_half_filters(None, svtgpu.ptr(h)) == -1 and L.svtgpu_resize_half_filters(svtgpu.ptr(h), None) == -1
    assert not h.any()
    # the device entries refuse a bad argument before they ask for a device
    assert L.svtgpu_resize_plane(None, 16, 8, 8, 8, None, 8, 4, 4, 10, None) == -1
    assert L.svtgpu_resize_frame(None, None, 8, 8, 4, 4, None) == -1


@pytest.mark.skipif(not (os.path.isdir(S) and os.path.exists(os.path.join(REF_OBJ, "Lib/Encoder/Codec/aom_dsp_rtcd.o"))),
                    reason="oracle/_ref/obj not built (needs /root/reference)")
def test_resize_install_sets_both_plane_pointers():
    """include/svtgpu_rtcd.h against the reference's own declarations: svtgpu_install_resize_rtcd() compiles without a
    cast under -Werror=incompatible-pointer-types and leaves both plane pointers on the shims."""
    objs = [os.path.join(REF_OBJ, p) for p in ("Lib/Encoder/Codec/aom_dsp_rtcd.o", "Lib/Common/Codec/common_dsp_rtcd.o",
                                               "Lib/Common/Codec/EbUtility.o")]
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "resize_install")
        r = subprocess.run(["gcc", "-O1", "-fPIC", "-ffunction-sections", "-fdata-sections"] + STRICT + INC +
                           [os.path.join(ROOT, "tests", "resize_install.c")] + objs +
                           ["-o", exe, "-Wl,--gc-sections", "-L" + LIB_DIR, "-lsvtgpu", "-Wl,-rpath," + LIB_DIR, "-ldl",
                            "-lm", "-lpthread"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split() == ["before", "0/2", "after", "2/2"], res.stdout
