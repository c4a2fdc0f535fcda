"""AV1 sub-pel interpolation and the temporal filter's motion compensation without a GPU: the numpy restatement
(tests/interp_cases.py) against every record of the reference's fixture, bit-exact; the fixture's coverage; the library's
filter tables against what the reference compiled; the ABI; refusal of bad arguments; the RTCD install."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import interp_cases as ic
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
BLOCKS = ic.block_cases()
PREDS = ic.pred_cases()
SYMBOLS = tuple("svtgpu_av1_%sconvolve_%s" % (hb, f) for hb in ("", "highbd_") for f in svtgpu.INTERP_FORMS) + \
    ("svtgpu_interp_tables", "svtgpu_tf_predict_frame")
SIZES = {(2, 2), (2, 4), (4, 4), (4, 16), (16, 4), (8, 8), (8, 32), (16, 16), (32, 32), (64, 16), (64, 64), (128, 128)}


def test_restatement_matches_every_block_record():
    for c in BLOCKS:
        got = ic.block_expected(c)
        np.testing.assert_array_equal(got, c["out"], err_msg=c["name"])
        assert (int(got.min()), int(got.max())) == c["mm"], c["name"]


@pytest.mark.parametrize("c", PREDS, ids=[c["name"] for c in PREDS])
def test_restatement_matches_every_prediction_record(c):
    for r in range(c["n_refs"]):
        got = ic.predict_frame(c["refs"][r], c["pad"], c["motion"][r], c["bd"], c["w"], c["h"], c["tf_chroma"])
        for p, want in enumerate(c["pred"][r]):
            np.testing.assert_array_equal(got[p], want, err_msg="%s reference %d plane %d" % (c["name"], r, p))


def test_a_border_of_72_never_clamps():
    """The read-border rule: with 72 readable samples the clamped restatement is the reference's."""
    c = PREDS[0]
    free = ic.predict_frame(c["refs"][0], c["pad"], c["motion"][0], c["bd"], c["w"], c["h"], 1)
    b72 = ic.predict_frame(c["refs"][0], c["pad"], c["motion"][0], c["bd"], c["w"], c["h"], 1, border=(72, 72))
    for p in range(3):
        np.testing.assert_array_equal(b72[p], free[p])


def test_fixture_covers_what_the_issue_lists():
    assert {(c["w"], c["h"]) for c in BLOCKS} == SIZES
    for w, h in SIZES:
        pairs = {(c["phx"], c["phy"]) for c in BLOCKS if (c["w"], c["h"]) == (w, h)}
        assert {0 if not (a or b) else 1 if not b else 2 if not a else 3 for a, b in pairs} == {0, 1, 2, 3}, (w, h)
        if w * h < 4096:
            assert pairs == {(a, b) for a in (0, 1, 8, 15) for b in (0, 1, 8, 15)}, (w, h)
    assert {c["bd"] for c in BLOCKS} == {8, 10, 12} and {c["kind"] for c in BLOCKS} == {0, 1, 2, 3}
    for hbd in (False, True):
        for form in range(4):
            mine = [c for c in BLOCKS if (c["bd"] > 8) == hbd and c["form"] == form]
            assert {c["content"] for c in mine} == {0, 1, 2, 3}, (hbd, form)
            assert any(c["mm"][0] == 0 for c in mine) and any(c["mm"][1] == (1 << c["bd"]) - 1 for c in mine), (hbd, form)
    # both 4-tap tables are taken, in either direction
    assert any(c["w"] <= 4 < c["h"] and c["kind"] in (0, 2) and c["form"] == 3 for c in BLOCKS)
    assert any(c["h"] <= 4 < c["w"] and c["kind"] in (0, 2) and c["form"] == 3 for c in BLOCKS)
    assert any(min(c["w"], c["h"]) <= 4 and c["kind"] == 1 and c["form"] for c in BLOCKS)
    assert {(c["bd"], c["tf_chroma"]) for c in PREDS} == {(8, 0), (8, 1), (10, 0), (10, 1)}
    for c in PREDS:
        assert (c["w"], c["h"], c["n_refs"], c["pad"]) == (136, 72, 2, 80) and all(k > 0 for k in c["kinds"]), c["name"]
        ms = [m for r in c["motion"] for m in r]
        assert any(m["use64"] for m in ms)
        mixed = [m for m in ms if not m["use64"] and 0 < sum(m["split32"]) < 4]
        assert any(any(m["split32"][i] and 0 < sum(m["split16"][4 * i:4 * i + 4]) < 4 for i in range(4)) for m in mixed)
    assert len(ic.chain_cases()) == 2 and {c["pred"]["bd"] for c in ic.chain_cases()} == {8, 10}


def test_tables_match_the_reference():
    t = svtgpu.interp_tables()
    assert t.shape == (6, 16, 8)
    np.testing.assert_array_equal(t, ic.tables())
    assert (t.sum(axis=2) == 128).all() and (t[4:, :, :2] == 0).all() and (t[4:, :, 6:] == 0).all()


def test_abi_version_and_symbols():
    L = svtgpu.lib()
    assert L.svtgpu_abi_version() >= 13
    for n in SYMBOLS:
        assert hasattr(L, n) and n in svtgpu.declared_symbols(), n
    assert ctypes.sizeof(svtgpu.TfMotion) == 368 and ctypes.sizeof(svtgpu.TfMotion) % 16 == 0
    assert svtgpu.TfMotion.mv8_x.offset == 112 and svtgpu.TfMotion.split16.offset == 12
    assert ctypes.sizeof(svtgpu.TfBlock) == 256


def test_predict_frame_refuses_bad_arguments():
    """-1 / -3 before a device is asked for (this test runs without one)."""
    L = svtgpu.lib()
    some = ctypes.c_void_p(4096)  # never dereferenced: refused first
    pl, mo = svtgpu.TfPlanes(), svtgpu.TfMotion()
    ok = dict(state=some, refs=ctypes.byref(pl), n=1, bx=72, by=72, motion=ctypes.byref(mo), bd=8, chroma=1, pred=ctypes.byref(pl))

    def call(**kw):
        a = dict(ok, **kw)
        return L.svtgpu_tf_predict_frame(a["state"], a["refs"], a["n"], a["bx"], a["by"], a["motion"], a["bd"], a["chroma"],
                                         a["pred"], None)
    assert call(state=None) == -1 and call(refs=None) == -1 and call(motion=None) == -1 and call(pred=None) == -1
    assert call(n=-1) == -1 and call(bx=-1) == -1 and call(by=-4) == -1
    for bd in (0, 9, 12, 16):
        assert call(bd=bd) == -1, bd
    assert call(n=27) == -3 and call(n=27, state=None) == -3  # SVTGPU_ERR_UNSUPPORTED, as the filter
    assert L.svtgpu_interp_tables(None, None) == -1


@pytest.mark.skipif(not (os.path.isdir(S) and os.path.exists(os.path.join(REF_OBJ, "Lib/Encoder/Codec/aom_dsp_rtcd.o"))),
                    reason="oracle/_ref/obj not built (needs /root/reference)")
def test_interp_install_sets_all_eight_pointers():
    """include/svtgpu_rtcd.h against the reference's own declarations and its complete InterpFilterParams /
    ConvolveParams: the adapters and svtgpu_install_interp_rtcd() compile without a cast under
    -Werror=incompatible-pointer-types, and the install leaves all eight pointers on the library's side."""
    objs = [os.path.join(REF_OBJ, p) for p in ("Lib/Encoder/Codec/aom_dsp_rtcd.o", "Lib/Common/Codec/common_dsp_rtcd.o",
                                               "Lib/Common/Codec/EbUtility.o")]
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "interp_install")
        r = subprocess.run(["gcc", "-O1", "-fPIC", "-ffunction-sections", "-fdata-sections"] + STRICT + INC +
                           [os.path.join(ROOT, "tests", "interp_install.c")] + objs +
                           ["-o", exe, "-Wl,--gc-sections", "-L" + LIB_DIR, "-lsvtgpu", "-Wl,-rpath," + LIB_DIR, "-ldl",
                            "-lm", "-lpthread"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split() == ["before", "0/8", "after", "8/8"], res.stdout
