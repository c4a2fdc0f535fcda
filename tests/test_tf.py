"""The temporal filter's filter half without a GPU: the numpy restatement (tests/tf_cases.py) against every record of the
reference's fixture, bit-exact; the fixture's coverage; the library's tables and host-only functions against what the
reference's C recorded; the ABI; refusal of bad arguments; the RTCD install."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import svtgpu
import tf_cases as tc

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
NOISE = list(tc.noise_cases())
BLOCKS = list(tc.block_cases())
CENTRAL = list(tc.central_cases())
FINAL = list(tc.final_cases())
FRAMES = list(tc.frame_cases())
SYMBOLS = ("svtgpu_tf_state_create", "svtgpu_tf_state_destroy", "svtgpu_tf_estimate_noise", "svtgpu_tf_estimate_noise_async",
           "svtgpu_tf_read_noise", "svtgpu_tf_filter_frame", "svtgpu_tf_noise_log1p_fp16", "svtgpu_tf_decay_factor_fp16",
           "svtgpu_tf_tables", "svtgpu_estimate_noise_fp16", "svtgpu_estimate_noise_highbd_fp16",
           "svtgpu_tf_apply_planewise_medium", "svtgpu_tf_apply_planewise_medium_hbd", "svtgpu_tf_apply_zz_planewise_medium",
           "svtgpu_tf_apply_zz_planewise_medium_hbd", "svtgpu_tf_apply_filtering_central",
           "svtgpu_tf_apply_filtering_central_highbd", "svtgpu_tf_get_final_filtered_pixels")


def _run_block(c, stats=None):
    acc, cnt = [a.copy() for a in c["accum_in"]], [a.copy() for a in c["count_in"]]
    tc.apply_block(c["meta"], c["idx"], c["src"], c["pre"], acc, cnt, c["decay"], c["mv_dist_th"], c["tf_chroma"], c["bd"],
                   c["zz"], stats)
    return acc, cnt


def test_fixture_covers_the_paths():
    g = tc.fixture()
    assert int(g["divu"][0]) == 1  # OD_DIVU's table branch equals plain division (count == 1000)
    assert {(c["bd"], c["w"], c["h"]) for c in NOISE} == {(b, w, h) for b in (8, 10) for w, h in ((64, 48), (67, 35), (640, 360))}
    assert {c["content"] for c in NOISE} == {0, 1, 2, 3, 4}
    for bd in (8, 10):
        nums = {c["content"]: tc.estimate_noise(c["src"], bd)[1] for c in NOISE if c["bd"] == bd and c["w"] == 64}
        assert nums[1] == 0 and nums[2] == 15 and nums[3] == 16
    axes = lambda k: {c[k] for c in BLOCKS}
    assert axes("bd") == {8, 10} and axes("bw") == {32, 16} and axes("zz") == {0, 1} and axes("tf_chroma") == {0, 1}
    assert axes("prefill") == {0, 1} and axes("content") == {0, 1, 2, 3} and axes("idx") == {0, 1, 2, 3}
    assert 1080 in axes("mv_dist_th") and min(axes("mv_dist_th")) < 100
    for bd in (8, 10):
        sub = [c for c in BLOCKS if c["bd"] == bd and not c["zz"]]
        assert {int(c["meta"]["split"][c["idx"]]) for c in sub} == {0, 1}
        assert any(c["wide"] for c in sub)  # the 32-bit avg_err product passes 2^32
        assert any(tc.d_factor_fp8(int(c["meta"]["mv32"][c["idx"]][0]), int(c["meta"]["mv32"][c["idx"]][1]),
                                   c["mv_dist_th"]) > 256 for c in sub)
        assert any(not c["meta"]["mv32"].any() for c in sub)  # zero motion: sqrt_fast's x <= 15 branch
    stats = []  # over the block and frame records: the 112 clamp, weight 1000 (scaled_diff16 0), and values between
    for c in BLOCKS:
        _run_block(c, stats)
    for c in FRAMES:
        tc.filter_frame(c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], c["tf_chroma"], c["bd"], c["zz"],
                        c["w"], c["h"], stats)
    assert any(sd == 112 for sd, _, _ in stats) and any(w == 1000 for _, w, _ in stats)
    assert any(0 < sd < 112 for sd, _, _ in stats)
    assert [int(v) for v in BLOCKS[0]["meta"]["err32"]] == [156756, 168763, 143351, 189005]  # the reference test's errors
    assert {(c["bd"], c["tf_chroma"]) for c in CENTRAL} >= {(8, 1), (10, 1), (10, 0)}
    assert {(c["bd"], c["mode"]) for c in FINAL} == {(8, 0), (8, 1), (10, 0), (10, 1)}
    assert all((c["count"][0] == 1000).all() for c in FINAL if c["mode"] == 0)
    assert {(c["bd"], c["n_refs"]) for c in FRAMES} == {(b, n) for b in (8, 10) for n in (0, 1, 5)}
    assert all((c["w"], c["h"]) == (136, 72) for c in FRAMES)
    assert any(c["zz"] for c in FRAMES) and any(not c["tf_chroma"] for c in FRAMES)
    assert any(len({int(m["split"][i]) for row in c["metas"] for m in row for i in range(4)}) == 2 for c in FRAMES)


@pytest.mark.parametrize("i", range(len(NOISE)))
def test_restatement_matches_noise_records(i):
    c = NOISE[i]
    assert tc.estimate_noise(c["src"], c["bd"])[0] == c["out"], c["name"]


@pytest.mark.parametrize("i", range(len(BLOCKS)))
def test_restatement_matches_block_records(i):
    c = BLOCKS[i]
    stats = []
    acc, cnt = _run_block(c, stats)
    for p in range(3):
        np.testing.assert_array_equal(acc[p], c["accum"][p], err_msg="%s accum %d" % (c["name"], p))
        np.testing.assert_array_equal(cnt[p], c["count"][p], err_msg="%s count %d" % (c["name"], p))
    assert any(wide for _, _, wide in stats) == bool(c["wide"]), c["name"]


@pytest.mark.parametrize("i", range(len(CENTRAL)))
def test_restatement_matches_central_records(i):
    c = CENTRAL[i]
    acc, cnt = tc.central(c["src"], c["tf_chroma"])
    for p in range(3):
        np.testing.assert_array_equal(acc[p], c["accum"][p], err_msg=c["name"])
        np.testing.assert_array_equal(cnt[p], c["count"][p], err_msg=c["name"])


@pytest.mark.parametrize("i", range(len(FINAL)))
def test_restatement_matches_final_records(i):
    c = FINAL[i]
    for p in range(3):
        np.testing.assert_array_equal(tc.final(c["accum"][p], c["count"][p]), c["out"][p], err_msg=c["name"])


@pytest.mark.parametrize("i", range(len(FRAMES)))
def test_restatement_matches_frame_records(i):
    c = FRAMES[i]
    got = tc.filter_frame(c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], c["tf_chroma"], c["bd"], c["zz"],
                          c["w"], c["h"])
    for p in range(3):
        h, w = c["out"][p].shape
        np.testing.assert_array_equal(got[p][:h, :w], c["out"][p], err_msg="%s plane %d" % (c["name"], p))


def test_restatement_scalars_match_the_records():
    g = tc.fixture()
    for a, b in g["log1p"]:
        assert tc.noise_log1p_fp16(int(a)) == int(b), a
    for dc, nl, q, out in g["decay"]:
        assert tc.decay_factor_fp16(int(dc), int(nl), int(q)) == int(out), (dc, nl, q)


def test_abi_version_and_symbols():
    L = svtgpu.lib()
    assert L.svtgpu_abi_version() >= 12
    for n in SYMBOLS:
        assert hasattr(L, n) and n in svtgpu.declared_symbols(), n
    assert ctypes.sizeof(svtgpu.TfBlock) == 256 and ctypes.sizeof(svtgpu.TfParams) == 28


def test_tables_match_the_reference():
    g = tc.fixture()
    log1p, sq, expf = svtgpu.tf_tables()
    np.testing.assert_array_equal(log1p, g["tab_log1p"])
    np.testing.assert_array_equal(sq, g["tab_sqrt"])
    np.testing.assert_array_equal(expf, g["tab_expf"])


def test_host_only_functions_match_the_records():
    g = tc.fixture()
    assert len(g["log1p"]) >= 100 and len(g["decay"]) >= 30
    assert {int(r[2]) >= 128 for r in g["decay"]} == {False, True}  # q either side of 128
    bases = [65536 + int(a) for a, _ in g["log1p"]]
    assert min(bases) <= 0 < 458751 < max(bases) and 458752 in bases and 458751 in bases
    for a, b in g["log1p"]:
        assert svtgpu.tf_noise_log1p_fp16(int(a)) == int(b), a
    for dc, nl, q, out in g["decay"]:
        assert svtgpu.tf_decay_factor_fp16(int(dc), int(nl), int(q)) == int(out), (dc, nl, q)


def test_entries_refuse_bad_arguments():
    """-1 before a device is asked for (this test runs without one)."""
    L = svtgpu.lib()
    h, v = ctypes.c_void_p(), ctypes.c_int32(7)
    some = ctypes.c_void_p(4096)  # never dereferenced: the size or bit depth is refused first
    assert L.svtgpu_tf_state_create(None, 64, 64, ctypes.byref(h)) == -1
    for w, hh in ((60, 64), (64, 60), (0, 64), (64, -8)):
        assert L.svtgpu_tf_state_create(some, w, hh, ctypes.byref(h)) == -1, (w, hh)
    assert L.svtgpu_tf_state_create(some, 64, 64, None) == -1 and not h.value
    assert L.svtgpu_tf_estimate_noise(None, some, 8, 64, 64, 48, None, ctypes.byref(v)) == -1
    assert L.svtgpu_tf_estimate_noise(some, None, 8, 64, 64, 48, None, ctypes.byref(v)) == -1
    assert L.svtgpu_tf_estimate_noise(some, some, 8, 64, 64, 48, None, None) == -1
    for bits in (0, 9, 12, 16):
        assert L.svtgpu_tf_estimate_noise(some, some, bits, 64, 64, 48, None, ctypes.byref(v)) == -1, bits
    assert L.svtgpu_tf_estimate_noise(some, some, 8, 32, 64, 48, None, ctypes.byref(v)) == -1  # stride < w
    assert v.value == 7
    assert L.svtgpu_tf_estimate_noise_async(None, some, 8, 64, 64, 48, None) == -1
    assert L.svtgpu_tf_read_noise(None, None, ctypes.byref(v)) == -1
    assert L.svtgpu_tf_filter_frame(None, None, None, 0, None, None, None, None) == -1
    assert L.svtgpu_tf_filter_frame(None, None, None, -1, None, None, None, None) == -1
    assert L.svtgpu_tf_filter_frame(None, None, None, 27, None, None, None, None) == -3  # SVTGPU_ERR_UNSUPPORTED
    assert L.svtgpu_tf_tables(None, None, None, None, None) == -1


@pytest.mark.skipif(not (os.path.isdir(S) and os.path.exists(os.path.join(REF_OBJ, "Lib/Encoder/Codec/aom_dsp_rtcd.o"))),
                    reason="oracle/_ref/obj not built (needs /root/reference)")
def test_tf_install_sets_all_nine_pointers():
    """include/svtgpu_rtcd.h against the reference's own declarations and its complete MeContext: the adapters and
    svtgpu_install_tf_rtcd() compile without a cast under -Werror=incompatible-pointer-types, and the install leaves all
    nine pointers on the library's side."""
    objs = [os.path.join(REF_OBJ, p) for p in ("Lib/Encoder/Codec/aom_dsp_rtcd.o", "Lib/Common/Codec/common_dsp_rtcd.o",
                                               "Lib/Common/Codec/EbUtility.o")]
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "tf_install")
        r = subprocess.run(["gcc", "-O1", "-fPIC", "-ffunction-sections", "-fdata-sections"] + STRICT + INC +
                           [os.path.join(ROOT, "tests", "tf_install.c")] + objs +
                           ["-o", exe, "-Wl,--gc-sections", "-L" + LIB_DIR, "-lsvtgpu", "-Wl,-rpath," + LIB_DIR, "-ldl",
                            "-lm", "-lpthread"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split() == ["before", "0/9", "after", "9/9"], res.stdout
