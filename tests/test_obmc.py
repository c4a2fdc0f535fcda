"""The OBMC distortion family without a GPU: the numpy restatement of tests/obmc_cases.py against every record of the
reference's fixture (the checker the GPU tests rely on), the library's exports, the shim prototypes against the
reference's RTCD pointers (compile-only), and the install point against the reference's own init_fn_ptr."""
import glob
import os
import subprocess
import tempfile

import numpy as np
import pytest

import obmc_cases as oc
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


@pytest.mark.parametrize("k", range(22))
def test_restatement_matches_block_records(k):
    assert tuple(int(v) for v in oc.fixture()["sizes"][k]) == oc.SIZES[k]
    for case in range(4):
        win, wsrc, mask, want = oc.block_case(k, case)
        np.testing.assert_array_equal(oc.block_expected(win, wsrc, mask), want, err_msg="size %d case %d" % (k, case))


def test_block_cases_are_what_they_claim():
    """The constant cases give +-255 per sample; the boundary case sits on the rounding boundary."""
    for k, (w, h) in enumerate(oc.SIZES):
        _, _, _, plus = oc.block_case(k, 2)
        _, _, _, minus = oc.block_case(k, 3)
        n = w * h
        assert plus[0] == minus[0] == 255 * n and plus[2] == minus[2] == 255 * 255 * n and plus[1] == minus[1] == 0
        win, wsrc, mask, _ = oc.block_case(k, 1)
        d = wsrc.astype(np.int64) - win[:h, :w].astype(np.int64) * mask
        r = (np.abs(d) - 2048) % 4096  # distance of |d| from 2048 + k * 4096
        assert (np.minimum(r, 4096 - r) <= 1).all() and (d < 0).any() and (d > 0).any()


def test_restatement_matches_walk_records():
    g = oc.fixture()
    frames = g["walk_frames"]
    cases = oc.walk_cases()
    assert len(cases) >= 20
    moves = []
    for i, (it, wsrc, mask, cost, res) in enumerate(cases):
        padded, pad = oc.pad_frame(frames[it["frame"]])
        col, row, best, var, sse, n = oc.walk(padded, pad, it, wsrc, mask, cost)
        assert (col, row, var, sse) == tuple(int(v) & 0xFFFFFFFF if j >= 2 else int(v) for j, v in enumerate(res[:4])), i
        if it["cost_mode"] == 0:  # the return adds svt_aom_mv_err_cost_light of the final MV (av1me.c:229-235, 716)
            light = 1296 + 50 * (abs(col * 8 - it["ref_mv_col"]) + abs(row * 8 - it["ref_mv_row"]))
            assert int(res[4]) == var + light, i
        moves.append(n)
    # the cases cover a walk that stops at once and walks that run their whole range
    assert 0 in moves and 16 in moves and 8 in moves, moves


def test_library_exports_obmc_symbols():
    names = ["svtgpu_aom_obmc_%s%dx%d" % (k, w, h) for k in ("sad", "variance", "sub_pixel_variance")
             for w, h in oc.SIZES]
    names += ["svtgpu_obmc_batch_create", "svtgpu_obmc_batch_destroy", "svtgpu_obmc_set_items", "svtgpu_obmc_search",
              "svtgpu_obmc_read"]
    assert len(names) == 71
    out = subprocess.run(["nm", "-D", "--defined-only", svtgpu.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    missing = [n for n in names if n not in exported]
    assert not missing, missing
    assert all(n in svtgpu._SIGS and n in svtgpu.declared_symbols() for n in names)


@pytest.mark.skipif(not os.path.isdir(S), reason="reference headers not present")
def test_obmc_shim_prototypes_match_reference_pointers():
    r = subprocess.run(["gcc", "-fsyntax-only"] + STRICT + INC + [os.path.join(ROOT, "tests", "obmc_bind.c")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(not (os.path.isdir(S) and os.path.exists(os.path.join(REF_OBJ, "Lib/Encoder/Codec/av1me.o"))),
                    reason="oracle/_ref/obj not built (needs /root/reference)")
def test_obmc_install_point_before_init_fn_ptr():
    """Installed before init_fn_ptr every osdf / ovf / osvf entry is a libsvtgpu symbol; installed after, none is."""
    objs = [os.path.join(REF_OBJ, p) for p in
            ("Lib/Encoder/Codec/av1me.o", "Lib/Encoder/C_DEFAULT/EbComputeSAD_C.o", "Lib/Encoder/C_DEFAULT/variance.o",
             "Lib/Encoder/Codec/EbPsnr.o", "Lib/Encoder/Codec/EbEncInterPrediction.o",
             "Lib/Common/C_DEFAULT/EbPictureOperators_C.o", "Lib/Common/Codec/EbPictureOperators.o",
             "Lib/Common/Codec/EbCdef.o", "Lib/Encoder/Codec/EbEncCdef.o", "Lib/Common/Codec/common_dsp_rtcd.o",
             "Lib/Encoder/Codec/aom_dsp_rtcd.o", "Lib/Common/Codec/EbUtility.o")]
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "obmc_install")
        r = subprocess.run(["gcc", "-O1", "-fPIC", "-ffunction-sections", "-fdata-sections"] + STRICT + INC +
                           [os.path.join(ROOT, "tests", "obmc_install.c")] + objs +
                           ["-o", exe, "-Wl,--gc-sections", "-L" + LIB_DIR, "-lsvtgpu", "-Wl,-rpath," + LIB_DIR, "-ldl",
                            "-lm", "-lpthread"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split() == ["documented", "66/66", "late", "0/66"], res.stdout


def test_extreme_batch_reaches_its_points():
    """obmc_cases.extreme_batch on the restatement: the flat items stay on the clamped start with every neighbour's SAD equal
    to the start's; on the stripes the two neighbours across the stripes tie, the first in NEIGHBORS order takes over, and
    the walk with that pair swapped ends elsewhere; the full-magnitude items start on 255 * w * h, walk their whole range,
    and with cost mode 1 form bits * sad_per_bit beyond 2^32."""
    frames, items, wsrcs, masks, costs, kinds = oc.extreme_batch()
    assert len(items) == 24 and len(frames) == 4 and all(f.shape == (136, 192) for f in frames)
    for kind in ("flat", "v_stripes", "h_stripes", "full"):
        sub = [it for it, k in zip(items, kinds) if k == kind]
        assert {(it["w"], it["h"]) for it in sub} == set(oc.EXTREME_SIZES), kind
        assert {it["cost_mode"] for it in sub} == {0, 1} and {it["search_diag"] for it in sub} == {0, 1}, kind
    padded = [oc.pad_frame(f) for f in frames]
    outside = 0
    for i, (it, ws, mk, ct, kind) in enumerate(zip(items, wsrcs, masks, costs, kinds)):
        pf, pad = padded[it["frame"]]
        col, row, best, var, sse, steps = oc.walk(pf, pad, it, ws, mk, ct)
        sc = min(max(it["mvp_col"], it["col_min"]), it["col_max"])
        sr = min(max(it["mvp_row"], it["row_min"]), it["row_max"])

        def sad(r, c):
            y, x = it["y"] + r + pad, it["x"] + c + pad
            return oc.obmc_sad(pf[y:y + it["h"], x:x + it["w"]], ws, mk)
        if kind == "flat":
            assert steps == 0 and (col, row) == (sc, sr), (i, it)
            assert {sad(sr + dr, sc + dc) for dr, dc in oc.NEIGHBORS} == {sad(sr, sc)} and sad(sr, sc) > 0, i
            outside += (sc, sr) != (it["mvp_col"], it["mvp_row"])
        elif kind in oc.SWAPPED:
            a, b = ((0, -1), (0, 1)) if kind == "v_stripes" else ((-1, 0), (1, 0))  # across the stripes; a is first in NEIGHBORS
            n = 255 * it["w"] * it["h"]
            assert sad(0, 0) == n and sad(*a) == sad(*b) == n // 2 and sad(2 * a[0], 2 * a[1]) == 0, i
            along = ((-1, 0), (1, 0)) if kind == "v_stripes" else ((0, -1), (0, 1))
            assert sad(*along[0]) == sad(*along[1]) == n  # these tie as well, at every step, and never take over
            assert (row, col, steps, var, sse) == (2 * a[0], 2 * a[1], 2, 0, 0), (i, it)
            other = oc.walk(pf, pad, it, ws, mk, ct, neighbors=oc.SWAPPED[kind])
            assert (other[1], other[0]) == (2 * b[0], 2 * b[1]) and other[2:] == (best, var, sse, steps), (i, other)
        else:
            n = 255 * it["w"] * it["h"]
            assert sad(sr, sc) == n and (n == 4177920) == (it["w"] == 128), i
            if it["cost_mode"] == 0:
                # down until the range ends or the block lies wholly in the corner; the large blocks stay near 255 * w * h
                assert steps == min(it["search_range"], it["h"]) and row == sr + steps, (i, steps)
                assert it["w"] < 64 or best > n * 3 // 4, (i, best)
            else:  # the product the restatement masks; no record of obmc.bin reaches it
                bits = int(ct[0]) + int(ct[4 + it["search_range"]]) + int(ct[4 + 3 * it["search_range"] + 1])
                assert bits * it["sad_per_bit"] > 1 << 32 and it["sad_per_bit"] == 6000, i
    assert outside == 4
    # the fixture's own walk records never reach that product: the 32-bit mask there rests on the restatement alone
    for it, _, _, cost, _ in oc.walk_cases():
        if cost is not None:
            assert int(np.max(cost[:4])) + 2 * int(np.max(cost[4:])) < (1 << 32) // it["sad_per_bit"]
