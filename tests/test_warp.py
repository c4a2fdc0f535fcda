"""AV1 warped-motion prediction without a GPU: the numpy restatement (tests/warp_cases.py) against every record of the
reference's fixture (tests/golden/warp.bin), the library's filter table and svtgpu_warp_shear_params against the same
fixture, the ABI, and SvtGpuWarpBlock's layout."""
import ctypes

import numpy as np
import pytest

import svtgpu
import warp_cases as wc

UNITS = wc.unit_cases()
BATCHES = wc.batch_cases()


def test_tables_match_the_reference():
    g = wc.fixture()
    np.testing.assert_array_equal(svtgpu.warp_filter_table(), g["filter"])
    assert g["filter"].shape == (193, 8) and (g["filter"].sum(1) == 128).all()
    # the divisor table is computed in csrc/warp_params.h: 2^22 / (256 + f), rounded
    want = [((1 << 22) + ((256 + f) >> 1)) // (256 + f) for f in range(257)]
    assert [int(v) for v in g["div_lut"]] == want


def test_shear_params_match_the_reference():
    g = wc.fixture()
    assert (g["shear_kinds"] > 0).all() and len(g["shear_in"]) == int(g["shear_kinds"][11])
    for mat, want in zip(g["shear_in"], g["shear_out"]):
        want = [int(v) for v in want]
        rc, abgd = svtgpu.warp_shear_params(mat)
        assert rc == want[0], list(mat)
        if mat[2] > 0:  # the reference leaves a model with mat[2] <= 0 untouched
            assert abgd == want[1:], list(mat)
        assert wc.shear_params(mat) == (want[0], want[1:]), list(mat)


def test_shear_params_refuse_null_pointers():
    L = svtgpu.lib()
    m, o = (ctypes.c_int32 * 6)(0, 0, 65536, 0, 0, 65536), (ctypes.c_int16 * 4)()
    assert L.svtgpu_warp_shear_params(None, o) == -1 and L.svtgpu_warp_shear_params(m, None) == -1
    assert L.svtgpu_warp_filter_table(None, None) == -1
    assert L.svtgpu_warp_shear_params(m, o) == 1 and list(o) == [0, 0, 0, 0]


@pytest.mark.parametrize("i", range(len(UNITS)))
def test_restatement_matches_unit_records(i):
    c = UNITS[i]
    out, conv = wc.unit_expected(c)
    np.testing.assert_array_equal(out, c["out"], err_msg=c["name"])
    if c["mode"]:
        np.testing.assert_array_equal(conv, c["conv"], err_msg=c["name"] + " conv")
    for s in (0, 1):
        assert wc.shear_params(c["mat"][s]) == (1, [int(v) for v in c["abgd"][s]]), c["name"]


def test_unit_records_cover_what_the_issue_names():
    g = wc.fixture()
    assert len(g["unit_kinds"]) == 16 and (g["unit_kinds"] > 0).all()  # the origin outside the plane on every side among them
    assert {(c["pw"], c["ph"]) for c in UNITS} == {(8, 8), (8, 16), (16, 8), (32, 8)}
    assert {(c["bd"], c["mode"]) for c in UNITS} == {(b, m) for b in (8, 10, 12) for m in (0, 1, 2)}
    assert {c["ss"] for c in UNITS} == {0, 1} and {c["content"] for c in UNITS} == {0, 1, 2, 3, 4}
    for bd in (8, 10, 12):  # the split reference holds ten bits, so a 12-bit output cannot reach its upper clip
        outs = np.concatenate([c["out"].ravel() for c in UNITS if c["bd"] == bd])
        assert outs.min() == 0 and (bd == 12 or outs.max() == (1 << bd) - 1), bd


def test_the_intermediate_reaches_its_analytic_ends_and_fits_sixteen_bits():
    """The horizontal intermediate over all unit records, by the restatement (which the records hold to the C): per bit depth
    its minimum and maximum are what the generator recorded from its own restatement of the C's loop, and both are the
    analytic ends: the offset plus max times the table's smallest sum of negative taps / largest sum of positive taps,
    rounded by reduce_bits_horiz.  The maximum is below 2^16, which the kernels' 16-bit LDS intermediate relies on; so is the
    bound for full-range 12-bit samples, which the split reference cannot carry.  Both ends of the filter table are reached by
    the horizontal pass; the vertical one reaches row 0 and its last, 176."""
    g = wc.fixture()
    T = wc.table()
    neg, pos = int(np.where(T < 0, T, 0).sum(1).min()), int(np.where(T > 0, T, 0).sum(1).max())
    all_rows = {"h": set(), "v": set()}
    for k, bd in enumerate((8, 10, 12)):
        stats = {}
        for c in UNITS:
            if c["bd"] == bd:
                wc.unit_expected(c, stats)
        r0, _ = wc.conv_rounds(bd, 0)
        rbh, maxv = wc.horiz_bits(bd, r0, bd > 8), (1 << min(bd, 10)) - 1
        lo, hi = [((1 << (bd + 6)) + t * maxv + ((1 << rbh) >> 1)) >> rbh for t in (neg, pos)]
        assert stats["tmp"] == (lo, hi), (bd, stats["tmp"], lo, hi)
        assert [int(v) for v in g["unit_tmp"][k]] == [lo, hi, neg, pos], bd
        assert hi < 1 << 16 and ((1 << (bd + 6)) + pos * ((1 << bd) - 1) + ((1 << rbh) >> 1)) >> rbh < 1 << 16, bd
        all_rows["h"] |= stats["h"]
        all_rows["v"] |= stats["v"]
    assert {0, 192} <= all_rows["h"] and 0 in all_rows["v"] and max(all_rows["v"]) == 176


@pytest.mark.parametrize("c", BATCHES, ids=[c["name"] for c in BATCHES])
def test_restatement_matches_batch_records(c):
    big = sum(b["w"] == 128 and b["h"] == 64 for b in c["blocks"])
    assert (np.delete(c["kinds"], 22) > 0).all() and int(c["kinds"][22]) == big
    got = wc.predict_batch(c["refs"], c["blocks"], c["bd"], c["w"], c["h"], c["chroma"])
    for p, want in enumerate(c["pred"]):
        np.testing.assert_array_equal(got[p], want, err_msg="%s plane %d" % (c["name"], p))
    small = [b for b in c["blocks"] if b["w"] < 16 or b["h"] < 16]
    assert len(small) == int(c["kinds"][13]) and small  # luma only: their chroma is no part of the call
    if c["chroma"]:
        for b in small:
            assert (c["pred"][1][b["y"] >> 1:(b["y"] + b["h"]) >> 1, b["x"] >> 1:(b["x"] + b["w"]) >> 1] == 0).all()


def test_abi_version_and_symbols():
    L = svtgpu.lib()
    assert L.svtgpu_abi_version() >= 18
    names = {"svtgpu_warp_shear_params", "svtgpu_warp_filter_table", "svtgpu_av1_warp_affine", "svtgpu_av1_highbd_warp_affine",
             "svtgpu_warp_predict_batch"}
    assert names <= set(svtgpu.declared_symbols())
    for n in names:
        assert getattr(L, n).argtypes is not None, n


def test_warp_block_layout():
    B = svtgpu.WarpBlock
    assert ctypes.sizeof(B) == 64
    offs = {"x": 0, "y": 2, "w_log2": 4, "h_log2": 5, "ref0": 6, "ref1": 7, "dist_wtd": 8, "fwd_offset": 9, "bck_offset": 10,
            "reserved0": 11, "wmmat0": 12, "wmmat1": 36, "reserved": 60}
    for name, o in offs.items():
        assert getattr(B, name).offset == o, name


def test_batch_refusals_that_need_no_device():
    """The argument checks that come before the state is looked at."""
    L = svtgpu.lib()
    pl, b = svtgpu.TfPlanes(), (svtgpu.WarpBlock * 1)()
    refs = (svtgpu.TfPlanes * 1)()
    assert L.svtgpu_warp_predict_batch(None, refs, 1, b, 1, 8, 1, ctypes.byref(pl), None) == -1
    assert L.svtgpu_warp_predict_batch(None, refs, 27, b, 1, 8, 1, ctypes.byref(pl), None) == -3


def test_a_128x64_block_is_predicted_with_chroma_at_both_depths():
    with_big = {(c["bd"], c["chroma"]) for c in BATCHES if c["kinds"][22] > 0}
    assert {(8, 1), (10, 1), (10, 0)} <= with_big
