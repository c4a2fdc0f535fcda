"""AV1 OBMC prediction (CPU): the numpy restatement of tests/obmc_pred_cases.py against every record of the reference's
fixture, the fixture's coverage counters, svtgpu_obmc_mask, the ABI number and the two struct layouts."""
import ctypes

import numpy as np
import pytest

import obmc_pred_cases as oc
import svtgpu

RECORDS = oc.records()


@pytest.mark.parametrize("c", RECORDS, ids=[c["name"] for c in RECORDS])
def test_restatement_matches_every_record(c):
    got = oc.predict_batch(c["refs"], c["pad"], c["blocks"], c["bd"], c["w"], c["h"], c["chroma"], border=(c["pad"], c["pad"]))
    for p, want in enumerate(c["pred"]):
        np.testing.assert_array_equal(got[p], want, err_msg="%s plane %d" % (c["name"], p))


def test_depth_mismatch_records_differ_from_the_plain_clamp():
    """The records over noise that goes on into the border: with the across clamp's spel taken from extent >> 1 the chroma
    of a side of 8 comes out different, so the records hold the rule."""
    n = 0
    for c in RECORDS:
        if c["content"] != 4:
            continue
        plain = oc.predict_batch(c["refs"], c["pad"], c["blocks"], c["bd"], c["w"], c["h"], 1, border=(c["pad"], c["pad"]), plain_clamp=True)
        np.testing.assert_array_equal(plain[0], c["pred"][0])  # luma: the two clamps are the same
        n += any((a != b).any() for a, b in zip(plain[1:], c["pred"][1:]))
    assert n >= 8


def test_fixture_holds_the_cases():
    k = oc.counts()
    assert all(k["size8"]) and all(k["size10"]) and all(k["size_nochroma"])
    assert all(k["size10_chroma"])
    assert all(k["fx"]) and all(k["fy"]) and all(k["n_above"]) and all(k["n_left"])
    for name in ("stopped", "gap", "wider", "pair4", "row0", "col0", "right", "bottom", "compound_nb", "lo", "hi", "ws_zero", "ws_max",
                 "ws_neg"):
        assert k[name][0] > 0, name
    assert all(k["mismatch"]) and all(k["tap4"])
    assert {(b["w"], b["h"]) for c in RECORDS for b in c["blocks"]} == set(oc.SIZES)
    assert {len(b["above"]) for c in RECORDS for b in c["blocks"]} == {0, 1, 2, 3, 4}
    assert {len(b["left"]) for c in RECORDS for b in c["blocks"]} == {0, 1, 2, 3, 4}
    assert {c["content"] for c in RECORDS} == {0, 1, 2, 3, 4}


WM = [(c, j, ws, mk) for c in RECORDS for (j, ws, mk) in c["wm"]]


def test_weighted_source_restatement_matches_every_record():
    assert {(c["blocks"][j]["w"], c["blocks"][j]["h"]) for c, j, _, _ in WM} == set(oc.SIZES)
    lo = hi = neg = 0
    for c, j, ws, mk in WM:
        src = oc.source_luma(c["index"], c["w"], c["h"], c["content"])
        got_ws, got_mk = oc.weighted_src(c["refs"], c["pad"], c["blocks"][j], src, c["w"], c["h"], border=(c["pad"], c["pad"]))
        np.testing.assert_array_equal(got_ws, ws, err_msg="%s block %d wsrc" % (c["name"], j))
        np.testing.assert_array_equal(got_mk, mk, err_msg="%s block %d mask" % (c["name"], j))
        lo, hi, neg = lo + (ws == 0).any(), hi + (ws == 255 * 4096).any(), neg + (ws < 0).any()
    assert lo and hi and neg  # the analytic ends of wsrc, and below zero


def test_blend_restatement_matches_every_record():
    cases = oc.blend_cases()
    assert {c["fn"] for c in cases} == set(range(6)) and {1, 128} <= {c["w"] for c in cases} and {1, 128} <= {c["h"] for c in cases}
    for c in cases:
        np.testing.assert_array_equal(oc.blend(c), c["out"], err_msg=c["name"])
    assert any(int(c["out"].max()) == (1 << c["bd"]) - 1 and int(c["out"].min()) == 0 for c in cases)


def test_lists_in_the_fixture_pass_the_headers_rules():
    for c in RECORDS:
        for b in c["blocks"]:
            for key, side, org in (("above", b["w"], b["y"]), ("left", b["h"], b["x"])):
                end = 0
                assert len(b[key]) <= oc.MAX_NEIGHBOURS[side] and (org > 0 or not b[key])
                for n in b[key]:
                    assert n["size"] in (2, 4, 8, 16) and n["rel"] % 2 == 0 and n["rel"] >= end and n["rel"] + n["size"] <= side // 4
                    end = n["rel"] + n["size"]


def test_masks():
    L = svtgpu.lib()
    for length, want in oc.MASKS.items():
        assert svtgpu.obmc_mask(length) == want
    m = ctypes.c_void_p()
    for bad in (0, 3, 5, 64, -1, 128):
        assert L.svtgpu_obmc_mask(bad, ctypes.byref(m)) == -1
    assert L.svtgpu_obmc_mask(8, None) == -1


def test_abi_version_and_layouts():
    L = svtgpu.lib()
    assert L.svtgpu_abi_version() == 19
    for name in ("svtgpu_obmc_predict_batch", "svtgpu_obmc_mask", "svtgpu_obmc_weighted_src_batch", "svtgpu_obmc_set_items_device_wm",
                 "svtgpu_aom_blend_a64_vmask", "svtgpu_aom_blend_a64_hmask", "svtgpu_aom_highbd_blend_a64_vmask_16bit",
                 "svtgpu_aom_highbd_blend_a64_hmask_16bit", "svtgpu_aom_highbd_blend_a64_vmask_8bit",
                 "svtgpu_aom_highbd_blend_a64_hmask_8bit"):
        assert hasattr(L, name), name
    N, B = svtgpu.ObmcNeighbour, svtgpu.ObmcBlock
    assert ctypes.sizeof(N) == 8 and [getattr(N, f).offset for f in ("rel", "size", "ref", "filters", "mv_x", "mv_y")] == [0, 1, 2, 3, 4, 6]
    assert ctypes.sizeof(B) == 96
    assert [getattr(B, f).offset for f in ("x", "y", "w_log2", "h_log2", "ref", "filter_x", "filter_y", "n_above", "n_left",
                                           "reserved0", "mv_x", "mv_y", "wm_offset", "reserved", "nb")] == \
        [0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 20, 32]
