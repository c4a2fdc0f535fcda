"""AV1 inter-intra prediction (CPU): the numpy restatement of tests/interintra_cases.py against every record of the
reference's fixture -- predictor planes, the prepared edges and predictor choices recorded inside build_intra_predictors, the
search distortions, the blends, the intra predictors -- the fixture's coverage counters, svtgpu_interintra_smooth_mask, the
symbols, the ABI number, the struct layout, and what the batch entries refuse before they look at a state.  (Every other
refusal needs a state, which needs a device: tests/test_interintra_gpu.py.)"""
import ctypes

import numpy as np
import pytest

import interintra_cases as ic
import svtgpu

RECORDS = ic.records()


@pytest.mark.parametrize("c", RECORDS, ids=[c["name"] for c in RECORDS])
def test_restatement_matches_every_prediction_record(c):
    got = ic.predict_batch(c["refs"], c["pad"], c["blocks"], c["edges"], c["bd"], c["w"], c["h"], c["chroma"], border=(c["pad"], c["pad"]))
    for p, want in enumerate(c["pred"]):
        np.testing.assert_array_equal(got[p], want, err_msg="%s plane %d" % (c["name"], p))


@pytest.mark.parametrize("c", RECORDS, ids=[c["name"] for c in RECORDS])
def test_edge_preparation_and_predictor_choice_match_the_references_own(c):
    """What the recorders saw inside build_intra_predictors: the predictor it chose per plane and the prepared arrays it
    handed over (the side a predictor does not read is not compared; the early fill has neither)."""
    for b in c["blocks"]:
        for p in range(3 if c["chroma"] else 1):
            ss = int(p > 0)
            pw, ph = b["w"] >> ss, b["h"] >> ss
            above, left = ic.block_edges(b, c["edges"], p)
            _, kind, a, l = ic.intra(b["mode"], above, left, b["n_top"][ss], b["n_left"][ss], pw, ph, c["bd"])
            assert kind == b["kinds"][p], (c["name"], b, p)
            pa, pl = ic.block_edges(b, c["prep"], p)
            if kind not in (5, 7):
                np.testing.assert_array_equal(a, pa, err_msg="%s above of plane %d of %r" % (c["name"], p, b))
            if kind not in (4, 7):
                np.testing.assert_array_equal(l, pl, err_msg="%s left of plane %d of %r" % (c["name"], p, b))
        if not c["chroma"]:
            assert b["kinds"][1:] == (-1, -1)


@pytest.mark.parametrize("c", RECORDS, ids=[c["name"] for c in RECORDS])
def test_restatement_matches_every_search_record(c):
    got = ic.mode_sse(c["refs"], c["pad"], c["blocks"], c["edges"], c["bd"], c["w"], c["h"], c["src"], border=(c["pad"], c["pad"]))
    np.testing.assert_array_equal(got, c["sse"], err_msg=c["name"])


def test_blend_restatement_matches_every_record():
    cases = ic.blend_cases()
    assert {(c["hbd"], c["subw"], c["subh"]) for c in cases} == {(a, b, d) for a in (0, 1) for b in (0, 1) for d in (0, 1)}
    assert {1, 128} <= {c["w"] for c in cases} and {1, 128} <= {c["h"] for c in cases} and {8, 10, 12} == {c["bd"] for c in cases}
    for c in cases:
        np.testing.assert_array_equal(ic.blend_a64_mask(c["src0"], c["src1"], c["mask"], c["subw"], c["subh"]), c["out"], err_msg=c["name"])
    assert any(int(c["out"].max()) == (1 << c["bd"]) - 1 and int(c["out"].min()) == 0 for c in cases)


def test_intra_restatement_matches_every_record():
    cases = ic.intra_cases()
    assert {(c["hbd"], c["kind"], c["w"], c["h"]) for c in cases} == \
        {(a, k, w, h) for a in (0, 1) for k in range(7) for (w, h) in ic.PLANE_SIZES}
    for c in cases:
        got = ic.intra_by_kind(c["kind"], c["above"].astype(np.int64), c["left"].astype(np.int64), c["bd"])
        np.testing.assert_array_equal(got, c["out"], err_msg=c["name"])


def test_fixture_holds_the_cases():
    k = ic.counts()
    for name, v in k.items():
        assert all(v), name
    blocks = [(c, b) for c in RECORDS for b in c["blocks"]]
    assert {(b["w"], b["h"]) for _, b in blocks} == set(ic.SIZES)
    assert {(c["bd"], b["w"], b["h"]) for c, b in blocks} == {(bd, w, h) for bd in (8, 10) for (w, h) in ic.SIZES}
    assert {b["mode"] for _, b in blocks} == {0, 1, 2, 3} and {b["use_wedge"] for _, b in blocks} == {0, 1}
    assert {b["wedge_index"] for _, b in blocks if b["use_wedge"]} == set(range(16))
    cls = lambda n, side: 0 if n == 0 else 1 if n < side else 2
    assert {(cls(b["n_top"][0], b["w"]), cls(b["n_left"][0], b["h"])) for _, b in blocks} == {(a, d) for a in range(3) for d in range(3)}
    assert {b["kinds"][0] for _, b in blocks} == set(range(8))
    assert {c["content"] for c in RECORDS} == {0, 1, 2, 3} and {c["chroma"] for c in RECORDS} == {0, 1}
    assert all(c["w"] <= 96 and c["h"] <= 64 for c in RECORDS)


def test_smooth_masks():
    L = svtgpu.lib()
    for (w, h) in ic.PLANE_SIZES:
        for mode in range(4):
            np.testing.assert_array_equal(svtgpu.interintra_smooth_mask(w, h, mode), ic.smooth_mask(mode, w, h), err_msg="%dx%d %d" % (w, h, mode))
    # against the records: a smooth block of a zero-MV, all-max inter prediction over all-zero edges would need a record of its
    # own; the records' predictor planes hold the masks through test_restatement_matches_every_prediction_record instead.
    m = np.zeros(32 * 32, np.uint8)
    for w, h, mode in ((4, 16, 0), (16, 4, 0), (64, 64, 0), (2, 2, 0), (8, 12, 0), (8, 8, 4), (8, 8, -1), (0, 8, 0), (32, 8, 1)):
        assert L.svtgpu_interintra_smooth_mask(w, h, mode, m.ctypes.data) == -1, (w, h, mode)
    assert L.svtgpu_interintra_smooth_mask(8, 8, 0, None) == -1


def test_abi_version_symbols_and_layout():
    L = svtgpu.lib()
    assert L.svtgpu_abi_version() == 19
    for name in ("svtgpu_interintra_predict_batch", "svtgpu_interintra_mode_sse_batch", "svtgpu_interintra_smooth_mask",
                 "svtgpu_aom_blend_a64_mask", "svtgpu_aom_highbd_blend_a64_mask", "svtgpu_aom_intra_predictor",
                 "svtgpu_aom_highbd_intra_predictor"):
        assert hasattr(L, name), name
        assert name in svtgpu.declared_symbols(), name
    B = svtgpu.InterIntraBlock
    assert ctypes.sizeof(B) == 32
    assert [getattr(B, f).offset for f in ("x", "y", "w_log2", "h_log2", "ref", "filter_x", "filter_y", "mode", "use_wedge",
                                           "wedge_index", "mv_x", "mv_y", "n_top", "n_left", "edge_offset", "reserved")] == \
        [0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 18, 20, 24]
    b = B.make(8, 16, 16, 32, 2, (-5, 7), 1, 3, 3, 1, 15, (16, 8), (32, 16), 77)
    assert (b.w_log2, b.h_log2, b.mode, b.use_wedge, b.wedge_index, b.edge_offset, list(b.n_top), list(b.n_left)) == \
        (4, 5, 3, 1, 15, 77, [16, 8], [32, 16]) and bytes(b.reserved) == bytes(8)


def test_refusals_that_need_no_state():
    """n_refs > 26 is refused as unsupported before anything is looked at; a null state, pred or result pointer as an
    invalid argument: no device is touched."""
    L = svtgpu.lib()
    planes, blk, edges = (svtgpu.TfPlanes * 27)(), (svtgpu.InterIntraBlock * 1)(), np.zeros(64, np.uint8)
    assert L.svtgpu_interintra_predict_batch(None, planes, 27, 0, 0, blk, 1, edges.ctypes.data, 64, 8, 1, ctypes.byref(planes[0]), None) == -3
    assert L.svtgpu_interintra_mode_sse_batch(None, planes, 27, 0, 0, blk, 1, edges.ctypes.data, 64, 8, None, 0, None, None) == -3
    assert L.svtgpu_interintra_predict_batch(None, planes, 1, 0, 0, blk, 1, edges.ctypes.data, 64, 8, 1, ctypes.byref(planes[0]), None) == -1
    assert L.svtgpu_interintra_mode_sse_batch(None, planes, 1, 0, 0, blk, 1, edges.ctypes.data, 64, 8, None, 0, None, None) == -1
