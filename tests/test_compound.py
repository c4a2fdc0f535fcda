"""AV1 compound prediction without a GPU: the numpy restatement (tests/compound_cases.py) against every record of the
reference's fixture, bit-exact; the fixture's coverage; the library's distance weights (csrc/compound_weights.h through
the host-only svtgpu_dist_wtd_weights) against the reference's table walk; the ABI; refusal of bad arguments."""
import ctypes
import os

import numpy as np
import pytest

import compound_cases as cc
import svtgpu

BLOCKS = cc.block_cases()
BATCHES = cc.batch_cases()
SYMBOLS = tuple("svtgpu_av1_%sjnt_convolve_%s" % (hb, f) for hb in ("", "highbd_") for f in svtgpu.COMPOUND_FORMS) + \
    ("svtgpu_dist_wtd_weights", "svtgpu_compound_predict_batch")
GOLDEN_DIR = os.path.dirname(cc.GOLDEN)


def test_restatement_matches_every_block_record():
    for c in BLOCKS:
        conv, out = cc.block_expected(c)
        np.testing.assert_array_equal(conv, c["conv"], err_msg=c["name"] + " conv_dst")
        np.testing.assert_array_equal(out, c["out"], err_msg=c["name"])
        assert (int(out.min()), int(out.max())) == c["mm"], c["name"]


@pytest.mark.parametrize("c", BATCHES, ids=[c["name"] for c in BATCHES])
def test_restatement_matches_every_batch_record(c):
    # the fixture's borders are edge-replicated: clamped at the border the samples are the reference's
    got = cc.predict_batch(c["refs"], c["pad"], c["blocks"], c["bd"], c["w"], c["h"], c["chroma"], border=(c["pad"], c["pad"]))
    for p, want in enumerate(c["pred"]):
        np.testing.assert_array_equal(got[p], want, err_msg="%s plane %d" % (c["name"], p))


def test_restated_weights_match_the_reference():
    t = cc.fixture()["weights"]
    assert t.shape == (34, 34, 2, 2)
    for d0 in range(34):
        for d1 in range(34):
            for o in range(2):
                assert cc.dist_wtd_weights(d0, d1, o) == tuple(int(v) for v in t[d0, d1, o]), (d0, d1, o)


def test_library_weights_match_the_reference_and_refuse_bad_arguments():
    t = cc.fixture()["weights"]
    n = 0
    for d0 in range(34):
        for d1 in range(34):
            for o in range(2):
                assert svtgpu.dist_wtd_weights(d0, d1, o) == tuple(int(v) for v in t[d0, d1, o]), (d0, d1, o)
                n += 1
    assert n == 2312
    assert {tuple(int(v) for v in t[a, b, o]) for a in range(34) for b in range(34) for o in range(2)} == \
        {m[1:] for m in cc.MODES[1:]}
    L = svtgpu.lib()
    f, b = ctypes.c_int32(77), ctypes.c_int32(77)
    for bad in ((-1, 3, 0), (3, -1, 0), (3, 3, 2), (3, 3, -1)):
        assert L.svtgpu_dist_wtd_weights(*bad, ctypes.byref(f), ctypes.byref(b)) == -1, bad
    assert L.svtgpu_dist_wtd_weights(3, 3, 0, None, ctypes.byref(b)) == -1
    assert L.svtgpu_dist_wtd_weights(3, 3, 0, ctypes.byref(f), None) == -1
    assert (f.value, b.value) == (77, 77)
    assert svtgpu.dist_wtd_weights(1000, 1, 0) == svtgpu.dist_wtd_weights(31, 1, 0)  # clamped to MAX_FRAME_DISTANCE


def test_fixture_covers_what_the_issue_lists():
    assert {(c["w"], c["h"]) for c in BLOCKS} == set(cc.SIZES) | set(cc.CHROMA_ONLY_SIZES)
    for w, h in set(cc.SIZES) | set(cc.CHROMA_ONLY_SIZES):
        forms = {c["form"] for c in BLOCKS if (c["w"], c["h"]) == (w, h)}
        assert forms == {0, 1, 2, 3} if w * h < 1024 else forms, (w, h)
    assert {c["bd"] for c in BLOCKS} == {8, 10, 12} and {c["kind"] for c in BLOCKS} == {0, 1, 2, 3}
    assert {c["mode"] for c in BLOCKS} == set(cc.MODES)
    for hbd in (False, True):
        for form in range(4):
            mine = [c for c in BLOCKS if (c["bd"] > 8) == hbd and c["form"] == form]
            assert {c["content"] for c in mine} == {0, 1, 2, 3}, (hbd, form)
    for bd in (8, 10, 12):
        mine = [c for c in BLOCKS if c["bd"] == bd]
        assert any(c["mm"][0] == 0 for c in mine) and any(c["mm"][1] == (1 << bd) - 1 for c in mine), bd
    assert [(c["bd"], c["chroma"]) for c in BATCHES] == [(8, 1), (10, 1), (8, 0)]
    for c in BATCHES:
        assert (c["w"], c["h"], c["n_refs"], c["pad"]) == (256, 192, 3, 80) and all(k > 0 for k in c["kinds"]), c["name"]
        assert {(b["w"], b["h"]) for b in c["blocks"]} == set(cc.SIZES)
        cover = np.zeros((c["h"], c["w"]), int)
        for b in c["blocks"]:
            cover[b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]] += 1
        assert (cover == 1).all()
    assert BATCHES[2]["blocks"] == BATCHES[0]["blocks"]
    assert os.path.getsize(cc.GOLDEN) <= os.path.getsize(os.path.join(GOLDEN_DIR, "interp.bin"))


def test_abi_version_and_symbols():
    L = svtgpu.lib()
    assert L.svtgpu_abi_version() >= 16
    for n in SYMBOLS:
        assert hasattr(L, n) and n in svtgpu.declared_symbols(), n
    assert ctypes.sizeof(svtgpu.CompoundBlock) == 32
    assert svtgpu.CompoundBlock.mv0_x.offset == 8 and svtgpu.CompoundBlock.filter_x.offset == 16
    assert svtgpu.CompoundBlock.bck_offset.offset == 20


def test_predict_batch_refuses_bad_arguments():
    """-1 / -3 before a device is asked for (this test runs without one)."""
    L = svtgpu.lib()
    some = ctypes.c_void_p(4096)  # never dereferenced: refused first
    pl, bl = svtgpu.TfPlanes(), svtgpu.CompoundBlock()
    ok = dict(state=some, refs=ctypes.byref(pl), n=1, bx=80, by=80, blocks=ctypes.byref(bl), nb=1, bd=8, chroma=1,
              pred=ctypes.byref(pl))

    def call(**kw):
        a = dict(ok, **kw)
        return L.svtgpu_compound_predict_batch(a["state"], a["refs"], a["n"], a["bx"], a["by"], a["blocks"], a["nb"], a["bd"],
                                               a["chroma"], a["pred"], None)
    assert call(state=None) == -1 and call(refs=None) == -1 and call(blocks=None) == -1 and call(pred=None) == -1
    assert call(n=-1) == -1 and call(nb=-1) == -1 and call(bx=-1) == -1 and call(by=-4) == -1
    for bd in (0, 9, 12, 16):
        assert call(bd=bd) == -1, bd
    assert call(n=27) == -3 and call(n=27, state=None) == -3  # SVTGPU_ERR_UNSUPPORTED, as the temporal filter's entries
