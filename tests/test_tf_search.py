"""The temporal filter's sub-pel motion search without a GPU: the numpy restatement (tests/tf_search_cases.py) against every
record the reference's C left in tests/golden/tf_search.bin, bit-exact; what the fixture covers; the ABI; refusal of bad
arguments."""
import ctypes

import numpy as np
import pytest

import svtgpu
import tf_search_cases as tc

CASES = tc.search_cases()
CHAINS = tc.chain_cases()
SYMBOLS = ("svtgpu_tf_search_frame", "svtgpu_tf_search_read", "svtgpu_tf_compensate_filter_frame")


@pytest.mark.parametrize("c", CASES + CHAINS, ids=[c["name"] for c in CASES + CHAINS])
def test_restatement_matches_the_record(c):
    got = tc.search_frame(c)
    for f in tc.FIELDS:
        np.testing.assert_array_equal(got[f], c["want"][f], err_msg="%s %s" % (c["name"], f))


@pytest.mark.parametrize("c", CHAINS, ids=[c["name"] for c in CHAINS])
def test_restatement_matches_the_chains_err32(c):
    """err32 of the use64 blocks from the recorded predictor pictures (convert_64x64_info_to_32x32_info), at the pictures'
    bit depth; and the recorded predictors are what interp_cases.predict_frame makes of the recorded motion."""
    import interp_cases as ic
    pics = tc.pictures(c["pic_bd"], c["low8"])
    got = tc.err32_of_use64(c["want"], [p[0] for p in c["pred"]], pics["cen"][0], c["pic_bd"], c["P"]["shift"])
    np.testing.assert_array_equal(got, c["err32p"])
    assert c["want"]["use64"].any() and (c["err32p"][c["want"]["use64"].astype(bool)] > 0).any()
    motion = tc.motion_dicts(tc.motion_block_arrays(c["want"])[0])
    for r in range(c["n_refs"]):
        pred = ic.predict_frame(pics["ref"][r], c["pad"], motion[r], c["pic_bd"], tc.W, tc.H, 1)
        for p in range(3):
            np.testing.assert_array_equal(pred[p], c["pred"][r][p], err_msg="%s reference %d plane %d" % (c["name"], r, p))


def test_fixture_covers_the_walk():
    """Nine parameter sets at 8 and 10 bits, every count a set can reach non-zero, the thresholds of sets 5 and 6 non-zero
    with blocks on each side, and three chains (8-bit; 10-bit searched on its 8-bit planes; 8-bit with sub_sampling_shift 1)."""
    assert len(CASES) == 18 and {(c["P"]["bd"], c["set"]) for c in CASES} == {(bd, s) for bd in (8, 10) for s in range(9)}
    for c in CASES:
        assert len(c["kinds"]) == len(tc.KINDS)
        for k, name in enumerate(tc.KINDS):
            if tc.reachable(c, k):
                assert c["kinds"][k] > 0, (c["name"], name)
            else:
                assert c["kinds"][k] == 0, (c["name"], name)
        P = c["P"]
        want = {0: ((1, 1, 1), 0, 0, 1), 1: ((2, 2, 2), 0, 0, 1), 2: ((1, 0, 0), 0, 0, 1), 3: ((1, 1, 1), 0, 1, 1),
                4: ((1, 1, 1), 1, 0, 1), 7: ((1, 1, 1), 0, 0, 0)}.get(c["set"], ((1, 1, 1), 0, 0, 1))
        assert (P["modes"], P["use_2tap"], P["shift"], P["enable8"]) == want, c["name"]
        assert (P["early"] != 0) == (c["set"] == 5) and (P["th32"] != 0) == (c["set"] == 6), c["name"]
        assert bool(c["force64"].any()) == (c["set"] == 8) and not c["force64"].all(), c["name"]
        if c["set"] == 6:  # unsplit 32x32 blocks below the threshold and searched ones above it
            e = c["want"]["err32"][(c["want"]["use64"] == 0)[..., None] & (c["want"]["split32"] == 0)]
            assert (e < P["th32"]).any() and c["want"]["split32"].any(), c["name"]
    assert [(c["pic_bd"], c["P"]["bd"], c["P"]["shift"]) for c in CHAINS] == [(8, 8, 0), (10, 8, 0), (8, 8, 1)]
    for bd in (8, 10):
        fp = CASES[0 if bd == 8 else 9]["fullpel"]
        assert max(np.abs(fp[k]).max() for k in fp) <= 2047 and max(np.abs(fp[k]).max() for k in fp) >= 150


def test_abi_version_and_symbols():
    L = svtgpu.lib()
    assert L.svtgpu_abi_version() >= 14
    for n in SYMBOLS:
        assert hasattr(L, n) and n in svtgpu.declared_symbols(), n
    F, P = svtgpu.TfFullpel, svtgpu.TfSearchParams
    assert ctypes.sizeof(F) == 352 and ctypes.sizeof(F) % 16 == 0 and ctypes.sizeof(P) == 40
    assert (F.mv64_x.offset, F.mv32_x.offset, F.mv32_y.offset, F.mv16_x.offset, F.mv16_y.offset, F.mv8_x.offset, F.mv8_y.offset,
            F.force64.offset) == (0, 4, 12, 20, 52, 84, 212, 340)
    assert (P.half_pel_mode.offset, P.eight_pel_mode.offset, P.use_2tap.offset, P.sub_sampling_shift.offset,
            P.enable_8x8_pred.offset, P.subpel_early_exit_th.offset, P.bit_depth.offset, P.pred_error_32x32_th.offset) == \
        (0, 8, 12, 16, 20, 24, 28, 32)
    assert ctypes.sizeof(svtgpu.TfMotion) == 368 and ctypes.sizeof(svtgpu.TfBlock) == 256


def test_entries_refuse_bad_arguments():
    """-1 / -3 before a device is asked for (this test runs without one)."""
    L = svtgpu.lib()
    some = ctypes.c_void_p(4096)  # never dereferenced: refused first
    pl, fp, tp = svtgpu.TfPlanes(), svtgpu.TfFullpel(), svtgpu.TfParams.make((1, 1, 1), 1080, 1, 8)

    def search(state=some, centre=ctypes.byref(pl), refs=ctypes.byref(pl), n=1, bx=72, by=72, fullpel=ctypes.byref(fp), prm=True, **kw):
        a = dict(modes=(1, 1, 1), use_2tap=0, sub_sampling_shift=0, enable_8x8_pred=1, subpel_early_exit_th=0,
                 pred_error_32x32_th=0, bit_depth=8)
        a.update(kw)
        p = svtgpu.TfSearchParams.make(**a)
        return L.svtgpu_tf_search_frame(state, centre, refs, n, bx, by, fullpel, ctypes.byref(p) if prm else None, None)
    assert search(state=None) == -1 and search(centre=None) == -1 and search(refs=None) == -1 and search(fullpel=None) == -1
    assert search(prm=False) == -1 and search(n=-1) == -1 and search(bx=-1) == -1 and search(by=-8) == -1
    for bd in (0, 9, 12, 16):
        assert search(bit_depth=bd) == -1, bd
    for modes in ((3, 1, 1), (1, -1, 1), (1, 1, 4)):
        assert search(modes=modes) == -1, modes
    assert search(use_2tap=2) == -1 and search(sub_sampling_shift=2) == -1 and search(sub_sampling_shift=-1) == -1
    assert search(enable_8x8_pred=2) == -1 and search(subpel_early_exit_th=256) == -1 and search(subpel_early_exit_th=-1) == -1
    assert search(n=27) == -3 and search(n=27, state=None) == -3
    mo, bl = svtgpu.TfMotion(), svtgpu.TfBlock()
    assert L.svtgpu_tf_search_read(None, 1, ctypes.byref(mo), ctypes.byref(bl), None) == -1
    assert L.svtgpu_tf_search_read(some, 1, None, ctypes.byref(bl), None) == -1
    assert L.svtgpu_tf_search_read(some, 1, ctypes.byref(mo), None, None) == -1
    assert L.svtgpu_tf_search_read(some, 0, ctypes.byref(mo), ctypes.byref(bl), None) == -1

    def chain(state=some, centre=ctypes.byref(pl), refs=ctypes.byref(pl), n=1, bx=72, by=72, prm=ctypes.byref(tp), shift=0,
              pred=ctypes.byref(pl), out=ctypes.byref(pl)):
        return L.svtgpu_tf_compensate_filter_frame(state, centre, refs, n, bx, by, prm, shift, pred, out, None)
    assert chain(state=None) == -1 and chain(refs=None) == -1 and chain(pred=None) == -1 and chain(prm=None) == -1
    assert chain(n=-1) == -1 and chain(bx=-1) == -1 and chain(by=-1) == -1 and chain(shift=2) == -1 and chain(shift=-1) == -1
    bad = svtgpu.TfParams.make((1, 1, 1), 1080, 1, 12)
    assert chain(prm=ctypes.byref(bad)) == -1
    assert chain(n=27) == -3 and chain(n=27, state=None) == -3
