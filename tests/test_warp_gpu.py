"""AV1 warped-motion prediction on the MI355X: the two shims against every unit record of the reference's fixture
(tests/golden/warp.bin) and svtgpu_warp_predict_batch against its three batch records, reversed and permuted, back to back
on one state, refused, and on a block whose every sample comes from the clamp.  Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import svtgpu
import warp_cases as wc
from test_compound_gpu import _dev, _host

pytestmark = pytest.mark.gpu

UNITS = wc.unit_cases()
BATCHES = wc.batch_cases()
FILL = 5


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


# ---------------------------------------------------------------------------------------------
# the two shims
# ---------------------------------------------------------------------------------------------
def _split(plane, bd):
    """The planes the shim takes: (uint8 plane, None) at 8 bits, else the high eight bits and the low two at bits 7..6."""
    if bd == 8:
        return np.ascontiguousarray(plane.astype(np.uint8)), None
    return np.ascontiguousarray((plane >> 2).astype(np.uint8)), np.ascontiguousarray(((plane & 3) << 6).astype(np.uint8))


def _shim(c, s, pred, conv, is_compound, do_average):
    bd = c["bd"]
    r0, r1 = wc.conv_rounds(bd, is_compound)
    ref, ref2 = _split(wc.unit_plane(c, s), bd)
    return svtgpu.warp_affine(c["mat"][s], ref, ref2, pred, 3, 2, c["p_col"], c["p_row"], c["pw"], c["ph"], c["ss"], c["ss"], bd, r0, r1,
                              is_compound, conv, do_average, c["mode"] == 2, c["fwd"], c["bck"], c["abgd"][s])


@pytest.mark.parametrize("i", range(len(UNITS)))
def test_shims_match_unit_records(i):
    c = UNITS[i]
    pw, ph = c["pw"], c["ph"]
    dtype = np.uint16 if c["bd"] > 8 else np.uint8
    pred = np.full((ph + 4, pw + 7), 9, dtype)       # the block at (3, 2) inside canary values
    conv = np.full((ph + 1, pw + 3), 7, np.uint16)   # conv_dst with a stride of its own
    if not c["mode"]:
        assert _shim(c, 0, pred, None, 0, 0) == 0
    else:
        assert _shim(c, 0, pred, conv, 1, 0) == 0    # first pass: conv_dst only
        np.testing.assert_array_equal(conv[:ph, :pw], c["conv"], err_msg=c["name"] + " conv_dst")
        assert (pred == 9).all(), c["name"]
        only_conv = conv.copy()
        assert _shim(c, 0, None, only_conv, 1, 0) == 0  # pred may be null on a first pass
        np.testing.assert_array_equal(only_conv, conv)
        assert _shim(c, 1, pred, conv, 1, 1) == 0    # second pass: conv_dst read, pixels written
        np.testing.assert_array_equal(conv[:ph, :pw], c["conv"], err_msg=c["name"] + " conv_dst after the second pass")
    np.testing.assert_array_equal(pred[2:2 + ph, 3:3 + pw], c["out"], err_msg=c["name"])
    assert (conv[ph:] == 7).all() and (conv[:, pw:] == 7).all(), c["name"]
    pred[2:2 + ph, 3:3 + pw] = 9
    assert (pred == 9).all(), c["name"]


def test_shims_refuse_without_a_launch():
    c = next(c for c in UNITS if c["bd"] == 8 and c["mode"] == 0)
    h = next(c for c in UNITS if c["bd"] == 10 and c["mode"] == 1)
    calls = svtgpu.lib().svtgpu_shim_calls()
    for base in (c, h):
        pred = np.full((40, 40), 9, np.uint16 if base["bd"] > 8 else np.uint8)
        conv = np.full((40, 40), 7, np.uint16)
        comp = int(base["mode"] != 0)
        for bad in (dict(pw=12), dict(ph=4), dict(pw=0), dict(ph=20), dict(pw=136), dict(ss=2), dict(p_col=-8)):
            assert _shim(dict(base, **bad), 0, pred, conv if comp else None, comp, 0) == -1, bad
        wild = dict(base, abgd=np.array([[16384, 0, 0, 0], [0, 0, 0, 0]]))            # beyond the first shear limit
        assert _shim(wild, 0, pred, conv if comp else None, comp, 0) == -1
        far = dict(base, mat=np.array([[0, 0, 2 ** 31 - 1, 0, 0, 65536], [0] * 6]))    # the projection leaves int32
        assert _shim(far, 0, pred, conv if comp else None, comp, 0) == -1
        assert _shim(base, 0, None, conv if comp else None, comp, comp) == -1         # a mode that writes pred needs one
        assert (pred == 9).all() and (conv == 7).all()
    assert _shim(h, 0, np.full((40, 40), 9, np.uint16), None, 1, 0) == -1              # compound without conv_dst
    assert svtgpu.lib().svtgpu_shim_calls() == calls                                   # nothing reached the device


# ---------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------
def _blocks(blocks):
    return [svtgpu.WarpBlock.make(b["x"], b["y"], b["w"], b["h"], b["ref0"], b["mat0"], b["ref1"], b["mat1"], b["dist_wtd"], b["fwd"],
                                  b["bck"]) for b in blocks]


def _prepare(w, h, refs):
    dr = [[_dev(a) for a in r] for r in refs]
    dp = [_dev(np.full((h >> (p > 0), w >> (p > 0)), FILL, refs[0][0].dtype)) for p in range(3)]
    rp = [svtgpu.TfPlanes.make([t[p].data_ptr() for p in range(3)], [r[p].shape[1] for p in range(3)]) for t, r in zip(dr, refs)]
    pp = svtgpu.TfPlanes.make([t.data_ptr() for t in dp], [w, w >> 1, w >> 1])
    return rp, pp, dp, dr


def _predict(st, c, blocks):
    rp, pp, dp, dr = _prepare(c["w"], c["h"], c["refs"])
    st.warp_predict_batch(rp, _blocks(blocks), c["bd"], c["chroma"], pp)
    st.ctx.synchronize()
    return [_host(t, c["refs"][0][0].dtype) for t in dp]


@pytest.mark.parametrize("c", BATCHES, ids=[c["name"] for c in BATCHES])
def test_batch_matches_records(ctx, c):
    """The record's samples inside the listed blocks' planes, the sentinel everywhere else: the chroma of blocks below 16 in
    a dimension included, and all chroma without it."""
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    want = wc.expected_planes(c, c["blocks"], FILL)
    for order in (range(len(c["blocks"])), reversed(range(len(c["blocks"]))), np.random.default_rng(3).permutation(len(c["blocks"]))):
        got = _predict(st, c, [c["blocks"][k] for k in order])
        for p in range(3):
            np.testing.assert_array_equal(got[p], want[p], err_msg="%s plane %d" % (c["name"], p))
    assert (want[0] == FILL).any() and sum(b["w"] < 16 or b["h"] < 16 for b in c["blocks"]) == int(c["kinds"][13])
    st.close()


def test_two_calls_back_to_back_on_one_state(ctx):
    """Two different lists queued with no wait in between, the longer one second: each predictor holds its own blocks."""
    c = BATCHES[1]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    lists = [c["blocks"][:4], c["blocks"][4:]]
    rp, pa, a, dr = _prepare(c["w"], c["h"], c["refs"])
    _, pb, b, _ = _prepare(c["w"], c["h"], c["refs"])
    st.warp_predict_batch(rp, _blocks(lists[0]), c["bd"], 1, pa)
    st.warp_predict_batch(rp, _blocks(lists[1]), c["bd"], 1, pb)
    ctx.synchronize()
    for blocks, planes in zip(lists, (a, b)):
        want = wc.expected_planes(c, blocks, FILL)
        for p in range(3):
            np.testing.assert_array_equal(_host(planes[p], np.uint16), want[p], err_msg="plane %d" % p)
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_every_sample_from_the_clamp(ctx, bd):
    """A 64 x 64 block on a 64 x 64 picture whose models send every unit outside the picture, two references on opposite
    sides: against the restatement."""
    w = h = 64
    refs = wc.ref_pictures(bd, w, h, 2, 77)
    far = 300 << 16
    blocks = [dict(x=0, y=0, w=64, h=64, ref0=0, ref1=1, dist_wtd=1, fwd=9, bck=7, mat0=[-far + 0x1234, far + 0x4321, 65536 + 700, -300, 250, 65536 - 900],
                   mat1=[far + 0x7777, -far + 0x0101, 65536 - 500, 420, -380, 65536 + 640])]
    c = dict(w=w, h=h, bd=bd, chroma=1, refs=refs)
    st = svtgpu.TfState(ctx, w, h)
    got = _predict(st, c, blocks)
    want = wc.predict_batch(refs, blocks, bd, w, h, 1, fill=FILL)
    for p in range(3):
        np.testing.assert_array_equal(got[p], want[p], err_msg="plane %d" % p)
        assert len(np.unique(want[p])) <= 4  # corner samples only
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_refusals_leave_pred_untouched(ctx, bd):
    c = BATCHES[0] if bd == 8 else BATCHES[1]
    bs = 1 if bd == 8 else 2
    w, h = c["w"], c["h"]
    st = svtgpu.TfState(ctx, w, h)
    rp, pp, dp, dr = _prepare(w, h, c["refs"])
    ra = (svtgpu.TfPlanes * 3)(*rp)
    good = next(b for b in c["blocks"] if b["w"] == 16 and b["h"] == 16 and b["ref1"] != wc.NO_REF and b["dist_wtd"])
    one = next(b for b in c["blocks"] if b["ref1"] == wc.NO_REF)
    L = svtgpu.lib()

    def rc(blocks=None, refs=ra, n_refs=3, pred=pp, nb=None, chroma=1, depth=bd):
        bl = _blocks([good] if blocks is None else blocks)
        ba = (svtgpu.WarpBlock * max(len(bl), 1))(*bl)
        return L.svtgpu_warp_predict_batch(st.h, refs, n_refs, ba, len(bl) if nb is None else nb, depth, chroma, ctypes.byref(pred), None)

    def changed(pl, plane, ptr=0, stride=0):
        q = svtgpu.TfPlanes.make([pl.plane[k] for k in range(3)], [pl.stride[k] for k in range(3)])
        q.plane[plane], q.stride[plane] = pl.plane[plane] + ptr, pl.stride[plane] + stride
        return q

    assert rc(nb=-1) == -1 and rc(n_refs=-1) == -1 and rc(depth=12) == -1 and rc(n_refs=27) == -3
    assert rc([dict(good, x=w - 8)]) == -1 and rc([dict(good, y=h - 8)]) == -1                 # leaves the picture
    assert rc([dict(good, x=-8)]) == -1 and rc([dict(good, x=good["x"] + 4)]) == -1 and rc([dict(good, y=good["y"] + 4)]) == -1
    for bw, bh in ((4, 8), (8, 4), (8, 64), (64, 8), (32, 128), (128, 32), (256, 128)):        # sizes outside the rule
        assert rc([dict(good, x=0, y=0, w=bw, h=bh)]) == -1, (bw, bh)
    assert rc([dict(good, ref0=3)]) == -1 and rc([dict(good, ref1=3)]) == -1 and rc([dict(good, ref1=254)]) == -1
    assert rc([dict(good, ref1=2)], n_refs=2) == -1
    assert rc([dict(good, dist_wtd=2)]) == -1 and rc([dict(good, fwd=9, bck=8)]) == -1
    assert rc([dict(good, mat0=[0, 0, 0, 0, 0, 65536])]) == -1 and rc([dict(good, mat1=[0, 0, -65536, 0, 0, 65536])]) == -1   # invalid
    assert rc([dict(good, mat0=[0, 0, 65536 + 16384, 0, 0, 65536])]) == -1                     # beyond the first shear limit
    assert rc([dict(good, mat1=[0, 0, 65536, 0, 8192, 65536 + 8192])]) == -1                   # beyond the second
    assert rc([dict(good, mat0=[2 ** 31 - 1, 0, 65536, 0, 0, 65536])]) == -1                   # the projection leaves int32
    assert rc([dict(good, mat1=[0, 2 ** 31 - 1, 65536, 0, 0, 65536])]) == -1
    for plane in range(3):
        assert rc(pred=changed(pp, plane, ptr=bs)) == -1, plane
        assert rc(pred=changed(pp, plane, stride=8 // bs // 2 or 1)) == -1, plane
        assert rc(pred=changed(pp, plane, stride=-16)) == -1, plane
        bad = (svtgpu.TfPlanes * 3)(rp[0], changed(rp[1], plane, stride=-8), rp[2])
        assert rc(refs=bad) == -1, plane
        if bs == 2:
            assert rc(refs=(svtgpu.TfPlanes * 3)(changed(rp[0], plane, ptr=1), rp[1], rp[2])) == -1, plane
    assert rc([good, dict(good, ref0=9)]) == -1   # a good block ahead of a bad one: still refused as a whole
    assert rc(nb=0) == 0                          # a no-op
    ctx.synchronize()
    dtype = c["refs"][0][0].dtype
    assert all((_host(t, dtype) == FILL).all() for t in dp)
    # with one reference the second model and the weights are not looked at
    assert rc([dict(one, mat1=[0] * 6, dist_wtd=7, fwd=1, bck=1)]) == 0
    assert rc(refs=(svtgpu.TfPlanes * 3)(changed(rp[0], 1, ptr=1), rp[1], rp[2]), pred=changed(pp, 2, ptr=1), chroma=0) == 0
    ctx.synchronize()
    st.close()
