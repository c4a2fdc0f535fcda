"""AV1 masked compound prediction on the MI355X: the three shims against every block record of the reference's fixture
(tests/golden/masked_compound.bin) and svtgpu_masked_compound_predict_batch against its four batch records, permuted, back
to back, beside svtgpu_compound_predict_batch on one state, without chroma, on a single corner block, and refused.
Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import compound_cases as cc
import masked_compound_cases as mc
import svtgpu
from test_compound_gpu import _blocks as _compound_blocks, _dev, _host, _prepare

pytestmark = pytest.mark.gpu

BLOCKS = mc.block_cases()
BATCHES = mc.batch_cases()
FILL = 5  # test_compound_gpu._prepare's sentinel


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


# ---------------------------------------------------------------------------------------------
# the three shims
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(BLOCKS)))
def test_shims_match_block_records(i):
    c = BLOCKS[i]
    w, h, bd = c["w"], c["h"], c["bd"]
    r0, r1 = cc.rounds(bd)
    # the two CONV_BUF_TYPE blocks inside larger buffers with strides of their own
    s0, s1 = np.full((h + 2, w + 5), 7, np.uint16), np.full((h + 1, w + 11), 9, np.uint16)
    s0[:h, :w], s1[:h, :w] = c["c0"], c["c1"]
    for t in (0, 1):
        np.testing.assert_array_equal(svtgpu.diffwtd_mask(t, s0, s1, w, h, r0, r1, bd), c["masks"][t], err_msg="%s mask %d" % (c["name"], t))
    mask = np.full((h + 3, w + 9), 77, np.uint8)
    mask[:h, :w] = c["masks"][c["index"] & 1]
    for f, want in c["outs"].items():
        subw, subh = f & 1, f >> 1
        ow, oh = w >> subw, h >> subh
        dst = np.full((oh + 4, ow + 7), 3, np.uint16 if bd > 8 else np.uint8)
        svtgpu.blend_a64_d16_mask(dst, 3, 2, s0, s1, mask, ow, oh, subw, subh, r0, r1, bd)
        np.testing.assert_array_equal(dst[2:2 + oh, 3:3 + ow], want, err_msg="%s form %d" % (c["name"], f))
        dst[2:2 + oh, 3:3 + ow] = 3
        assert (dst == 3).all(), c["name"]
    assert (s0[:h, :w] == c["c0"]).all() and (s0[:, w:] == 7).all() and (mask[:, w:] == 77).all()


def test_highbd_blend_takes_eight_bit_blocks_too():
    """The highbd entry at bd 8 gives what the lowbd entry gives."""
    c = next(c for c in BLOCKS if c["bd"] == 8 and c["content"] == 0 and c["w"] >= 8)
    r0, r1 = cc.rounds(8)
    dst = np.zeros((c["h"], c["w"]), np.uint16)
    svtgpu.blend_a64_d16_mask(dst, 0, 0, c["c0"], c["c1"], np.ascontiguousarray(c["masks"][c["index"] & 1]), c["w"], c["h"], 0, 0, r0, r1, 8)
    np.testing.assert_array_equal(dst, c["outs"][0])


# ---------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------
def _blocks(blocks):
    return [svtgpu.MaskedCompoundBlock.make(b["x"], b["y"], b["w"], b["h"], b["ref0"], b["ref1"], b["mv0"], b["mv1"], b["fx"], b["fy"],
                                            b["type"], b["widx"], b["wsign"], b["mtype"]) for b in blocks]


def _predict(st, c, blocks, chroma=None, prepared=None):
    """One call on record c's references with `blocks`; the three predictor planes (FILL where nothing is written)."""
    rp, pp, dp, dr = prepared or _prepare(c["w"], c["h"], c["refs"], c["pad"])
    st.masked_compound_predict_batch(rp, c["border"], c["border"], _blocks(blocks), c["bd"], c["chroma"] if chroma is None else chroma, pp)
    st.ctx.synchronize()
    return [_host(t, c["refs"][0][0].dtype) for t in dp]


@pytest.mark.parametrize("c", BATCHES, ids=[c["name"] for c in BATCHES])
def test_batch_matches_records(ctx, c):
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _predict(st, c, c["blocks"])
    for p, want in enumerate(c["pred"]):
        np.testing.assert_array_equal(got[p], want, err_msg="%s plane %d" % (c["name"], p))
    if not c["chroma"]:
        assert (got[1] == FILL).all() and (got[2] == FILL).all(), c["name"]  # untouched
    st.close()


def test_output_unchanged_when_the_list_is_permuted(ctx):
    c = BATCHES[1]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    order = np.random.default_rng(3).permutation(len(c["blocks"]))
    got = _predict(st, c, [c["blocks"][k] for k in order])
    for p in range(3):
        np.testing.assert_array_equal(got[p], c["pred"][p], err_msg="plane %d" % p)
    st.close()


def test_two_calls_back_to_back_keep_their_own_masks(ctx):
    """The DIFFWTD blocks, then the wedge blocks of the same picture, queued on one state and stream with no wait in between,
    into two predictors: each holds its own blocks' samples of the record and the sentinel elsewhere, so the second call saw
    nothing of the first's mask plane."""
    c = BATCHES[0]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    lists = [[b for b in c["blocks"] if b["type"] == t] for t in (mc.DIFFWTD, mc.WEDGE)]
    rp, pa, a, dr = _prepare(c["w"], c["h"], c["refs"], c["pad"])
    _, pb, b, _ = _prepare(c["w"], c["h"], c["refs"], c["pad"])
    st.masked_compound_predict_batch(rp, c["border"], c["border"], _blocks(lists[0]), c["bd"], 1, pa)
    st.masked_compound_predict_batch(rp, c["border"], c["border"], _blocks(lists[1]), c["bd"], 1, pb)
    ctx.synchronize()
    dtype = c["refs"][0][0].dtype
    for blocks, planes in zip(lists, (a, b)):
        for p in range(3):
            want = np.full(c["pred"][p].shape, FILL, dtype)
            for k in blocks:
                ss = int(p > 0)
                x, y = (((k["x"] >> 3) << 3) >> 1, ((k["y"] >> 3) << 3) >> 1) if ss else (k["x"], k["y"])
                want[y:y + (k["h"] >> ss), x:x + (k["w"] >> ss)] = c["pred"][p][y:y + (k["h"] >> ss), x:x + (k["w"] >> ss)]
            np.testing.assert_array_equal(_host(planes[p], dtype), want, err_msg="plane %d" % p)
    st.close()


def test_beside_the_average_compound_on_one_state(ctx):
    """svtgpu_compound_predict_batch, then the masked entry, then svtgpu_compound_predict_batch again on one state: the
    state's metadata buffer and mask plane serve all three, and the average entry still gives tests/golden/compound.bin."""
    c, avg = BATCHES[1], cc.batch_cases()[1]
    assert (c["w"], c["h"], c["bd"]) == (avg["w"], avg["h"], avg["bd"])
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    outs = []
    for which in (avg, c, avg):
        rp, pp, dp, dr = _prepare(which["w"], which["h"], which["refs"], which["pad"])
        if which is avg:
            st.compound_predict_batch(rp, avg["pad"], avg["pad"], _compound_blocks(avg["blocks"]), avg["bd"], 1, pp)
        else:
            st.masked_compound_predict_batch(rp, c["border"], c["border"], _blocks(c["blocks"]), c["bd"], 1, pp)
        outs.append((dp, dr))
    ctx.synchronize()
    for which, (dp, _) in zip((avg, c, avg), outs):
        for p in range(3):
            np.testing.assert_array_equal(_host(dp[p], which["refs"][0][0].dtype), which["pred"][p], err_msg="%s plane %d" % (which["name"], p))
    st.close()


def test_luma_only_with_null_chroma_planes(ctx):
    c = BATCHES[0]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    rp, pp, dp, dr = _prepare(c["w"], c["h"], c["refs"], c["pad"])
    luma_refs = [svtgpu.TfPlanes.make([r.plane[0], 0, 0], [r.stride[0], 0, 0]) for r in rp]
    luma_pred = svtgpu.TfPlanes.make([pp.plane[0], 0, 0], [pp.stride[0], 0, 0])
    st.masked_compound_predict_batch(luma_refs, c["border"], c["border"], _blocks(c["blocks"]), c["bd"], 0, luma_pred)
    ctx.synchronize()
    dtype = c["refs"][0][0].dtype
    np.testing.assert_array_equal(_host(dp[0], dtype), c["pred"][0])
    assert (_host(dp[1], dtype) == FILL).all() and (_host(dp[2], dtype) == FILL).all()
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_samples_outside_the_listed_blocks_are_unchanged(ctx, bd):
    c = BATCHES[0] if bd == 8 else BATCHES[1]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    some = c["blocks"][2::3]
    got = _predict(st, c, some)
    want = mc.predict_batch(c["refs"], c["pad"], some, bd, c["w"], c["h"], 1, border=(c["border"], c["border"]), fill=FILL)
    for p in range(3):
        np.testing.assert_array_equal(got[p], want[p], err_msg="plane %d" % p)
        assert (want[p] == FILL).any()
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_single_diffwtd_block_at_the_bottom_right_corner(ctx, bd):
    """One 8x8 DIFFWTD block whose last sample is the picture's: the highest index of the mask plane, and a second launch of
    one wave with one slot."""
    c = BATCHES[0] if bd == 8 else BATCHES[1]
    w, h = c["w"], c["h"]
    st = svtgpu.TfState(ctx, w, h)
    for mtype in (0, 1):
        one = [dict(x=w - 8, y=h - 8, w=8, h=8, ref0=0, ref1=2, mv0=(-21, 9), mv1=(30, -13), fx=0, fy=2, type=mc.DIFFWTD, widx=0,
                    wsign=0, mtype=mtype)]
        got = _predict(st, c, one)
        want = mc.predict_batch(c["refs"], c["pad"], one, bd, w, h, 1, border=(c["border"], c["border"]), fill=FILL)
        for p in range(3):
            np.testing.assert_array_equal(got[p], want[p], err_msg="mask type %d plane %d" % (mtype, p))
        assert (want[0][h - 8:, w - 8:] != FILL).any() and (want[0][:h - 8] == FILL).all()
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_refusals_leave_pred_untouched(ctx, bd):
    """Every refusal the entry lists: its code, before any launch, on a real state; then n_blocks = 0, a no-op."""
    c = BATCHES[0] if bd == 8 else BATCHES[1]
    bs = 1 if bd == 8 else 2
    w, h = c["w"], c["h"]
    st = svtgpu.TfState(ctx, w, h)
    rp, pp, dp, dr = _prepare(w, h, c["refs"], c["pad"])
    ra = (svtgpu.TfPlanes * 3)(*rp)
    good = c["blocks"][10]   # a 16x16 wedge block
    diff = c["blocks"][11]   # a 16x16 DIFFWTD block
    assert good["type"] == mc.WEDGE and diff["type"] == mc.DIFFWTD
    L = svtgpu.lib()

    def rc(blocks=None, refs=ra, n_refs=3, pred=pp, nb=None, chroma=1, bx=c["pad"], by=c["pad"], patch=None):
        bl = _blocks([good] if blocks is None else blocks)
        ba = (svtgpu.MaskedCompoundBlock * max(len(bl), 1))(*bl)
        if patch:
            patch(ba)
        return L.svtgpu_masked_compound_predict_batch(st.h, refs, n_refs, bx, by, ba, len(bl) if nb is None else nb, bd, chroma,
                                                      ctypes.byref(pred), None)

    def changed(pl, plane, ptr=0, stride=0):
        q = svtgpu.TfPlanes.make([pl.plane[k] for k in range(3)], [pl.stride[k] for k in range(3)])
        q.plane[plane], q.stride[plane] = pl.plane[plane] + ptr, pl.stride[plane] + stride
        return q

    def reserved(k):
        def patch(ba):
            ba[0].reserved[k] = 1
        return patch
    # the added refusals
    assert rc([dict(good, type=2)]) == -1 and rc([dict(diff, type=255)]) == -1
    for bw, bh in ((64, 64), (64, 32), (16, 64), (64, 16), (128, 128)):               # sizes a compound may have, without wedges
        assert rc([dict(good, x=0, y=0, w=bw, h=bh)]) == -1, (bw, bh)
        assert rc([dict(diff, x=0, y=0, w=bw, h=bh)]) == 0, (bw, bh)
    ctx.synchronize()
    for t in dp:                                                                      # the accepted calls wrote: start again
        t.fill_(FILL)
    torch.cuda.synchronize()
    assert rc([dict(good, widx=16)]) == -1 and rc([dict(diff, widx=16)]) == -1
    assert rc([dict(good, wsign=2)]) == -1 and rc([dict(diff, wsign=2)]) == -1
    assert rc([dict(good, mtype=2)]) == -1 and rc([dict(diff, mtype=2)]) == -1
    for k in range(10):
        assert rc(patch=reserved(k)) == -1, k
    # svtgpu_compound_predict_batch's refusals
    assert rc(nb=-1) == -1
    assert rc([dict(good, x=w - good["w"] + 8)]) == -1 and rc([dict(good, y=h - good["h"] + 8)]) == -1   # leaves the picture
    assert rc([dict(good, x=-8)]) == -1 and rc([dict(good, x=good["x"] + 2)]) == -1                      # negative, not at 4
    for bw, bh in ((4, 8), (8, 4), (8, 64), (64, 8), (32, 128), (128, 32), (256, 128)):                   # sizes outside the rule
        assert rc([dict(diff, x=0, y=0, w=bw, h=bh)]) == -1, (bw, bh)
    assert rc([dict(good, ref0=3)]) == -1 and rc([dict(good, ref1=3)]) == -1 and rc([dict(good, ref1=2)], n_refs=2) == -1
    assert rc([dict(good, fx=4)]) == -1 and rc([dict(good, fy=4)]) == -1
    assert rc(bx=-1) == -1 and rc(by=-1) == -1
    assert rc(bx=c["pad"] + 1) == -1  # the stride cannot hold width + 2 * border
    assert rc(n_refs=27) == -3
    for plane in range(3):
        assert rc(pred=changed(pp, plane, ptr=bs)) == -1, plane                    # pred not 16-byte aligned
        assert rc(pred=changed(pp, plane, stride=8 // bs // 2 or 1)) == -1, plane   # pred stride no multiple of 16 bytes
        assert rc(pred=changed(pp, plane, stride=-16)) == -1, plane                # pred narrower than the picture
        bad = (svtgpu.TfPlanes * 3)(rp[0], changed(rp[1], plane, stride=-(c["refs"][1][plane].shape[1] - (w >> (plane > 0)))), rp[2])
        assert rc(refs=bad) == -1, plane
        if bs == 2:
            bad = (svtgpu.TfPlanes * 3)(changed(rp[0], plane, ptr=1), rp[1], rp[2])
            assert rc(refs=bad) == -1, plane                                       # a 16-bit plane at an odd address
    assert rc([good, dict(good, fx=9)]) == -1  # a good block behind a bad one: still refused as a whole
    assert rc(nb=0) == 0  # a no-op
    ctx.synchronize()
    dtype = c["refs"][0][0].dtype
    assert all((_host(t, dtype) == FILL).all() for t in dp)
    # without chroma planes 1 and 2 are not looked at, and the unchanged arguments are accepted
    assert rc(refs=(svtgpu.TfPlanes * 3)(changed(rp[0], 1, ptr=1), rp[1], rp[2]), pred=changed(pp, 2, ptr=1), chroma=0) == 0
    assert rc() == 0
    ctx.synchronize()
    st.close()


def test_the_average_entry_still_ignores_its_reserved_bytes(ctx):
    c = cc.batch_cases()[0]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    rp, pp, dp, dr = _prepare(c["w"], c["h"], c["refs"], c["pad"])
    bl = _compound_blocks(c["blocks"])
    for b in bl:
        for k in range(11):
            b.reserved[k] = 0xFF
    st.compound_predict_batch(rp, c["pad"], c["pad"], bl, c["bd"], 1, pp)
    ctx.synchronize()
    for p in range(3):
        np.testing.assert_array_equal(_host(dp[p], c["refs"][0][0].dtype), c["pred"][p])
    st.close()
