"""AV1 compound prediction on the MI355X: the eight jnt_convolve shims against every block record of the reference's
fixture (tests/golden/compound.bin), svtgpu_compound_predict_batch against the three batch records and, on a picture the
fixture does not hold and with the read clamp acting, against the numpy restatement that tests/test_compound.py holds to
those records.  Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import compound_cases as cc
import svtgpu

pytestmark = pytest.mark.gpu

BLOCKS = cc.block_cases()
BATCHES = cc.batch_cases()
FILL = 5


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype == np.uint16 else np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


# ---------------------------------------------------------------------------------------------
# the eight shims
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(BLOCKS)))
def test_shims_match_block_records(i):
    c = BLOCKS[i]
    w, h, bd = c["w"], c["h"], c["bd"]
    fx, fy = cc.block_filters(c)
    r0, r1 = cc.rounds(bd)
    form = cc.FORMS[c["form"]]
    srcs = []
    for k in (0, 1):  # the (h + 8) x (w + 8) source inside a larger buffer whose stride is no multiple of 16
        src = cc.block_source(bd, w, h, c["content"], c["index"], k)
        big = np.full((h + 14, w + 21), 1, src.dtype)
        big[2:2 + h + 8, 5:5 + w + 8] = src
        srcs.append(big)
    conv = np.full((h, w + 3), 7, np.uint16)  # conv_dst with a stride of its own
    dst = np.full((h + 4, w + 7), 9, srcs[0].dtype)
    # first call: only conv_dst is written
    svtgpu.jnt_convolve(form, srcs[0], 5 + 3, 2 + 3, w, h, fx, fy, r0, r1, bd, conv, 0, dst=dst, dx0=3, dy0=2)
    np.testing.assert_array_equal(conv[:, :w], c["conv"], err_msg=c["name"] + " conv_dst")
    assert (conv[:, w:] == 7).all() and (dst == 9).all(), c["name"]
    # second call: conv_dst read, pixels written
    svtgpu.jnt_convolve(form, srcs[1], 5 + 3, 2 + 3, w, h, fx, fy, r0, r1, bd, conv, 1, c["mode"][0], c["mode"][1], c["mode"][2],
                        dst=dst, dx0=3, dy0=2)
    np.testing.assert_array_equal(dst[2:2 + h, 3:3 + w], c["out"], err_msg=c["name"])
    np.testing.assert_array_equal(conv[:, :w], c["conv"], err_msg=c["name"] + " conv_dst after the second call")
    guard = dst.copy()
    guard[2:2 + h, 3:3 + w] = 9
    assert (guard == 9).all(), c["name"]


def test_shim_shapes_the_issue_names_are_in_the_records():
    assert {(4, 4), (4, 16), (128, 128)} <= {(c["w"], c["h"]) for c in BLOCKS}
    assert {c["content"] for c in BLOCKS} == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------
def _blocks(blocks):
    return [svtgpu.CompoundBlock.make(b["x"], b["y"], b["w"], b["h"], b["ref0"], b["ref1"], b["mv0"], b["mv1"], b["fx"], b["fy"],
                                      *b["mode"]) for b in blocks]


def _prepare(w, h, refs, pad):
    """Device copies of padded reference pictures and predictor planes prefilled with FILL: (TfPlanes of the references at
    sample (0, 0), TfPlanes of the predictor, the predictor tensors, the reference tensors)."""
    dr = [[_dev(a) for a in r] for r in refs]
    dp = [_dev(np.full((h >> (p > 0), w >> (p > 0)), FILL, refs[0][0].dtype)) for p in range(3)]
    rp = [svtgpu.TfPlanes.make([t[p].data_ptr() + ((pad >> (p > 0)) * (r[p].shape[1] + 1)) * r[p].itemsize for p in range(3)],
                               [r[p].shape[1] for p in range(3)]) for t, r in zip(dr, refs)]
    pp = svtgpu.TfPlanes.make([t.data_ptr() for t in dp], [w, w >> 1, w >> 1])
    return rp, pp, dp, dr


def _predict(st, refs, pad, blocks, bd, chroma, border):
    rp, pp, dp, dr = _prepare(st.width, st.height, refs, pad)
    st.compound_predict_batch(rp, border[0], border[1], _blocks(blocks), bd, chroma, pp)
    st.ctx.synchronize()
    return [_host(t, refs[0][0].dtype) for t in dp]


@pytest.mark.parametrize("c", BATCHES, ids=[c["name"] for c in BATCHES])
def test_batch_matches_records(ctx, c):
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _predict(st, c["refs"], c["pad"], c["blocks"], c["bd"], c["chroma"], (c["pad"], c["pad"]))
    for p, want in enumerate(c["pred"]):
        np.testing.assert_array_equal(got[p], want, err_msg="%s plane %d" % (c["name"], p))
    if not c["chroma"]:
        assert (got[1] == FILL).all() and (got[2] == FILL).all(), c["name"]  # untouched
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_batch_with_a_declared_border_smaller_than_the_allocation(ctx, bd):
    """128 x 64, planes of noise allocated with 80 samples around the picture, 40 declared readable: every MV puts its block
    one eighth inside the MV clamp's bound or far outside it, so blocks reach up to 64 + 7 samples out and the read clamp
    acts.  The device must give what the restatement gives from planes whose samples beyond the declared border are
    overwritten; without the clamp the result differs (asserted on the restatement)."""
    w, h, pad, border = 128, 64, 80, 40
    rng = np.random.default_rng(1000 + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    refs = [[rng.integers(0, 1 << bd, ((h + 2 * pad) >> (p > 0), (w + 2 * pad) >> (p > 0))).astype(dt)
             for p in range(3)] for _ in range(2)]
    blocks = cc.pyramid_blocks(rng)
    assert [(b["w"], b["h"]) for b in blocks][:2] == [(64, 64), (32, 64)] and (blocks[-1]["w"], blocks[-1]["h"]) == (8, 8)
    cut = []
    for r in refs:
        planes = []
        for p, a in enumerate(r):
            k = (pad - border) >> (p > 0)
            b = np.full(a.shape, 1, a.dtype)
            b[k:a.shape[0] - k, k:a.shape[1] - k] = a[k:a.shape[0] - k, k:a.shape[1] - k]
            planes.append(b)
        cut.append(planes)
    want = cc.predict_batch(cut, pad, blocks, bd, w, h, 1, border=(border, border), fill=FILL)
    free = cc.predict_batch(refs, pad, blocks, bd, w, h, 1, border=(pad, pad), fill=FILL)
    for p in range(3):
        assert (want[p] != free[p]).any(), "the clamp changes nothing in plane %d" % p
    st = svtgpu.TfState(ctx, w, h)
    got = _predict(st, refs, pad, blocks, bd, 1, (border, border))
    for p in range(3):
        np.testing.assert_array_equal(got[p], want[p], err_msg="plane %d" % p)
    st.close()


def test_two_calls_back_to_back_keep_their_own_lists(ctx):
    """Two calls queued on one state and stream with different block lists and no wait in between."""
    c = BATCHES[0]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    other = [dict(b, mv0=b["mv1"], mv1=b["mv0"], fx=b["fy"], fy=b["fx"]) for b in c["blocks"][::-1]]
    rp, pa, a, dr = _prepare(c["w"], c["h"], c["refs"], c["pad"])
    _, pb, b, _ = _prepare(c["w"], c["h"], c["refs"], c["pad"])
    st.compound_predict_batch(rp, c["pad"], c["pad"], _blocks(c["blocks"]), c["bd"], 1, pa)
    st.compound_predict_batch(rp, c["pad"], c["pad"], _blocks(other), c["bd"], 1, pb)
    ctx.synchronize()
    want_b = cc.predict_batch(c["refs"], c["pad"], other, c["bd"], c["w"], c["h"], 1, border=(c["pad"], c["pad"]))
    dtype = c["refs"][0][0].dtype
    for p in range(3):
        np.testing.assert_array_equal(_host(a[p], dtype), c["pred"][p], err_msg="first call, plane %d" % p)
        np.testing.assert_array_equal(_host(b[p], dtype), want_b[p], err_msg="second call, plane %d" % p)
    st.close()


def test_output_unchanged_when_the_list_is_permuted(ctx):
    c = BATCHES[1]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    order = np.random.default_rng(3).permutation(len(c["blocks"]))
    got = _predict(st, c["refs"], c["pad"], [c["blocks"][k] for k in order], c["bd"], 1, (c["pad"], c["pad"]))
    for p in range(3):
        np.testing.assert_array_equal(got[p], c["pred"][p], err_msg="plane %d" % p)
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
    good = c["blocks"][5]
    L = svtgpu.lib()

    def rc(blocks=None, refs=ra, n_refs=3, pred=pp, nb=None, chroma=1, bx=c["pad"], by=c["pad"]):
        bl = _blocks([good] if blocks is None else blocks)
        ba = (svtgpu.CompoundBlock * max(len(bl), 1))(*bl)
        return L.svtgpu_compound_predict_batch(st.h, refs, n_refs, bx, by, ba, len(bl) if nb is None else nb, bd, chroma,
                                               ctypes.byref(pred), None)

    def changed(pl, plane, ptr=0, stride=0):
        q = svtgpu.TfPlanes.make([pl.plane[k] for k in range(3)], [pl.stride[k] for k in range(3)])
        q.plane[plane], q.stride[plane] = pl.plane[plane] + ptr, pl.stride[plane] + stride
        return q
    assert rc(nb=-1) == -1
    assert rc([dict(good, x=w - good["w"] + 8)]) == -1 and rc([dict(good, y=h - good["h"] + 8)]) == -1   # leaves the picture
    assert rc([dict(good, x=-8)]) == -1 and rc([dict(good, x=good["x"] + 2)]) == -1                      # negative, not at 4
    for bw, bh in ((4, 8), (8, 4), (8, 64), (64, 8), (32, 128), (128, 32), (256, 128)):                   # sizes outside the rule
        assert rc([dict(good, x=0, y=0, w=bw, h=bh)]) == -1, (bw, bh)
    assert rc([dict(good, ref0=3)]) == -1 and rc([dict(good, ref1=3)]) == -1 and rc([dict(good, ref1=2)], n_refs=2) == -1
    assert rc([dict(good, fx=4)]) == -1 and rc([dict(good, fy=4)]) == -1
    assert rc([dict(good, mode=(1, 9, 8))]) == -1 and rc([dict(good, mode=(1, 0, 0))]) == -1 and rc([dict(good, mode=(2, 9, 7))]) == -1
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
    # a good block behind a bad one: still refused as a whole
    assert rc([good, dict(good, fx=9)]) == -1
    assert rc(nb=0) == 0  # a no-op
    ctx.synchronize()
    dtype = c["refs"][0][0].dtype
    assert all((_host(t, dtype) == FILL).all() for t in dp)
    # without chroma planes 1 and 2 are not looked at, and the unchanged arguments are accepted
    assert rc(refs=(svtgpu.TfPlanes * 3)(changed(rp[0], 1, ptr=1), rp[1], rp[2]), pred=changed(pp, 2, ptr=1), chroma=0) == 0
    assert rc() == 0
    ctx.synchronize()
    st.close()
