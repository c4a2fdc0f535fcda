"""AV1 sub-pel interpolation and the temporal filter's motion compensation on the MI355X: the eight interpolation shims
against every block record of the reference's fixture (tests/golden/interp.bin), svtgpu_tf_predict_frame against every
prediction record, with the encoder's 68-sample border and on a frame the fixture does not hold against the numpy
restatement that tests/test_interp.py holds to those records, and the chain predict -> svtgpu_tf_filter_frame against the
chain records.  Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import interp_cases as ic
import svtgpu

pytestmark = pytest.mark.gpu

BLOCKS = ic.block_cases()
PREDS = ic.pred_cases()
CHAINS = ic.chain_cases()


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def _dev(a):
    """A device copy of a uint8 / uint16 array (torch has no uint16 arithmetic: the bits travel as int16)."""
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
    w, h = c["w"], c["h"]
    src = ic.block_source(c["bd"], w, h, c["content"], c["index"])
    # the (h + 8) x (w + 8) source inside a larger buffer whose stride is no multiple of 16; guard values around dst
    big = np.full((h + 14, w + 21), 1, src.dtype)
    big[2:2 + h + 8, 5:5 + w + 8] = src
    dst = np.full((h + 4, w + 7), 9, src.dtype)
    fx, fy = ic.block_filters(c)
    r0, r1 = ic.rounds(c["bd"])
    svtgpu.convolve_sr(ic.FORMS[c["form"]], big, 5 + 3, 2 + 3, w, h, fx, fy, r0, r1, c["bd"], dst, 3, 2)
    np.testing.assert_array_equal(dst[2:2 + h, 3:3 + w], c["out"], err_msg=c["name"])
    guard = dst.copy()
    guard[2:2 + h, 3:3 + w] = 9
    assert (guard == 9).all(), c["name"]


# ---------------------------------------------------------------------------------------------
# whole pictures
# ---------------------------------------------------------------------------------------------
def _motion(rows):
    return [svtgpu.TfMotion.make(m["use64"], m["mv64"], m["split32"], m["split16"], m["mv32"], m["mv16"], m["mv8"])
            for row in rows for m in row]


def _prepare(state, refs, pad):
    """Device copies of padded reference pictures (lists of three planes, `pad` luma samples around the picture) and
    predictor planes over the 64-aligned area prefilled with 5: (TfPlanes of the references at sample (0, 0), TfPlanes of
    the predictors, the predictor tensors, the reference tensors)."""
    aw, ah = (state.width + 63) & ~63, (state.height + 63) & ~63
    dr = [[_dev(a) for a in r] for r in refs]
    dp = [[_dev(np.full((ah >> (p > 0), aw >> (p > 0)), 5, refs[0][0].dtype)) for p in range(3)] for _ in refs]
    rp = [svtgpu.TfPlanes.make([t[p].data_ptr() + ((pad >> (p > 0)) * (r[p].shape[1] + 1)) * r[p].itemsize for p in range(3)],
                               [r[p].shape[1] for p in range(3)]) for t, r in zip(dr, refs)]
    pp = [svtgpu.TfPlanes.make([t.data_ptr() for t in d], [aw, aw >> 1, aw >> 1]) for d in dp]
    return rp, pp, dp, dr


def _predict(state, refs, pad, motion, bd, tf_chroma, border):
    """svtgpu_tf_predict_frame; returns per reference the three predictor planes over the 64-aligned area."""
    rp, pp, dp, dr = _prepare(state, refs, pad)
    state.predict_frame(rp, border[0], border[1], _motion(motion), bd, tf_chroma, pp)
    state.ctx.synchronize()
    return [[_host(t, refs[0][0].dtype) for t in d] for d in dp]


@pytest.mark.parametrize("c", PREDS, ids=[c["name"] for c in PREDS])
def test_predict_frame_matches_records(ctx, c):
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _predict(st, c["refs"], c["pad"], c["motion"], c["bd"], c["tf_chroma"], (c["pad"], c["pad"]))
    for r in range(c["n_refs"]):
        for p, want in enumerate(c["pred"][r]):
            np.testing.assert_array_equal(got[r][p], want, err_msg="%s reference %d plane %d" % (c["name"], r, p))
        if not c["tf_chroma"]:
            assert (got[r][1] == 5).all() and (got[r][2] == 5).all(), c["name"]  # untouched
    st.close()


@pytest.mark.parametrize("c", [PREDS[0], PREDS[2]], ids=["8-bit", "10-bit"])
def test_predict_frame_with_the_encoders_border(ctx, c):
    """border 68 / 34 on planes of noise that are allocated to 80: the device must give what the restatement gives from
    planes whose samples beyond 68 / 34 are overwritten.  Without the clamp the result differs (asserted on the
    restatement, in luma and in chroma), so a kernel that does not clamp, or clamps elsewhere, fails here; it would still
    read allocated memory only."""
    refs, motion, want, free = ic.border_case(c, 68)
    assert any(m["use64"] and abs(int(m["mv64"][0])) > 8 * c["w"] for row in motion for m in row)
    for p in range(3):
        assert any((want[r][p] != free[r][p]).any() for r in range(c["n_refs"])), "the clamp changes nothing in plane %d" % p
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _predict(st, refs, c["pad"], motion, c["bd"], 1, (68, 68))
    for r in range(c["n_refs"]):
        for p in range(3):
            np.testing.assert_array_equal(got[r][p], want[r][p], err_msg="%s reference %d plane %d" % (c["name"], r, p))
    # the same planes with 80 declared readable: the reference's own reads, no clamp
    got = _predict(st, refs, c["pad"], motion, c["bd"], 1, (80, 80))
    for r in range(c["n_refs"]):
        for p in range(3):
            np.testing.assert_array_equal(got[r][p], free[r][p], err_msg="%s reference %d plane %d" % (c["name"], r, p))
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_predict_frame_refuses_misaligned_and_narrow_planes(ctx, bd):
    """SVTGPU_ERR_INVALID_ARG before any launch, on a real state: nothing is written."""
    c = PREDS[0] if bd == 8 else PREDS[2]
    bs = 1 if bd == 8 else 2
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    rp, pp, dp, dr = _prepare(st, c["refs"][:1], c["pad"])
    mo = (svtgpu.TfMotion * c["nblk"])(*_motion(c["motion"][:1]))
    L = svtgpu.lib()

    def rc(ref, pred, chroma=1, border=68):
        return L.svtgpu_tf_predict_frame(st.h, ctypes.byref(ref), 1, border, border, mo, bd, chroma, ctypes.byref(pred), None)

    def changed(pl, plane, ptr=0, stride=0):
        q = svtgpu.TfPlanes.make([pl.plane[k] for k in range(3)], [pl.stride[k] for k in range(3)])
        q.plane[plane], q.stride[plane] = pl.plane[plane] + ptr, pl.stride[plane] + stride
        return q
    for plane in range(3):
        assert rc(rp[0], changed(pp[0], plane, ptr=bs)) == -1, plane                   # pred not 16-byte aligned
        assert rc(rp[0], changed(pp[0], plane, stride=8 // bs // 2 or 1)) == -1, plane  # pred stride no multiple of 16 bytes
        assert rc(rp[0], changed(pp[0], plane, stride=-64)) == -1, plane               # pred narrower than the aligned width
        assert rc(changed(rp[0], plane, stride=-(c["refs"][0][plane].shape[1] - (c["w"] >> (plane > 0)))), pp[0]) == -1, plane
        if bs == 2:
            assert rc(changed(rp[0], plane, ptr=1), pp[0]) == -1, plane                # a 16-bit plane at an odd address
    assert rc(rp[0], pp[0], border=81) == -1  # the stride cannot hold width + 2 * border
    # without tf_chroma the chroma planes are not looked at
    assert rc(changed(changed(rp[0], 1, ptr=1), 2, stride=-10000), changed(pp[0], 1, ptr=1), chroma=0) == 0
    ctx.synchronize()
    want = ic.predict_frame(c["refs"][0], c["pad"], c["motion"][0], bd, c["w"], c["h"], 0, border=(68, 68))
    np.testing.assert_array_equal(_host(dp[0][0], c["refs"][0][0].dtype), want[0])
    assert all((_host(dp[0][p], c["refs"][0][0].dtype) == 5).all() for p in (1, 2))
    assert rc(rp[0], pp[0]) == 0  # and the unchanged arguments are accepted
    ctx.synchronize()
    st.close()


def test_predict_frame_cross_check_against_the_restatement(ctx):
    """200x136 10-bit (4x3 blocks, partial right and bottom blocks), two references, random partitions and MVs."""
    w, h, bd, pad = 200, 136, 10, 80
    rng = np.random.default_rng(11)
    refs = [ic.padded_reference(bd, w, h, 0x4950000000500000 + 4 * r, pad) for r in range(2)]
    motion = [ic.random_motion(rng, 12, w) for _ in range(2)]
    st = svtgpu.TfState(ctx, w, h)
    got = _predict(st, refs, pad, motion, bd, 1, (72, 72))
    for r in range(2):
        want = ic.predict_frame(refs[r], pad, motion[r], bd, w, h, 1)
        for p in range(3):
            np.testing.assert_array_equal(got[r][p], want[p], err_msg="reference %d plane %d" % (r, p))
    st.close()


@pytest.mark.parametrize("c", CHAINS, ids=[c["name"] for c in CHAINS])
def test_predict_then_filter_matches_the_chain_record(ctx, c):
    pc = c["pred"]
    st = svtgpu.TfState(ctx, pc["w"], pc["h"])
    rp, pp, dp, dr = _prepare(st, pc["refs"], pc["pad"])
    aw = (pc["w"] + 63) & ~63
    strides = [aw, aw >> 1, aw >> 1]
    dc = [_dev(a) for a in c["centre"]]
    do = [_dev(np.full(a.shape, 5, a.dtype)) for a in c["centre"]]
    blocks = []
    for r in range(pc["n_refs"]):
        for b, m in enumerate(pc["motion"][r]):
            blocks.append(svtgpu.TfBlock.make(m["split32"], m["mv32"], m["mv16"], c["err32"][r][b], c["err16"][r][b]))
    prm = svtgpu.TfParams.make(c["decay"], c["mv_dist_th"], c["tf_chroma"], pc["bd"], 0)

    def planes(ts):
        return svtgpu.TfPlanes.make([t.data_ptr() for t in ts], strides)
    st.predict_frame(rp, pc["pad"], pc["pad"], _motion(pc["motion"]), pc["bd"], 1, pp)
    st.filter_frame(planes(dc), pp, blocks, prm, planes(do))  # same stream: no wait in between
    ctx.synchronize()
    for p in range(3):
        hh, ww = c["out"][p].shape
        np.testing.assert_array_equal(_host(do[p], c["centre"][p].dtype)[:hh, :ww], c["out"][p], err_msg="%s plane %d" % (c["name"], p))
    st.close()


def test_two_predict_calls_back_to_back_keep_their_own_motion(ctx):
    """Two calls queued on one state with different motion and no wait in between: the metadata buffer's reuse."""
    c = PREDS[0]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    swapped = [c["motion"][1], c["motion"][0]]
    rp, pa, a, dr = _prepare(st, c["refs"], c["pad"])
    _, pb, b, _ = _prepare(st, c["refs"], c["pad"])
    st.predict_frame(rp, c["pad"], c["pad"], _motion(c["motion"]), c["bd"], 1, pa)
    st.predict_frame(rp, c["pad"], c["pad"], _motion(swapped), c["bd"], 1, pb)
    ctx.synchronize()
    dtype = c["refs"][0][0].dtype
    for r in range(2):
        want_b = ic.predict_frame(c["refs"][r], c["pad"], swapped[r], c["bd"], c["w"], c["h"], 1)
        for p in range(3):
            np.testing.assert_array_equal(_host(a[r][p], dtype), c["pred"][r][p], err_msg="first call, reference %d plane %d" % (r, p))
            np.testing.assert_array_equal(_host(b[r][p], dtype), want_b[p], err_msg="second call, reference %d plane %d" % (r, p))
    st.close()
