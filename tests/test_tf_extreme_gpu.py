"""The temporal filter on the MI355X on worst-case and all-tie content: svtgpu_tf_search_frame + svtgpu_tf_search_read,
svtgpu_tf_compensate_filter_frame (and its two sibling entries) and svtgpu_tf_filter_frame against every record the
reference's C left in tests/golden/tf_extreme.bin.  Bit-exact; a record field no consumer reads must be 0.
tests/test_tf_extreme.py asserts that each case reaches the value or the tie named here.

One-line changes these cases catch and the suite before them did not (read from the kernels; no changed kernel was built):

tf_search_kernel (tf_search.hip)
  * variance() with `(int)sum * (int)sum` at 8 bits, or `m * m` in int at 10: max_zero.  A 64x64 block differs by 255
    (1023) everywhere: sum^2 = 1.09e12, the variance must be exactly 0 and everything ends split to 8x8 with zero errors; a
    wrapped square leaves a non-zero error and other flags.  On the drawn fixture |sum| stays near 1e4.
  * the four waves' sse combined in int (or tsse held in 32 signed bits): near_max at 10 bits.  The 64x64 sse is
    4 282 394 624 in (2^31, 2^32) with a sum of 4 188 160, so the error is 64 against 4 x 16 for the 32x32 blocks and every
    block ends on the 64x64 path; a sign-extended sse gives an error near 4e9, which fails `err64 < 1 << 18`, and use64,
    mv32 and err32 of all twelve records change.  (inv_checker_pinned brings the combine a larger sse still, 4 286 582 784,
    but its error fails the 64-vs-32 test either way.)
  * a dropped clip_bd in the x, y or 2-D form of search_step: inv_checker_walk (cells of 2 x 2; the plain checker never
    leaves the range) and the stripes; each form overshoots on evaluated positions, so errors and MVs change.
  * the 8-bit 2-D result not held in int16, or `im` not int16: the same cases, largest intermediate values.
  * a.th32 narrowed to 32 bits: th32_wide (2^32 becomes 0, nothing is skipped, blocks split).
  * `dist <= best`: flat_ref (all 25 positions tie on a non-zero best in every block: the last wins instead of the start),
    v_stripes / h_stripes (the last of the positions tied along the stripes), max_zero is immune (best == 0 skips).
  * positions walked y outer: inv_checker_walk, where (-4, 0) and (0, -4) tie in every block.
  * `(uint64_t)err64 * 14 < sum32 * 16` in 32 bits: inv_checker_pinned, 3.75e9 against 4.29e9 (both beyond 2^31, and
    err64 * 16 beyond 2^32).
tf_err64_kernel
  * variance() with an int square: the forced 64x64 blocks of the max_zero chain, sum = 261 120 per 32x32, square
    6.8e10, err32 exactly 0.
tf_frame_kernel (tf.hip)
  * tf_weight with a 64-bit avg_err product: wide_frame, 96 luma and 192 chroma quadrants beyond 2^32 as the frame kernel
    (before: through the per-block shim only).
  * tf_d_factor without the 32-bit wrap of (col^2 + row^2) << 8: wide_frame's reference 2, MVs of +-16 383.
  * the reference loop or its arrays sized below kMaxRefs, or count held in 16 bits wrongly: refs26 (26 predictors,
    count 14 000, the largest accum).
"""
import ctypes

import numpy as np
import pytest

import svtgpu
import test_tf_gpu as fg
import test_tf_search_gpu as sg
import tf_extreme_cases as xc
import tf_search_cases as tc

pytestmark = pytest.mark.gpu

CASES = xc.search_cases()
CHAINS = xc.chain_cases()
FILTERS = xc.filter_cases()


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_search_matches_the_record(ctx, c):
    st = svtgpu.TfState(ctx, tc.W, tc.H)
    sg.Search(c).run(st)
    gm, gb = sg._read(st, c["n_refs"])
    wm, wb = sg._expected(c["want"])
    sg._same(gm, wm, c["name"] + " motion")
    sg._same(gb, wb, c["name"] + " blocks")
    st.close()


@pytest.mark.parametrize("c", CHAINS, ids=[c["name"] for c in CHAINS])
def test_chain_matches_the_record_and_the_sibling_entries(ctx, c):
    st = svtgpu.TfState(ctx, tc.W, tc.H)
    s, ch = sg.Search(c), sg.Chain(c)
    s.run(st)
    st.compensate_filter_frame(ch.cp, ch.rp, c["pad"], c["pad"], ch.prm, c["P"]["shift"], ch.pp, ch.op)
    gm, gb = sg._read(st, c["n_refs"])
    wm, wb = sg._expected(c["want"], err32=c["err32p"])
    sg._same(gm, wm, c["name"] + " motion")
    sg._same(gb, wb, c["name"] + " blocks with err32 patched")
    pred, out = ch.pred(), ch.out()
    for r in range(c["n_refs"]):
        for p in range(3):
            np.testing.assert_array_equal(pred[r][p], c["pred"][r][p], err_msg="%s predictor %d plane %d" % (c["name"], r, p))
    for p in range(3):
        hh, ww = c["out"][p].shape
        np.testing.assert_array_equal(out[p][:hh, :ww], c["out"][p], err_msg="%s plane %d" % (c["name"], p))
    # the same through svtgpu_tf_predict_frame + svtgpu_tf_filter_frame fed with the records read back
    ch2 = sg.Chain(c)
    mo = (svtgpu.TfMotion * len(gm)).from_buffer_copy(gm.tobytes())
    bl = (svtgpu.TfBlock * len(gb)).from_buffer_copy(gb.tobytes())
    st.predict_frame(ch2.rp, c["pad"], c["pad"], list(mo), c["pic_bd"], c["tf_chroma"], ch2.pp)
    st.filter_frame(ch2.cp, ch2.pp, list(bl), ch2.prm, ch2.op)
    ctx.synchronize()
    for a, b in zip([t for d in ch2.pred() for t in d] + ch2.out(), [t for d in pred for t in d] + out):
        np.testing.assert_array_equal(a, b)
    st.close()


def _run_filter(ctx, c):
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = fg._filter(st, c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], 1, c["bd"], 0)
    st.close()
    return got


@pytest.mark.parametrize("c", FILTERS, ids=[c["name"] for c in FILTERS])
def test_filter_frame_matches_the_record(ctx, c):
    got = _run_filter(ctx, c)
    for p in range(3):
        hh, ww = c["out"][p].shape
        np.testing.assert_array_equal(got[p][:hh, :ww], c["out"][p], err_msg="%s plane %d" % (c["name"], p))
    if c["n_refs"] == 26:  # 13 weights of 1000 on the centre's own samples, 13 of 0: the output is the centre
        assert (c["wt"].reshape(26, -1)[0::2] == 1000).all() and not c["wt"].reshape(26, -1)[1::2].any()
        for p in range(3):
            np.testing.assert_array_equal(got[p], c["centre"][p], err_msg="%s plane %d" % (c["name"], p))


def test_block_shim_on_a_quadrant_of_wide_frame_that_wraps():
    """svtgpu_tf_apply_planewise_medium_hbd on the first 32x32 block of wide_frame's full-range reference whose luma
    product passes 2^32, from zeroed accumulators: count is the record's weight of each quadrant, accum weight * predictor."""
    c = FILTERS[0]
    wide = c["wide"].reshape(c["nblk"], c["n_refs"], 4, 3, 4)
    blk, idx = [(b, i) for b in range(c["nblk"]) for i in range(4) if wide[b, 1, i, 0].any()][0]
    wt = c["wt"].reshape(c["nblk"], c["n_refs"], 4, 3, 4)[blk, 1, idx]
    m = c["metas"][1][blk]
    blkrec = svtgpu.TfBlock.make(m["split"], m["mv32"], m["mv16"], m["err32"], m["err16"])
    prm = svtgpu.TfParams.make(c["decay"], c["mv_dist_th"], 1, c["bd"], 0)

    def sub(pl, p):
        s, bc = 32 >> (p > 0), c["w"] // 64 + 1
        y, x = ((blk // bc) * 64 + (idx >> 1) * 32) >> (p > 0), ((blk % bc) * 64 + (idx & 1) * 32) >> (p > 0)
        return np.ascontiguousarray(pl[p][y:y + s, x:x + s])
    src, pre = [sub(c["centre"], p) for p in range(3)], [sub(c["refs"][1], p) for p in range(3)]
    acc = [np.zeros(a.shape, np.uint32) for a in pre]
    cnt = [np.zeros(a.shape, np.uint16) for a in pre]
    pp = svtgpu.ptr
    svtgpu.lib().svtgpu_tf_apply_planewise_medium_hbd(
        ctypes.byref(blkrec), idx, ctypes.byref(prm), pp(src[0]), 32, pp(pre[0]), 32, pp(src[1]), pp(src[2]), 16, pp(pre[1]),
        pp(pre[2]), 16, 32, 32, 1, 1, pp(acc[0]), pp(cnt[0]), pp(acc[1]), pp(cnt[1]), pp(acc[2]), pp(cnt[2]), c["bd"])
    for p in range(3):
        h = 16 >> (p > 0)
        want = np.repeat(np.repeat(wt[p].reshape(2, 2), h, axis=0), h, axis=1)
        np.testing.assert_array_equal(cnt[p], want, err_msg="count %d" % p)
        np.testing.assert_array_equal(acc[p], want.astype(np.uint32) * pre[p], err_msg="accum %d" % p)


def test_everything_split_then_nothing_split_on_one_state(ctx):
    """max_zero (every 8x8 MV written), then inv_checker_pinned, no wait in between: the read gives the second picture's
    records whole, so no 8x8 or 16x16 field of the first survives where the second leaves a block unsplit."""
    for bd in (8, 10):
        a = next(c for c in CASES if c["cls"] == "max_zero" and c["P"]["bd"] == bd)
        b = next(c for c in CASES if c["cls"] == "th32_wide" and c["P"]["bd"] == bd)  # pinned, and nothing split at all
        p = next(c for c in CASES if c["cls"] == "inv_checker_pinned" and c["P"]["bd"] == bd)
        st = svtgpu.TfState(ctx, tc.W, tc.H)
        sa, sb, sp = sg.Search(a), sg.Search(b), sg.Search(p)
        for s, c in ((sb, b), (sp, p)):
            sa.run(st)
            s.run(st)
            gm, gb = sg._read(st, 2)
            wm, wb = sg._expected(c["want"])
            sg._same(gm, wm, c["name"] + " motion after max_zero")
            sg._same(gb, wb, c["name"] + " blocks after max_zero")
        st.close()
