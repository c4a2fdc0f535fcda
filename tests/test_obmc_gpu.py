"""OBMC distortion parity on the MI355X: the 66 RTCD shims against every block record of tests/golden/obmc.bin (the
reference's own sad_av1.c / variance.c), and the batched full-pel search against the fixture's walk records (the
reference's svt_av1_obmc_full_pixel_search) and against the numpy restatement of tests/obmc_cases.py (held to the
fixture by tests/test_obmc.py) on a mixed batch.  Bit-exact."""
import ctypes

import numpy as np
import pytest

import obmc_cases as oc
import svtgpu

pytestmark = pytest.mark.gpu
P = lambda a: ctypes.c_void_p(a.ctypes.data)
INVALID_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def luma_frame(ctx, y):
    h, w = y.shape
    f = svtgpu.Frame(ctx, w, h, 8)
    f.upload([y, np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)])
    return f


def shim_values(w, h, win, stride, wsrc, mask):
    """The 11 values of a blk<k>_res row through the three shims of size w x h; win has `stride` bytes per row."""
    L = svtgpu.lib()
    sse = ctypes.c_uint(0)
    ws, mk = np.ascontiguousarray(wsrc, np.int32), np.ascontiguousarray(mask, np.int32)
    out = [getattr(L, "svtgpu_aom_obmc_sad%dx%d" % (w, h))(P(win), stride, P(ws), P(mk))]
    out.append(getattr(L, "svtgpu_aom_obmc_variance%dx%d" % (w, h))(P(win), stride, P(ws), P(mk), ctypes.byref(sse)))
    out.append(sse.value)
    for xo, yo in oc.SUBPEL:
        out.append(getattr(L, "svtgpu_aom_obmc_sub_pixel_variance%dx%d" % (w, h))(P(win), stride, xo, yo, P(ws), P(mk),
                                                                                 ctypes.byref(sse)))
        out.append(sse.value)
    return np.array(out, np.uint32)


@pytest.mark.parametrize("k", range(22))
def test_shims_match_block_records(ctx, k):
    w, h = oc.SIZES[k]
    for case in range(4):
        win, wsrc, mask, want = oc.block_case(k, case)
        np.testing.assert_array_equal(shim_values(w, h, win, w + 1, wsrc, mask), want,
                                      err_msg="%dx%d case %d" % (w, h, case))


def test_shims_with_a_wide_stride(ctx):
    """pre_stride larger than W: the window of a block record placed inside a wider buffer."""
    for k in (0, 6, 15):  # 4x4, 16x16, 128x128
        w, h = oc.SIZES[k]
        win, wsrc, mask, want = oc.block_case(k, 0)
        stride = w + 37
        wide = np.full((h + 1, stride), 0xA5, np.uint8)
        wide[:, :w + 1] = win
        np.testing.assert_array_equal(shim_values(w, h, wide, stride, wsrc, mask), want, err_msg="%dx%d" % (w, h))


def run_batch(ctx, frames, items, wsrcs, masks, costs, batch=None):
    rows, wm, cp = oc.pack(items, wsrcs, masks, costs)
    h, w = frames[0].shape
    b = batch or svtgpu.ObmcBatch(ctx, w, h, len(frames), max(len(items), 1))
    b.set_items(rows, wm, cp)
    refs = [luma_frame(ctx, f) for f in frames]
    b.search(refs)
    return b, b.read()  # synchronous: the references live until the search has run


def test_batch_matches_walk_records(ctx):
    frames = [np.ascontiguousarray(f) for f in oc.fixture()["walk_frames"]]
    cases = oc.walk_cases()
    _, got = run_batch(ctx, frames, *zip(*[(it, ws, mk, ct) for it, ws, mk, ct, _ in cases]))
    assert len(got) == len(cases)
    for i, ((it, _, _, _, res), r) in enumerate(zip(cases, got)):
        assert (int(r["mv_col"]), int(r["mv_row"]), int(r["variance"]), int(r["sse"])) == \
            (int(res[0]), int(res[1]), int(res[2]) & 0xFFFFFFFF, int(res[3]) & 0xFFFFFFFF), (i, it, r, res)


@pytest.fixture(scope="module")
def mixed():
    """The mixed batch and the restatement's results of it, computed once."""
    frames, items, wsrcs, masks, costs = oc.mixed_batch()
    padded = [oc.pad_frame(f) for f in frames]
    want = [oc.walk(*padded[it["frame"]], it, ws, mk, ct) for it, ws, mk, ct in zip(items, wsrcs, masks, costs)]
    return frames, items, wsrcs, masks, costs, want


def check_results(got, want, items):
    assert len(got) == len(want)
    for i, (r, w) in enumerate(zip(got, want)):
        assert tuple(int(r[k]) for k in ("mv_col", "mv_row", "best_sad", "variance", "sse", "steps")) == w, \
            (i, items[i], r, w)


def test_batch_matches_restatement_on_a_mixed_batch(ctx, mixed):
    frames, items, wsrcs, masks, costs, want = mixed
    assert len(items) == 40 and {(it["w"], it["h"]) for it in items} >= {(4, 4), (64, 128), (128, 64), (128, 128)}
    assert {it["cost_mode"] for it in items} == {0, 1} and {it["search_range"] for it in items} == {8, 16}
    assert max(w[5] for w in want) >= 4  # the batch holds walks of several steps
    _, got = run_batch(ctx, frames, items, wsrcs, masks, costs)
    check_results(got, want, items)


def test_second_search_on_the_same_batch_has_no_stale_state(ctx, mixed):
    frames, items, wsrcs, masks, costs, want = mixed
    b, got = run_batch(ctx, frames, items, wsrcs, masks, costs)
    check_results(got, want, items)
    pick = [33, 7, 18, 2, 25]  # fewer items, another order
    sub = [[seq[i] for i in pick] for seq in (items, wsrcs, masks, costs)]
    _, got2 = run_batch(ctx, frames, *sub, batch=b)
    check_results(got2, [want[i] for i in pick], sub[0])
    # the earlier list's results beyond the new count are not readable
    out = np.zeros(len(items), svtgpu.OBMC_RESULT_DTYPE)
    assert svtgpu.lib().svtgpu_obmc_read(b.h, P(out), 0, len(items), None) == INVALID_ARG


def test_argument_checks(ctx, mixed):
    frames, items, wsrcs, masks, costs, _ = mixed
    L = svtgpu.lib()
    rows, wm, cp = oc.pack(items[:4], wsrcs[:4], masks[:4], costs[:4])
    b = svtgpu.ObmcBatch(ctx, 192, 136, 2, 8)
    refs = [luma_frame(ctx, f) for f in frames]
    arr = (ctypes.c_void_p * 2)(*[r.h for r in refs])
    for bad in (dict(w=12, h=16), dict(search_range=17), dict(ref=2), dict(ref=-1), dict(wm_offset=wm.size)):
        lst = [dict(r) for r in rows]
        lst[2].update(bad)
        with pytest.raises(svtgpu.SvtGpuError, match="invalid argument"):
            b.set_items(lst, wm, cp)
        # the rejected list left nothing to launch: any item range is refused
        assert L.svtgpu_obmc_search(b.h, arr, 0, 1, None) == INVALID_ARG
    assert L.svtgpu_obmc_set_items(b.h, None, 9, P(wm), wm.size, P(cp), cp.size, None) == INVALID_ARG  # > max_items
    b.set_items(rows, wm, cp)
    assert L.svtgpu_obmc_search(b.h, arr, 0, 5, None) == INVALID_ARG
    assert L.svtgpu_obmc_search(b.h, None, 0, 4, None) == INVALID_ARG
    b.search(refs)
    assert len(b.read()) == 4


def test_batch_matches_restatement_on_tie_and_full_magnitude_content(ctx):
    """obmc_cases.extreme_batch (tests/test_obmc.py asserts what its items reach): a flat frame, stripes whose two
    neighbours across tie at the first step, and WSRC_MAX against a zero frame with a 255 corner, with an MV cost whose
    32-bit product wraps.  mv_col, mv_row, best_sad, variance, sse and steps, exactly."""
    frames, items, wsrcs, masks, costs, _ = oc.extreme_batch()
    padded = [oc.pad_frame(f) for f in frames]
    want = [oc.walk(*padded[it["frame"]], it, ws, mk, ct) for it, ws, mk, ct in zip(items, wsrcs, masks, costs)]
    _, got = run_batch(ctx, frames, items, wsrcs, masks, costs)
    check_results(got, want, items)
