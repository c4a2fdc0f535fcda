"""The deblocking tile item (dlf_tile_item: apply and level trials) on grids built to break its apron trimming and its
packed vertical-pass write-back (tests/dlf_item_cases.py): 14-tap luma edges on both tile boundaries with lengths 4, 8
and 14 (chroma 4 and 6) in neighbouring 4-sample segments, 4-tap edges on the item's outermost edge rows and columns
(y0-4, y0+68: the only length an edge record can take there, see dlf_item_cases), runs of length-8 edges 8 samples
apart, a level class at level 0 on one side of an edge, partial last tiles.  Bit-exact against the C oracle: the
filtered planes (oracle.dlf_frame), their SSE against the source, and the levels picked by searches whose first round
tries two levels per plane and by searches that try level 0 for a whole picture (oracle.dlf_pick)."""
import numpy as np
import pytest

import dlf_item_cases as ic
import oracle
import svtgpu
import synth

pytestmark = pytest.mark.gpu

APPLY_LEVELS = [(40, 36, 20, 28), (63, 63, 63, 63), (5, 0, 0, 9)]
PICK_STARTS = [(16, 16, 8, 8), (0, 0, 0, 0), (2, 1, 1, 2)]  # two levels per plane in round 1; level 0 tried


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


@pytest.fixture(scope="module", params=ic.SHAPES, ids=lambda s: "%dx%d_bd%d" % s)
def case(request, ctx):
    w, h, bd = request.param
    src, rec = synth.frame_pair(w, h, bd, seed=0x5EED0400 + bd)
    R, S = svtgpu.Frame(ctx, w, h, bd), svtgpu.Frame(ctx, w, h, bd)
    R.upload(rec)
    S.upload(src)
    mi = ic.mode_info(w, h, 7)
    st = svtgpu.DlfState(ctx, w, h)
    st.set_mode_info(mi)
    return dict(w=w, h=h, bd=bd, src=src, rec=rec, R=R, S=S, mi=mi, st=st)


@pytest.mark.parametrize("levels", APPLY_LEVELS)
def test_item_apply(ctx, case, levels):
    c = case
    prm = ic.params(levels)
    want = oracle.dlf_frame(c["rec"], c["bd"], c["mi"], prm)
    O = svtgpu.Frame(ctx, c["w"], c["h"], c["bd"])
    c["st"].filter_to(c["R"], O, prm)
    got = O.download()
    for p in range(3):
        assert np.array_equal(got[p], want[p]), p
        sse = int(((want[p].astype(np.int64) - c["src"][p].astype(np.int64)) ** 2).sum())
        assert svtgpu.plane_sse(O, c["S"], p) == sse, p
    assert any(not np.array_equal(want[p], c["rec"][p]) for p in range(3))


@pytest.mark.parametrize("start", PICK_STARTS)
def test_item_trials(ctx, case, start):
    """The trial launches behind both searches: the host-driven bisection (svtgpu_dlf_pick) and the device one
    (svtgpu_dlf_pick_async), each against the oracle's search -- equal levels mean equal trial SSEs at every step."""
    c = case
    prm = ic.params(start)
    want = oracle.dlf_pick(c["rec"], c["src"], c["bd"], c["mi"], prm, 0, 0, 0, 0, 0)
    got = c["st"].pick(c["R"], c["S"], prm, 0, 0, 0, 0, 0)
    assert got.levels() == want.levels()
    c["st"].pick_async(c["R"], c["S"], prm, 0, 0, 0, 0, 0)
    assert c["st"].read_levels().levels() == want.levels()
    back = c["R"].download()  # a trial never modifies the recon
    assert all(np.array_equal(back[p], c["rec"][p]) for p in range(3))
