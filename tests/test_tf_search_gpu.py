"""The temporal filter's sub-pel motion search on the MI355X: svtgpu_tf_search_frame + svtgpu_tf_search_read against every
record of the reference's fixture (tests/golden/tf_search.bin), svtgpu_tf_compensate_filter_frame against both chain
records and against the two sibling entries fed with the read-back records, two pictures back to back on one state, and
the read clamp at the encoder's 68-sample border.  Bit-exact; a record field no consumer reads must be 0."""
import ctypes

import numpy as np
import pytest
import torch

import interp_cases as ic
import svtgpu
import tf_search_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.search_cases()
CHAINS = tc.chain_cases()
MOTION_DT = np.dtype([("mv64", "<i2", 2), ("use64", "u1"), ("r0", "u1", 3), ("split32", "u1", 4), ("split16", "u1", 16),
                      ("r1", "u1", 4), ("mv32_x", "<i2", 4), ("mv32_y", "<i2", 4), ("mv16_x", "<i2", 16), ("mv16_y", "<i2", 16),
                      ("mv8_x", "<i2", 64), ("mv8_y", "<i2", 64)])
BLOCK_DT = np.dtype([("split32", "<i4", 4), ("mv32_x", "<i2", 4), ("mv32_y", "<i2", 4), ("mv16_x", "<i2", 16),
                     ("mv16_y", "<i2", 16), ("err32", "<u8", 4), ("err16", "<u8", 16)])
assert MOTION_DT.itemsize == 368 and BLOCK_DT.itemsize == 256


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype == np.uint16 else np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _expected(rec, err32=None):
    """The two record arrays the device must hold, whole: every field the fixture does not name is 0."""
    mo, bl = tc.motion_block_arrays(rec)
    n = rec["use64"].size
    m, b = np.zeros(n, MOTION_DT), np.zeros(n, BLOCK_DT)
    m["mv64"], m["use64"] = mo["mv64"].reshape(n, 2), mo["use64"].reshape(n)
    m["split32"], m["split16"] = mo["split32"].reshape(n, 4), mo["split16"].reshape(n, 16)
    b["split32"] = bl["split32"].reshape(n, 4)
    for f, k in (("mv32", 4), ("mv16", 16), ("mv8", 64)):
        m[f + "_x"], m[f + "_y"] = mo[f].reshape(n, k, 2)[..., 0], mo[f].reshape(n, k, 2)[..., 1]
    for f, k in (("mv32", 4), ("mv16", 16)):
        b[f + "_x"], b[f + "_y"] = bl[f].reshape(n, k, 2)[..., 0], bl[f].reshape(n, k, 2)[..., 1]
    b["err32"], b["err16"] = (bl["err32"] if err32 is None else err32).reshape(n, 4), bl["err16"].reshape(n, 16)
    return m, b


def _same(got, want, what):
    for f in want.dtype.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg="%s: %s" % (what, f))


def _ref_planes(ts, arrays, pad):
    return svtgpu.TfPlanes.make([t.data_ptr() + ((pad >> (p > 0)) * (a.shape[1] + 1)) * a.itemsize
                                 for p, (t, a) in enumerate(zip(ts, arrays))], [a.shape[1] for a in arrays])


def _planes(ts):
    return svtgpu.TfPlanes.make([t.data_ptr() for t in ts], [tc.AW, tc.AW >> 1, tc.AW >> 1])


def _params(P):
    return svtgpu.TfSearchParams.make(P["modes"], P["use_2tap"], P["shift"], P["enable8"], P["early"], P["th32"], P["bd"])


def _fullpel(c, n_refs=None):
    fp = c["fullpel"]
    return [svtgpu.TfFullpel.make(fp["mv64"][r][b], fp["mv32"][r][b], fp["mv16"][r][b], fp["mv8"][r][b], c["force64"][r][b])
            for r in range(n_refs or c["n_refs"]) for b in range(tc.NBLK)]


class Search:
    """The device copies of a case's search planes, kept alive while calls are queued."""

    def __init__(self, c, refs=None):
        pics = tc.case_pictures(c)
        self.c, self.refs = c, [r for r in pics["ref8"]] if refs is None else refs
        self.dc = [_dev(a) for a in pics["cen8"]]
        self.dr = [[_dev(a) for a in r] for r in self.refs]
        self.cp = _planes(self.dc)
        self.rp = [_ref_planes(t, r, c["pad"]) for t, r in zip(self.dr, self.refs)]

    def run(self, st, border=None, n_refs=None):
        n = n_refs or self.c["n_refs"]
        b = border or (self.c["pad"], self.c["pad"])
        st.search_frame(self.cp, self.rp[:n], b[0], b[1], _fullpel(self.c, n), _params(self.c["P"]))


def _read(st, n_refs):
    mo, bl = st.search_read(n_refs)
    return np.frombuffer(mo, MOTION_DT).copy(), np.frombuffer(bl, BLOCK_DT).copy()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_search_matches_the_record(ctx, c):
    st = svtgpu.TfState(ctx, tc.W, tc.H)
    Search(c).run(st)
    gm, gb = _read(st, c["n_refs"])
    wm, wb = _expected(c["want"])
    _same(gm, wm, c["name"] + " motion")
    _same(gb, wb, c["name"] + " blocks")
    st.close()


class Chain:
    """The device planes of a chain case at the pictures' bit depth: centre, references, predictors, output."""

    def __init__(self, c):
        pics = tc.case_pictures(c)
        dt = pics["cen"][0].dtype
        self.c, self.dt = c, dt
        self.dc = [_dev(a) for a in pics["cen"]]
        self.dr = [[_dev(a) for a in r] for r in pics["ref"]]
        self.dp = [[_dev(np.full((tc.AH >> (p > 0), tc.AW >> (p > 0)), 5, dt)) for p in range(3)] for _ in pics["ref"]]
        self.do = [_dev(np.full(a.shape, 5, dt)) for a in pics["cen"]]
        self.cp, self.op = _planes(self.dc), _planes(self.do)
        self.rp = [_ref_planes(t, r, c["pad"]) for t, r in zip(self.dr, pics["ref"])]
        self.pp = [_planes(d) for d in self.dp]
        self.prm = svtgpu.TfParams.make(c["decay"], c["mv_dist_th"], c["tf_chroma"], c["pic_bd"], 0)

    def pred(self):
        return [[_host(t, self.dt) for t in d] for d in self.dp]

    def out(self):
        return [_host(t, self.dt) for t in self.do]


@pytest.mark.parametrize("c", CHAINS, ids=[c["name"] for c in CHAINS])
def test_chain_matches_the_record_and_the_sibling_entries(ctx, c):
    st = svtgpu.TfState(ctx, tc.W, tc.H)
    s, ch = Search(c), Chain(c)
    s.run(st)
    st.compensate_filter_frame(ch.cp, ch.rp, c["pad"], c["pad"], ch.prm, c["P"]["shift"], ch.pp, ch.op)  # no wait in between
    gm, gb = _read(st, c["n_refs"])
    wm, wb = _expected(c["want"], err32=c["err32p"])
    _same(gm, wm, c["name"] + " motion")
    _same(gb, wb, c["name"] + " blocks with err32 patched")
    pred, out = ch.pred(), ch.out()
    for r in range(c["n_refs"]):
        for p in range(3):
            np.testing.assert_array_equal(pred[r][p], c["pred"][r][p], err_msg="%s predictor %d plane %d" % (c["name"], r, p))
    for p in range(3):
        hh, ww = c["out"][p].shape
        np.testing.assert_array_equal(out[p][:hh, :ww], c["out"][p], err_msg="%s plane %d" % (c["name"], p))
    # the same through svtgpu_tf_predict_frame + svtgpu_tf_filter_frame fed with the records read back
    ch2 = Chain(c)
    mo = (svtgpu.TfMotion * len(gm)).from_buffer_copy(gm.tobytes())
    bl = (svtgpu.TfBlock * len(gb)).from_buffer_copy(gb.tobytes())
    st.predict_frame(ch2.rp, c["pad"], c["pad"], list(mo), c["pic_bd"], c["tf_chroma"], ch2.pp)
    st.filter_frame(ch2.cp, ch2.pp, list(bl), ch2.prm, ch2.op)
    ctx.synchronize()
    for a, b in zip([t for d in ch2.pred() for t in d] + ch2.out(), [t for d in pred for t in d] + out):
        np.testing.assert_array_equal(a, b)
    st.close()


def test_two_pictures_back_to_back_leave_no_residue(ctx):
    """Three searches queued on one state with no wait in between: a set that splits nearly everything, the force64 set,
    the first again.  Each read gives its own record, whole: nothing of the previous picture stays in a field the next one
    does not write.  Then the 8-bit chain twice on the same state gives the same pictures."""
    a, b = CASES[0], CASES[8]
    st = svtgpu.TfState(ctx, tc.W, tc.H)
    sa, sb = Search(a), Search(b)
    sa.run(st)
    sb.run(st)
    gm, gb = _read(st, 2)
    wm, wb = _expected(b["want"])
    _same(gm, wm, "second picture motion")
    _same(gb, wb, "second picture blocks")
    sa.run(st)
    gm, gb = _read(st, 2)
    wm, wb = _expected(a["want"])
    _same(gm, wm, "third picture motion")
    _same(gb, wb, "third picture blocks")
    c = CHAINS[0]
    s, outs = Search(c), []
    for _ in range(2):
        ch = Chain(c)
        s.run(st)
        st.compensate_filter_frame(ch.cp, ch.rp, c["pad"], c["pad"], ch.prm, c["P"]["shift"], ch.pp, ch.op)
        outs.append(ch)
    ctx.synchronize()
    for p in range(3):
        np.testing.assert_array_equal(outs[0].out()[p], outs[1].out()[p])
        hh, ww = c["out"][p].shape
        np.testing.assert_array_equal(outs[1].out()[p][:hh, :ww], c["out"][p])
    st.close()


@pytest.mark.parametrize("c", [CASES[0], CASES[9]], ids=["8-bit", "10-bit"])
def test_search_with_the_encoders_border(ctx, c):
    """border 68 on a plane allocated to 80 with noise beyond 68.  One reference, every block on the 64x64 path with a
    full-pel MV at the MV clamp's bound (left / top: -(4 + 64) samples from the picture; right / bottom the same beyond the
    far edge), so that the window lies against the border and every position of non-zero phase reaches 71 samples out.  The
    padding inside the border is flat: with the clamp every position of such a block ties and the start wins; reading the
    noise beyond the border moves the best.  The device must give what the restatement gives from a plane whose samples
    beyond 68 are overwritten; the restatement without the clamp differs (asserted), so a kernel that does not clamp fails
    here, and it would still read allocated memory only."""
    fp = dict(c["fullpel"], mv64=c["fullpel"]["mv64"].copy())
    fp["mv64"][0] = [(-68, -68), (tc.W - 128 + 67, -68), (tc.W - 192 + 67, 2), (-68, tc.H - 128 + 67), (tc.W - 128 + 67, tc.H - 128 + 67),
                     (tc.W - 192 + 67, tc.H - 128 + 67)]
    c = dict(c, n_refs=1, force64=np.ones((tc.NR, tc.NBLK), np.uint8), fullpel=fp)
    rng = np.random.default_rng(68 + c["P"]["bd"])
    ref = tc.pictures(c["pic_bd"], c["low8"])["ref8"][0]
    k, pad = c["pad"] - 68, c["pad"]
    flat = np.full(ref[0].shape, 100, ref[0].dtype)
    flat[pad:pad + tc.H, pad:pad + tc.W] = ref[0][pad:pad + tc.H, pad:pad + tc.W]
    noisy, cut = rng.integers(0, 1 << c["P"]["bd"], flat.shape).astype(flat.dtype), np.full(flat.shape, 1, flat.dtype)
    inner = (slice(k, flat.shape[0] - k), slice(k, flat.shape[1] - k))
    noisy[inner], cut[inner] = flat[inner], flat[inner]
    want, free = tc.search_frame(c, border=(68, 68), refs=[cut]), tc.search_frame(c, refs=[noisy])
    assert (want["mv64"] != free["mv64"]).any(), "the clamp changes nothing"
    st = svtgpu.TfState(ctx, tc.W, tc.H)
    s = Search(c, refs=[[noisy] + ref[1:]])
    s.run(st, border=(68, 68), n_refs=1)
    gm, gb = _read(st, 1)
    wm, wb = _expected({f: v[:1] for f, v in want.items()})
    _same(gm, wm, "motion")
    _same(gb, wb, "blocks")
    # the same plane with 80 declared readable: the reference's own reads, no clamp
    s.run(st, border=(80, 80), n_refs=1)
    gm, gb = _read(st, 1)
    wm, wb = _expected({f: v[:1] for f, v in free.items()})
    _same(gm, wm, "motion, no clamp")
    _same(gb, wb, "blocks, no clamp")
    st.close()


def test_search_refuses_misaligned_narrow_planes_and_wide_mvs(ctx):
    """SVTGPU_ERR_INVALID_ARG before any launch, on a real state."""
    c = CASES[0]
    st = svtgpu.TfState(ctx, tc.W, tc.H)
    s = Search(c)
    L, prm = svtgpu.lib(), _params(c["P"])
    fp = (svtgpu.TfFullpel * (2 * tc.NBLK))(*_fullpel(c))
    ra = (svtgpu.TfPlanes * 2)(*s.rp)

    def rc(centre=s.cp, refs=ra, border=68, fullpel=fp):
        return L.svtgpu_tf_search_frame(st.h, ctypes.byref(centre), refs, 2, border, border, fullpel, ctypes.byref(prm), None)

    def changed(pl, ptr=0, stride=0):
        q = svtgpu.TfPlanes.make([pl.plane[k] for k in range(3)], [pl.stride[k] for k in range(3)])
        q.plane[0], q.stride[0] = pl.plane[0] + ptr, pl.stride[0] + stride
        return q
    assert rc(centre=changed(s.cp, ptr=1)) == -1 and rc(centre=changed(s.cp, stride=8)) == -1 and rc(centre=changed(s.cp, stride=-64)) == -1
    assert rc(refs=(svtgpu.TfPlanes * 2)(s.rp[0], changed(s.rp[1], stride=-(2 * c["pad"])))) == -1
    assert rc(border=81) == -1  # the stride cannot hold width + 2 * border
    wide = (svtgpu.TfFullpel * (2 * tc.NBLK))(*_fullpel(c))
    wide[7].mv8_y[63] = 2048
    assert rc(fullpel=wide) == -1
    wide[7].mv8_y[63] = -2047
    assert rc(fullpel=wide) == 0 and rc() == 0
    assert L.svtgpu_tf_search_read(st.h, 1, (svtgpu.TfMotion * 12)(), (svtgpu.TfBlock * 12)(), None) == -1  # 2 were searched
    gm, gb = _read(st, 2)
    wm, wb = _expected(c["want"])
    _same(gm, wm, "motion")
    _same(gb, wb, "blocks")
    # a picture without references ends the previous picture's records: nothing to read, and the chain runs on none
    assert L.svtgpu_tf_search_frame(st.h, ctypes.byref(s.cp), None, 0, 68, 68, None, ctypes.byref(prm), None) == 0
    assert L.svtgpu_tf_search_read(st.h, 2, (svtgpu.TfMotion * 12)(), (svtgpu.TfBlock * 12)(), None) == -1
    ch = Chain(CHAINS[0])
    assert L.svtgpu_tf_compensate_filter_frame(st.h, ctypes.byref(ch.cp), None, 2, 68, 68, ctypes.byref(ch.prm), 0, None,
                                               ctypes.byref(ch.op), None) == -1
    assert L.svtgpu_tf_compensate_filter_frame(st.h, ctypes.byref(ch.cp), None, 0, 68, 68, ctypes.byref(ch.prm), 0, None,
                                               ctypes.byref(ch.op), None) == 0
    ctx.synchronize()
    for got, cen in zip(ch.out(), tc.pictures(8)["cen"]):
        np.testing.assert_array_equal(got, cen)  # the centre alone: (1000 * c + 500) / 1000
    st.close()
