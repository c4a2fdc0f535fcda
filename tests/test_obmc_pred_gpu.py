"""AV1 OBMC prediction on the MI355X: svtgpu_obmc_predict_batch against every record of the reference's fixture
(tests/golden/obmc_pred.bin), and -- on pictures the fixture does not hold, with the read clamp acting, with the largest and
the smallest block in one list -- against the numpy restatement that tests/test_obmc_pred.py holds to those records.
Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import interp_cases as ic
import obmc_pred_cases as oc
import svtgpu

pytestmark = pytest.mark.gpu

RECORDS = oc.records()
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


def _blocks(blocks):
    return [svtgpu.ObmcBlock.make(b["x"], b["y"], b["w"], b["h"], b["ref"], b["mv"], b["fx"], b["fy"], b["above"], b["left"])
            for b in blocks]


def _prepare(w, h, refs, pad, fill=FILL):
    """Device copies of padded reference pictures and predictor planes prefilled with `fill`; the predictor rows are padded to
    16 bytes."""
    dt = refs[0][0].dtype
    dr = [[_dev(a) for a in r] for r in refs]
    strides = [-(-(w >> (p > 0)) * dt.itemsize // 16) * 16 // dt.itemsize for p in range(3)]
    dp = [_dev(np.full((h >> (p > 0), strides[p]), fill, dt)) for p in range(3)]
    rp = [svtgpu.TfPlanes.make([t[p].data_ptr() + ((pad >> (p > 0)) * (r[p].shape[1] + 1)) * r[p].itemsize for p in range(3)],
                               [r[p].shape[1] for p in range(3)]) for t, r in zip(dr, refs)]
    pp = svtgpu.TfPlanes.make([t.data_ptr() for t in dp], strides)
    return rp, pp, dp, dr


def _predict(st, refs, pad, blocks, bd, chroma, border):
    rp, pp, dp, dr = _prepare(st.width, st.height, refs, pad)
    st.obmc_predict_batch(rp, border[0], border[1], _blocks(blocks), bd, chroma, pp)
    st.ctx.synchronize()
    return [_host(t, refs[0][0].dtype)[:, :st.width >> (p > 0)] for p, t in enumerate(dp)]


def _written(blocks, w, h, p):
    m = np.zeros((h >> (p > 0), w >> (p > 0)), bool)
    for b in blocks:
        m[b["y"] >> (p > 0):(b["y"] + b["h"]) >> (p > 0), b["x"] >> (p > 0):(b["x"] + b["w"]) >> (p > 0)] = True
    return m


@pytest.mark.parametrize("c", RECORDS, ids=[c["name"] for c in RECORDS])
def test_batch_matches_records(ctx, c):
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _predict(st, c["refs"], c["pad"], c["blocks"], c["bd"], c["chroma"], (c["pad"], c["pad"]))
    for p, want in enumerate(c["pred"]):
        m = _written(c["blocks"], c["w"], c["h"], p)
        np.testing.assert_array_equal(got[p][m], want[m], err_msg="%s plane %d" % (c["name"], p))
        assert (got[p][~m] == FILL).all(), c["name"]  # nothing outside the listed blocks
    if not c["chroma"]:
        assert (got[1] == FILL).all() and (got[2] == FILL).all(), c["name"]
    st.close()


def _noise_refs(rng, bd, w, h, pad, n=3):
    dt = np.uint16 if bd > 8 else np.uint8
    return [[rng.integers(0, 1 << bd, ((h + 2 * pad) >> (p > 0), (w + 2 * pad) >> (p > 0))).astype(dt) for p in range(3)]
            for _ in range(n)]


def _cut(refs, pad, border):
    """The planes with everything beyond the declared border overwritten."""
    out = []
    for r in refs:
        planes = []
        for p, a in enumerate(r):
            k = (pad - border) >> (p > 0)
            b = np.full(a.shape, 1, a.dtype)
            b[k:a.shape[0] - k, k:a.shape[1] - k] = a[k:a.shape[0] - k, k:a.shape[1] - k]
            planes.append(b)
        out.append(planes)
    return out


def _span(rng, rel, size, far=None):
    mv = [int(rng.integers(-40, 41)), int(rng.integers(-40, 41))]
    if far is not None:
        mv[far[0]] = far[1]
    return dict(rel=rel, size=size, ref=int(rng.integers(0, 3)), fx=int(rng.integers(0, 4)), fy=int(rng.integers(0, 4)), mv=tuple(mv))


@pytest.mark.parametrize("bd", [8, 10])
def test_largest_and_smallest_block_in_one_list_with_the_read_clamp_acting(ctx, bd):
    """One 128 x 128 block with four spans above and four left (mixed lengths, a gap) and one 8 x 8 block with one span each
    way, in a 160 x 144 picture of noise allocated with 160 samples around it, 24 declared readable; some MVs far outside,
    so the read clamp acts.  The device gives what the restatement gives from planes whose samples beyond the declared
    border are overwritten; without the clamp the result differs (asserted on the restatement)."""
    w, h, pad, border = 160, 144, 160, 24
    rng = np.random.default_rng(77 + bd)
    refs = _noise_refs(rng, bd, w, h, pad)
    big = dict(x=32, y=16, w=128, h=128, ref=1, fx=0, fy=2, mv=(13, -27),
               above=[_span(rng, 0, 2), _span(rng, 2, 4, (1, -2000)), _span(rng, 8, 8), _span(rng, 16, 16, (0, 3000))],
               left=[_span(rng, 0, 4, (0, -2500)), _span(rng, 4, 2), _span(rng, 8, 8, (1, 2600)), _span(rng, 16, 16)])
    small = dict(x=8, y=8, w=8, h=8, ref=2, fx=1, fy=3, mv=(-1300, 5), above=[_span(rng, 0, 2)], left=[_span(rng, 0, 2, (1, 1900))])
    blocks = [big, small]
    want = oc.predict_batch(_cut(refs, pad, border), pad, blocks, bd, w, h, 1, border=(border, border), fill=FILL)
    free = oc.predict_batch(refs, pad, blocks, bd, w, h, 1, border=(pad, pad), fill=FILL)
    assert all((a != b).any() for a, b in zip(want, free)), "the read clamp changes nothing"
    st = svtgpu.TfState(ctx, w, h)
    got = _predict(st, refs, pad, blocks, bd, 1, (border, border))
    for p in range(3):
        np.testing.assert_array_equal(got[p], want[p], err_msg="plane %d" % p)
    st.close()


def test_two_calls_back_to_back_keep_their_own_lists(ctx):
    c = RECORDS[0]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    other = [dict(b, mv=(b["mv"][1], b["mv"][0]), fx=b["fy"], fy=b["fx"], above=b["above"][:1], left=[]) for b in c["blocks"][::-1]]
    rp, pa, a, dr = _prepare(c["w"], c["h"], c["refs"], c["pad"])
    _, pb, b, _ = _prepare(c["w"], c["h"], c["refs"], c["pad"])
    st.obmc_predict_batch(rp, c["pad"], c["pad"], _blocks(c["blocks"]), c["bd"], 1, pa)
    st.obmc_predict_batch(rp, c["pad"], c["pad"], _blocks(other), c["bd"], 1, pb)
    ctx.synchronize()
    want_b = oc.predict_batch(c["refs"], c["pad"], other, c["bd"], c["w"], c["h"], 1, border=(c["pad"], c["pad"]), fill=FILL)
    dtype = c["refs"][0][0].dtype
    for p in range(3):
        m = _written(c["blocks"], c["w"], c["h"], p)
        np.testing.assert_array_equal(_host(a[p], dtype)[:, :m.shape[1]][m], c["pred"][p][m], err_msg="first call, plane %d" % p)
        np.testing.assert_array_equal(_host(b[p], dtype)[:, :m.shape[1]], want_b[p], err_msg="second call, plane %d" % p)
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_without_neighbours_it_is_the_sr_shims_block(ctx, bd):
    """n_above = n_left = 0: the plain single-reference predictor, equal to the convolve_*_sr shim of each block's form on the
    same window (luma, MVs inside the clamp)."""
    w, h, pad = 64, 64, 80
    rng = np.random.default_rng(5 + bd)
    refs = _noise_refs(rng, bd, w, h, pad, 1)
    blocks = [dict(x=x, y=y, w=bw, h=bh, ref=0, fx=k & 3, fy=(k >> 1) & 3, mv=mv, above=[], left=[])
              for k, (x, y, bw, bh, mv) in enumerate([(0, 0, 32, 32, (5, 11)), (32, 0, 32, 16, (-8, 3)), (32, 16, 16, 16, (7, 0)),
                                                      (48, 16, 8, 8, (0, 0)), (48, 24, 8, 8, (-3, -5)), (0, 32, 64, 32, (1, -9))])]
    st = svtgpu.TfState(ctx, w, h)
    got = _predict(st, refs, pad, blocks, bd, 0, (pad, pad))
    t, (r0, r1) = ic.tables(), ic.rounds(bd)
    src = np.ascontiguousarray(refs[0][0])
    for b in blocks:
        phx, phy = (2 * b["mv"][0]) & 15, (2 * b["mv"][1]) & 15
        form = ic.FORMS[(1 if phx else 0) | (2 if phy else 0)]
        dst = np.zeros((b["h"], b["w"]), src.dtype)
        svtgpu.convolve_sr(form, src, pad + b["x"] + ((2 * b["mv"][0]) >> 4), pad + b["y"] + ((2 * b["mv"][1]) >> 4), b["w"], b["h"],
                           t[ic.filter_table(b["fx"], b["w"])][phx], t[ic.filter_table(b["fy"], b["h"])][phy], r0, r1, bd, dst, 0, 0)
        np.testing.assert_array_equal(got[0][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]], dst, err_msg=str(b))
    st.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_refusals_leave_pred_untouched(ctx, bd):
    c, good = next((r, b) for r in RECORDS if r["bd"] == bd and r["chroma"] for b in r["blocks"]
                   if len(b["above"]) >= 2 and len(b["left"]) >= 1)
    w, h = c["w"], c["h"]
    st = svtgpu.TfState(ctx, w, h)
    rp, pp, dp, dr = _prepare(w, h, c["refs"], c["pad"])
    ra = (svtgpu.TfPlanes * 3)(*rp)
    L = svtgpu.lib()

    def rc(blocks=None, n_refs=3, nb=None, raw=None, bx=c["pad"]):
        bl = _blocks([good] if blocks is None else blocks)
        if raw:
            raw(bl[0])
        ba = (svtgpu.ObmcBlock * max(len(bl), 1))(*bl)
        return L.svtgpu_obmc_predict_batch(st.h, ra, n_refs, bx, c["pad"], ba, len(bl) if nb is None else nb, bd, 1, ctypes.byref(pp), None)

    def nbs(key, k, **kw):
        spans = [dict(s) for s in good[key]]
        spans[k].update(kw)
        return dict(good, **{key: spans})
    assert rc(nb=-1) == -1 and rc(bx=-1) == -1 and rc(n_refs=27) == -3
    assert rc([dict(good, x=good["x"] + 4)]) == -1 and rc([dict(good, y=good["y"] + 4)]) == -1       # a position not on 8
    assert rc([dict(good, x=w)]) == -1 and rc([dict(good, w=8, h=64)]) == -1                           # outside, a size outside the rule
    assert rc([dict(good, fx=4)]) == -1 and rc([dict(good, fy=4)]) == -1 and rc([dict(good, ref=3)]) == -1
    assert rc([nbs("above", 0, ref=3)]) == -1 and rc([nbs("left", 0, ref=2)], n_refs=2) == -1
    assert rc([nbs("above", 0, fx=4)]) == -1 and rc([nbs("left", 0, fy=4)]) == -1
    assert rc([nbs("above", 0, size=3)]) == -1 and rc([nbs("above", 0, size=1)]) == -1 and rc([nbs("above", 0, size=32)]) == -1
    assert rc([nbs("above", 1, rel=good["above"][1]["rel"] + 1)]) == -1                                 # rel odd
    assert rc([nbs("above", 1, rel=0)]) == -1                                                           # overlaps the first span
    assert rc([nbs("left", 0, rel=good["h"] // 4 - 2, size=4)]) == -1                                   # leaves the side
    assert rc([dict(good, w=8, h=8, above=good["above"][:2], left=[])]) == -1                            # more than max_neighbor_obmc
    assert rc([dict(good, y=0)]) == -1 and rc([dict(good, x=0)]) == -1                                   # a list where there is no neighbour
    assert rc(raw=lambda b: setattr(b, "reserved0", 1)) == -1
    assert rc(raw=lambda b: b.reserved.__setitem__(11, 1)) == -1
    assert rc(raw=lambda b: setattr(b, "n_above", 5)) == -1
    assert rc([good, dict(good, fx=9)]) == -1  # a good block behind a bad one: refused as a whole
    assert rc(nb=0) == 0
    ctx.synchronize()
    dtype = c["refs"][0][0].dtype
    assert all((_host(t, dtype) == FILL).all() for t in dp)
    assert rc(raw=lambda b: setattr(b, "wm_offset", -7)) == 0  # ignored here
    ctx.synchronize()
    st.close()


# ---------------------------------------------------------------------------------------------
# the six blend shims
# ---------------------------------------------------------------------------------------------
BLENDS = oc.blend_cases()
FORM = {0: None, 1: None, 2: "16bit", 3: "16bit", 4: "8bit", 5: "8bit"}


@pytest.mark.parametrize("c", BLENDS, ids=[c["name"] for c in BLENDS])
def test_blend_shims_match_records(c):
    """Each record through its shim with strides of their own and guards around dst; then again with src0 aliasing dst, and
    with src1 aliasing dst."""
    w, h, d = c["w"], c["h"], "h" if c["fn"] & 1 else "v"

    def framed(a, fill):
        big = np.full((h + 3, w + 5), fill, a.dtype)
        big[1:1 + h, 2:2 + w] = a
        return big
    a, b, dst = framed(c["src0"], 1), framed(c["src1"], 2), np.full((h + 2, w + 9), 9, c["src0"].dtype)
    svtgpu.blend_a64_mask(d, (dst, 4, 1), (a, 2, 1), (b, 2, 1), c["mask"], w, h, c["bd"], FORM[c["fn"]])
    np.testing.assert_array_equal(dst[1:1 + h, 4:4 + w], c["out"], err_msg=c["name"])
    guard = dst.copy()
    guard[1:1 + h, 4:4 + w] = 9
    assert (guard == 9).all(), c["name"]
    for alias in (0, 1):
        a, b = framed(c["src0"], 1), framed(c["src1"], 2)
        dst = a if alias == 0 else b
        svtgpu.blend_a64_mask(d, (dst, 2, 1), (a, 2, 1), (b, 2, 1), c["mask"], w, h, c["bd"], FORM[c["fn"]])
        np.testing.assert_array_equal(dst[1:1 + h, 2:2 + w], c["out"], err_msg="%s aliasing src%d" % (c["name"], alias))


# ---------------------------------------------------------------------------------------------
# wsrc / mask on the device and the chain into the search
# ---------------------------------------------------------------------------------------------
def _wm_blocks(blocks):
    """ObmcBlocks with compact wm_offsets; (list, total entries)."""
    out, off = [], 0
    for b in _blocks(blocks):
        b.wm_offset = off
        off += 2 << (b.w_log2 + b.h_log2)
        out.append(b)
    return out, off


WM_RECORDS = [c for c in RECORDS if c["wm"]]


@pytest.mark.parametrize("c", WM_RECORDS, ids=[c["name"] for c in WM_RECORDS])
def test_weighted_source_matches_records(ctx, c):
    w, h = c["w"], c["h"]
    st = svtgpu.TfState(ctx, w, h)
    rp, _, _, dr = _prepare(w, h, c["refs"], c["pad"])
    blocks = [c["blocks"][j] for j, _, _ in c["wm"]]
    ob, total = _wm_blocks(blocks)
    src = _dev(oc.source_luma(c["index"], w, h, c["content"]))
    wm = torch.full((total + 8,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st.obmc_weighted_src_batch(rp, c["pad"], c["pad"], src.data_ptr(), w, ob, wm.data_ptr(), total)
    ctx.synchronize()
    got = wm.cpu().numpy()
    assert (got[total:] == -77).all()
    for b, o, (_, ws, mk) in zip(blocks, ob, c["wm"]):
        n = b["w"] * b["h"]
        np.testing.assert_array_equal(got[o.wm_offset:o.wm_offset + n].reshape(b["h"], b["w"]), ws, err_msg=c["name"] + " wsrc")
        np.testing.assert_array_equal(got[o.wm_offset + n:o.wm_offset + 2 * n].reshape(b["h"], b["w"]), mk, err_msg=c["name"] + " mask")
    st.close()


def test_weighted_source_refusals(ctx):
    c = WM_RECORDS[0]
    w, h = c["w"], c["h"]
    st = svtgpu.TfState(ctx, w, h)
    rp, _, _, dr = _prepare(w, h, c["refs"], c["pad"])
    ra = (svtgpu.TfPlanes * 3)(*rp)
    src = _dev(oc.source_luma(c["index"], w, h, c["content"]))
    good = c["blocks"][c["wm"][0][0]]
    n2 = 2 * good["w"] * good["h"]
    wm = torch.full((n2 + 16,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = svtgpu.lib()

    def rc(off=0, count=n2 + 16, srcp=src.data_ptr(), stride=w, wmp=wm.data_ptr(), block=good, raw=None):
        b = _blocks([block])[0]
        b.wm_offset = off
        if raw:
            raw(b)
        return L.svtgpu_obmc_weighted_src_batch(st.h, ra, 3, c["pad"], c["pad"], srcp, stride, (svtgpu.ObmcBlock * 1)(b), 1, wmp, count, None)
    assert rc(off=-4) == -1 and rc(off=2) == -1 and rc(off=20) == -1 and rc(count=n2 - 1) == -1 and rc(count=-1) == -1
    assert rc(srcp=None) == -1 and rc(wmp=None) == -1 and rc(stride=w - 1) == -1 and rc(wmp=wm.data_ptr() + 4) == -1
    assert rc(block=dict(good, x=good["x"] + 4)) == -1 and rc(raw=lambda b: setattr(b, "reserved0", 1)) == -1
    if good["above"]:
        assert rc(block=dict(good, above=[dict(good["above"][0], ref=3)])) == -1
    ctx.synchronize()
    assert (wm.cpu().numpy() == -77).all()
    assert rc(off=16, block=dict(good, ref=200, fx=9, fy=9)) == 0  # the block's own reference and filters are not looked at
    ctx.synchronize()
    st.close()


def test_chain_weighted_source_then_search_equals_the_host_pool(ctx):
    """64 x 64, 8 bits: a dozen items of mixed sizes.  svtgpu_obmc_set_items_device_wm hands the pool out,
    svtgpu_obmc_weighted_src_batch fills it on the device, svtgpu_obmc_search reads it: exactly the results of
    svtgpu_obmc_set_items with the pool computed on the host (the restatement the records hold)."""
    w = h = 64
    pad = 80
    rng = np.random.default_rng(4242)
    pics = [np.clip(np.add.outer(np.arange(h) * 2, np.arange(w)) + rng.integers(0, 60, (h, w)) + 10 * r, 0, 255).astype(np.uint8)
            for r in range(2)]
    refs = [[np.pad(p, pad, mode="edge"), np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.uint8)] for p in pics]
    src = np.clip(pics[0].astype(int) + rng.integers(-12, 13, (h, w)), 0, 255).astype(np.uint8)
    shapes = [(8, 8, 8, 8), (16, 8, 8, 8), (24, 8, 8, 16), (32, 8, 32, 8), (8, 16, 16, 16), (8, 32, 16, 32), (24, 24, 8, 8),
              (32, 16, 32, 16), (32, 32, 32, 32), (24, 32, 8, 32), (8, 24, 16, 8), (16, 8, 8, 8)]
    blocks = []
    for k, (x, y, bw, bh) in enumerate(shapes):
        def spans(side, maxn):
            out, rel = [], 0
            for j in range(min(maxn, side // 8)):
                out.append(dict(rel=rel, size=2, ref=int(rng.integers(0, 2)), fx=int(rng.integers(0, 4)), fy=int(rng.integers(0, 4)),
                                mv=(int(rng.integers(-24, 25)), int(rng.integers(-24, 25)))))
                rel += 2 + (2 if j == 0 and side >= 32 else 0)
            return out
        blocks.append(dict(x=x, y=y, w=bw, h=bh, ref=0, fx=0, fy=0, mv=(0, 0), above=spans(bw, oc.MAX_NEIGHBOURS[bw]),
                           left=spans(bh, oc.MAX_NEIGHBOURS[bh])))
    ob, total = _wm_blocks(blocks)
    pool = np.zeros(total, np.int32)
    for b, o in zip(blocks, ob):
        ws, mk = oc.weighted_src(refs, pad, b, src, w, h, border=(pad, pad))
        n = b["w"] * b["h"]
        pool[o.wm_offset:o.wm_offset + n], pool[o.wm_offset + n:o.wm_offset + 2 * n] = ws.ravel(), mk.ravel()
    items = [dict(ref=k & 1, x=b["x"], y=b["y"], w=b["w"], h=b["h"], mvp_col=int(rng.integers(-3, 4)), mvp_row=int(rng.integers(-3, 4)),
                  ref_mv_col=0, ref_mv_row=0, col_min=-16, col_max=16, row_min=-16, row_max=16, sad_per_bit=0, search_range=8,
                  search_diag=1, cost_mode=0, wm_offset=o.wm_offset, cost_offset=0) for k, (b, o) in enumerate(zip(blocks, ob))]
    frames = []
    for p in pics:
        f = svtgpu.Frame(ctx, w, h, 8)
        f.upload([p, np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)])
        frames.append(f)
    host = svtgpu.ObmcBatch(ctx, w, h, 2, len(items))
    host.set_items(items, pool)
    host.search(frames)
    want = host.read()
    dev = svtgpu.ObmcBatch(ctx, w, h, 2, len(items))
    wm_dev = dev.set_items_device_wm(items, total)
    st = svtgpu.TfState(ctx, w, h)
    dr = [_dev(r[0]) for r in refs]
    rp = [svtgpu.TfPlanes.make([t.data_ptr() + pad * (r[0].shape[1] + 1), 0, 0], [r[0].shape[1], 0, 0]) for t, r in zip(dr, refs)]
    ds = _dev(src)
    st.obmc_weighted_src_batch(rp, pad, pad, ds.data_ptr(), w, ob, wm_dev, total)
    dev.search(frames)
    got = dev.read()
    assert got.tolist() == want.tolist()
    assert len({(int(r["mv_col"]), int(r["mv_row"])) for r in want}) > 1  # the searches moved
    host.close(), dev.close(), st.close()
