"""AV1 inter-intra prediction on the MI355X: svtgpu_interintra_predict_batch and svtgpu_interintra_mode_sse_batch against
every record of the reference's fixture (tests/golden/interintra.bin), and -- on lists the fixture does not hold -- against
the numpy restatement that tests/test_interintra.py holds to those records; the blend and intra shims against the records
and the restatement; the refusals; two streams.  Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import interintra_cases as ic
import svtgpu
from test_obmc_pred_gpu import _cut, _dev, _host, _noise_refs, _prepare, _written

pytestmark = pytest.mark.gpu

RECORDS = ic.records()
FILL = 5


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def _blocks(blocks):
    return [svtgpu.InterIntraBlock.make(b["x"], b["y"], b["w"], b["h"], b["ref"], b["mv"], b["fx"], b["fy"], b["mode"], b["use_wedge"],
                                        b["wedge_index"], b["n_top"], b["n_left"], b["edge_offset"]) for b in blocks]


def _predict(st, refs, pad, blocks, edges, bd, chroma, border, stream=None):
    rp, pp, dp, dr = _prepare(st.width, st.height, refs, pad)
    st.interintra_predict_batch(rp, border[0], border[1], _blocks(blocks), edges, bd, chroma, pp, stream)
    st.ctx.synchronize(stream)
    return [_host(t, refs[0][0].dtype)[:, :st.width >> (p > 0)] for p, t in enumerate(dp)]


def _mode_sse(st, refs, pad, blocks, edges, bd, src, border, stream=None):
    rp, _, _, dr = _prepare(st.width, st.height, refs, pad)
    ds = _dev(src)
    out = torch.full((max(len(blocks), 1), 4), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st.interintra_mode_sse_batch(rp, border[0], border[1], _blocks(blocks), edges, bd, ds.data_ptr(), src.shape[1], out.data_ptr(), stream)
    st.ctx.synchronize(stream)
    return out.cpu().numpy()[:len(blocks)]


@pytest.mark.parametrize("c", RECORDS, ids=[c["name"] for c in RECORDS])
def test_predict_batch_matches_records(ctx, c):
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _predict(st, c["refs"], c["pad"], c["blocks"], c["edges"], c["bd"], c["chroma"], (c["pad"], c["pad"]))
    for p, want in enumerate(c["pred"]):
        m = _written(c["blocks"], c["w"], c["h"], p)
        np.testing.assert_array_equal(got[p][m], want[m], err_msg="%s plane %d" % (c["name"], p))
        assert (got[p][~m] == FILL).all(), c["name"]  # nothing outside the listed blocks
    if not c["chroma"]:
        assert (got[1] == FILL).all() and (got[2] == FILL).all(), c["name"]
    st.close()


@pytest.mark.parametrize("c", RECORDS, ids=[c["name"] for c in RECORDS])
def test_mode_sse_batch_matches_records(ctx, c):
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _mode_sse(st, c["refs"], c["pad"], c["blocks"], c["edges"], c["bd"], c["src"], (c["pad"], c["pad"]))
    np.testing.assert_array_equal(got, c["sse"], err_msg=c["name"])
    st.close()


def _draw_blocks(rng, cells, bd, chroma, far=()):
    """Blocks over `cells` (x, y, w, h) with drawn fields and an edge pool of noise; far: indices whose MV leaves the border."""
    blocks, n = [], 0
    for k, (x, y, w, h) in enumerate(cells):
        mv = (int(rng.integers(-40, 41)), int(rng.integers(-40, 41)))
        if k in far:
            mv = (int(rng.choice([-1, 1])) * int(rng.integers(1500, 2500)), int(rng.choice([-1, 1])) * int(rng.integers(1500, 2500)) + 1)
        nt, nl = int(rng.choice([0, w // 2, w])), int(rng.choice([0, h // 4, h]))
        blocks.append(dict(x=x, y=y, w=w, h=h, ref=int(rng.integers(0, 3)), fx=int(rng.integers(0, 4)), fy=int(rng.integers(0, 4)), mv=mv,
                           mode=int(rng.integers(0, 4)), use_wedge=int(rng.integers(0, 2)), wedge_index=int(rng.integers(0, 16)),
                           n_top=(nt, nt // 2), n_left=(nl, nl // 2), edge_offset=n))
        n += (w + h) * (2 if chroma else 1)
    edges = rng.integers(0, 1 << bd, n).astype(np.uint16 if bd > 8 else np.uint8)
    return blocks, edges


# all seven sizes in one 64 x 64 picture (gathered items hold slots of different blocks, modes and wedge flags), an 8x8 beside
# a 32x32, a block at each picture corner
CELLS64 = [(0, 0, 8, 8), (8, 0, 32, 32), (40, 0, 16, 8), (56, 0, 8, 16), (40, 8, 16, 16), (56, 16, 8, 8), (0, 8, 8, 16), (0, 24, 8, 8),
           (40, 24, 16, 8), (56, 24, 8, 8), (0, 32, 16, 32), (16, 32, 32, 16), (16, 48, 16, 16), (32, 48, 16, 8), (32, 56, 8, 8),
           (40, 56, 8, 8), (48, 32, 16, 16), (48, 48, 16, 16)]


@pytest.mark.parametrize("bd,chroma", [(8, 1), (10, 1), (10, 0)])
def test_mixed_list_on_a_64x64_picture_with_the_read_clamp_acting(ctx, bd, chroma):
    """64 x 64 of noise allocated with 160 samples around it, 24 declared readable; the four corner blocks' MVs far outside, so
    the read clamp acts: the device gives what the restatement gives from planes whose samples beyond the declared border are
    overwritten; without the clamp the result differs (asserted on the restatement)."""
    w = h = 64
    pad, border = 160, 24
    rng = np.random.default_rng(4949 + bd + chroma)
    assert {(c[2], c[3]) for c in CELLS64} == set(ic.SIZES)
    corners = [k for k, c in enumerate(CELLS64) if (c[0] in (0, w - c[2])) and (c[1] in (0, h - c[3]))]
    assert len(corners) == 4
    refs = _noise_refs(rng, bd, w, h, pad)
    blocks, edges = _draw_blocks(rng, CELLS64, bd, chroma, far=corners)
    want = ic.predict_batch(_cut(refs, pad, border), pad, blocks, edges, bd, w, h, chroma, border=(border, border), fill=FILL)
    free = ic.predict_batch(refs, pad, blocks, edges, bd, w, h, chroma, border=(pad, pad), fill=FILL)
    assert (want[0] != free[0]).any(), "the read clamp changes nothing"
    st = svtgpu.TfState(ctx, w, h)
    got = _predict(st, refs, pad, blocks, edges, bd, chroma, (border, border))
    for p in range(3):
        np.testing.assert_array_equal(got[p], want[p], err_msg="plane %d" % p)
    src = rng.integers(0, 1 << bd, (h, w)).astype(refs[0][0].dtype)
    sse = _mode_sse(st, refs, pad, blocks, edges, bd, src, (border, border))
    np.testing.assert_array_equal(sse, ic.mode_sse(_cut(refs, pad, border), pad, blocks, edges, bd, w, h, src, border=(border, border)))
    st.close()


def test_two_calls_on_two_streams_equal_the_single_stream_results(ctx):
    a, b = RECORDS[0], RECORDS[1]
    one = [_predict(svtgpu.TfState(ctx, c["w"], c["h"]), c["refs"], c["pad"], c["blocks"], c["edges"], c["bd"], c["chroma"],
                    (c["pad"], c["pad"])) for c in (a, b)]
    streams = [ctx.stream_create(), ctx.stream_create()]
    states = [svtgpu.TfState(ctx, c["w"], c["h"]) for c in (a, b)]
    prep = [_prepare(c["w"], c["h"], c["refs"], c["pad"]) for c in (a, b)]
    for c, st, s, (rp, pp, dp, dr) in zip((a, b), states, streams, prep):
        st.interintra_predict_batch(rp, c["pad"], c["pad"], _blocks(c["blocks"]), c["edges"], c["bd"], c["chroma"], pp, s)
    for s in streams:
        ctx.synchronize(s)
    for c, want, (rp, pp, dp, dr) in zip((a, b), one, prep):
        for p in range(3):
            np.testing.assert_array_equal(_host(dp[p], c["refs"][0][0].dtype)[:, :c["w"] >> (p > 0)], want[p], err_msg="%s plane %d" % (c["name"], p))
    for st in states:
        st.close()
    for s in streams:
        ctx.stream_destroy(s)


def test_blend_shims_match_records_and_the_restatement_with_aliasing():
    for c in ic.blend_cases():
        for alias in (None, 0, 1):
            s0, s1 = c["src0"].copy(), c["src1"].copy()
            dst = np.zeros_like(s0) if alias is None else (s0, s1)[alias]
            svtgpu.blend_a64_mask2d((dst, 0, 0), (s0, 0, 0), (s1, 0, 0), c["mask"], c["w"], c["h"], c["subw"], c["subh"], c["bd"] if c["hbd"] else None)
            np.testing.assert_array_equal(dst, c["out"], err_msg="%s alias %r" % (c["name"], alias))
    # a pruned grid of all sizes 1 .. 128, strided operands inside larger arrays
    rng = np.random.default_rng(11)
    sizes = [1, 2, 4, 8, 16, 32, 64, 128]
    for k, (w, h) in enumerate((w, h) for w in sizes for h in sizes):
        if (k * 7) % 5 > 1 and w * h not in (1, 128 * 128):
            continue
        hbd, subw, subh = k & 1, (k >> 1) & 1, (k >> 2) & 1
        bd = (10, 12)[(k >> 3) & 1] if hbd else 8
        dt = np.uint16 if hbd else np.uint8
        big = [rng.integers(0, 1 << bd, (h + 3, w + 5)).astype(dt) for _ in range(3)]
        mask = rng.integers(0, 65, ((h << subh) + 1, (w << subw) + 3)).astype(np.uint8)
        want = ic.blend_a64_mask(big[1][1:1 + h, 2:2 + w], big[2][2:2 + h, 3:3 + w], mask[:h << subh, :w << subw], subw, subh)
        keep = big[0].copy()
        svtgpu.blend_a64_mask2d((big[0], 1, 0), (big[1], 2, 1), (big[2], 3, 2), mask, w, h, subw, subh, bd if hbd else None)
        np.testing.assert_array_equal(big[0][0:h, 1:1 + w], want, err_msg="%dx%d sub %d %d" % (w, h, subw, subh))
        keep[0:h, 1:1 + w] = want
        np.testing.assert_array_equal(big[0], keep)  # nothing outside the block


def test_intra_shims_match_records():
    for c in ic.intra_cases():
        got = svtgpu.intra_predictor(ic.KINDS[c["kind"]], c["above"], c["left"], c["bd"] if c["hbd"] else None)
        np.testing.assert_array_equal(got, c["out"], err_msg=c["name"])
    a, l = np.full(16, 4095, np.uint16), np.full(8, 4095, np.uint16)  # 12 bits
    for kind in ic.KINDS:
        want = ic.intra_by_kind(ic.KINDS.index(kind), a.astype(np.int64), l.astype(np.int64), 12)
        np.testing.assert_array_equal(svtgpu.intra_predictor(kind, a, l, 12), want, err_msg=kind)


def test_refusals_leave_pred_untouched(ctx):
    """Every refusal of both entries, each a one-field change of a call that succeeds; pred keeps its prefill throughout."""
    c = RECORDS[0]
    w, h, bd, pad = c["w"], c["h"], c["bd"], c["pad"]
    st = svtgpu.TfState(ctx, w, h)
    rp, pp, dp, dr = _prepare(w, h, c["refs"], pad)
    L, good = svtgpu.lib(), c["blocks"][:3]
    edges = c["edges"]
    ds, out = _dev(c["src"]), torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ra = (svtgpu.TfPlanes * 3)(*rp)

    def call(blocks=good, n_refs=3, bx=pad, by=pad, e=edges, n_edges=None, depth=bd, pred=pp, refs=ra, n_blocks=None, state=st.h):
        ba = (svtgpu.InterIntraBlock * len(blocks))(*_blocks(blocks))
        nb, ne = len(blocks) if n_blocks is None else n_blocks, (0 if e is None else e.size) if n_edges is None else n_edges
        ep = None if e is None else e.ctypes.data
        pr = None if pred is None else ctypes.byref(pred)
        return (L.svtgpu_interintra_predict_batch(state, refs, n_refs, bx, by, ba, nb, ep, ne, depth, 1, pr, None),
                L.svtgpu_interintra_mode_sse_batch(state, refs, n_refs, bx, by, ba, nb, ep, ne, depth, ds.data_ptr(), w, out.data_ptr(), None))

    def bad(i, **kw):
        return [dict(b, **kw) if k == i else b for k, b in enumerate(good)]

    b0 = good[0]
    both = [dict(n_refs=27), dict(state=None), dict(refs=None), dict(n_refs=-1), dict(n_blocks=-1), dict(n_edges=-1), dict(depth=12),
            dict(bx=-1), dict(by=-1), dict(e=None), dict(n_edges=b0["edge_offset"] + (b0["w"] + b0["h"]) - 1, blocks=good[:1], n_blocks=1),
            dict(blocks=bad(1, x=w)), dict(blocks=bad(1, x=good[1]["x"] + 4)), dict(blocks=bad(1, y=-8)), dict(blocks=bad(2, w=8, h=32)),
            dict(blocks=bad(2, w=64, h=64)), dict(blocks=bad(0, ref=3)), dict(blocks=bad(0, fx=4)), dict(blocks=bad(0, fy=4)),
            dict(blocks=bad(1, n_top=(good[1]["w"] + 1, 0))), dict(blocks=bad(1, n_left=(good[1]["h"] + 1, 0))), dict(blocks=bad(2, edge_offset=-1)),
            dict(blocks=bad(2, edge_offset=edges.size - 8))]
    for kw in both:
        rc = call(**kw)
        assert rc == ((-3, -3) if kw.get("n_refs") == 27 else (-1, -1)), (kw, rc)
    # the predict entry alone: mode, wedge fields, chroma counts, pred
    for kw in (dict(blocks=bad(0, mode=4)), dict(blocks=bad(0, use_wedge=2)), dict(blocks=bad(0, wedge_index=16)),
               dict(blocks=bad(1, n_top=(0, good[1]["w"] // 2 + 1))), dict(blocks=bad(1, n_left=(0, good[1]["h"] // 2 + 1)))):
        rc = call(**kw)
        assert rc == (-1, 0), (kw, rc)
    assert call(pred=None)[0] == -1
    narrow = svtgpu.TfPlanes.make([t.data_ptr() for t in dp], [w - 16, w // 2, w // 2])
    assert call(pred=narrow)[0] == -1
    # a reserved byte, through the raw struct
    ba = (svtgpu.InterIntraBlock * 1)(*_blocks(good[:1]))
    ba[0].reserved[7] = 1
    assert L.svtgpu_interintra_predict_batch(st.h, ra, 3, pad, pad, ba, 1, edges.ctypes.data, edges.size, bd, 1, ctypes.byref(pp), None) == -1
    # the distortion entry alone: src, stride, sse
    ba[0].reserved[7] = 0
    args = (st.h, ra, 3, pad, pad, ba, 1, edges.ctypes.data, edges.size, bd)
    assert L.svtgpu_interintra_mode_sse_batch(*args, None, w, out.data_ptr(), None) == -1
    assert L.svtgpu_interintra_mode_sse_batch(*args, ds.data_ptr(), w - 1, out.data_ptr(), None) == -1
    assert L.svtgpu_interintra_mode_sse_batch(*args, ds.data_ptr(), w, None, None) == -1
    assert L.svtgpu_interintra_mode_sse_batch(*args, ds.data_ptr(), w, out.data_ptr() + 4, None) == -1
    ctx.synchronize()
    for p, t in enumerate(dp):
        assert (_host(t, c["refs"][0][0].dtype) == FILL).all(), "a refused call wrote plane %d" % p
    # the controls: the unchanged call succeeds, and an empty list is accepted without edges
    assert call() == (0, 0) and call(blocks=good[:1], n_blocks=0, e=None) == (0, 0)
    ctx.synchronize()
    st.close()
