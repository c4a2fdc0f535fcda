"""AV1 single-reference interpolation and the temporal filter's motion compensation: reader of tests/golden/interp.bin
(written by tests/golden/gen_golden_interp.c from the reference's own C) and a numpy restatement of the four convolve forms
(EbInterPrediction.c:320-427, :679-786), the filter choice (EbInterPrediction.h:139-155), the MV clamp
(EbEncInterPrediction.c:28-48, :3166-3177) and the frame walk of tf_64x64_inter_prediction / tf_32x32_inter_prediction
(EbTemporalFiltering.c:2230-2580).  Shared by tests/test_interp.py (CPU) and tests/test_interp_gpu.py."""
import functools
import os

import numpy as np

import golden_io
from tf_cases import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interp.bin")
REGULAR, SMOOTH, SHARP, BILINEAR, REGULAR4, SMOOTH4 = range(6)
FORMS = ("2d_copy_sr", "x_sr", "y_sr", "2d_sr")  # by (phase_x != 0) | (phase_y != 0) << 1
PAD = 80


@functools.lru_cache(maxsize=1)
def fixture():
    return golden_io.load(GOLDEN)


def tables():
    return fixture()["tables"]


def rounds(bd):
    """get_conv_params_no_round (convolve.h:40-64), not compound: (round_0, round_1)."""
    extra = max(bd + 7 - 3 + 2 - 16, 0)
    return 3 + extra, 11 - extra


def filter_table(kind, size):
    """av1_get_interp_filter_params_with_block_size: kind 0 regular, 1 smooth, 2 sharp, 3 bilinear; size = w for the
    horizontal filter, h for the vertical."""
    if size <= 4 and kind in (REGULAR, SHARP):
        return REGULAR4
    if size <= 4 and kind == SMOOTH:
        return SMOOTH4
    return kind


def _rnd(v, n):  # ROUND_POWER_OF_TWO on signed values: an arithmetic shift
    return (v + ((1 << n) >> 1)) >> n


def convolve(win, w, h, fx, fy, form, bd, clip=True):
    """One block.  `win` is the (h + 7) x (w + 7) window with the block at (3, 3); fx / fy the 8-tap rows; form 0 copy, 1 x,
    2 y, 3 2d.  clip=False (tests only) leaves out the final clip to the sample range."""
    win = np.asarray(win, dtype=np.int64)
    fx, fy = np.asarray(fx, dtype=np.int64), np.asarray(fy, dtype=np.int64)
    r0, r1 = rounds(bd)
    maxv = (1 << bd) - 1
    lo, maxv = (0, maxv) if clip else (-(1 << 62), 1 << 62)
    if form == 0:
        return win[3:3 + h, 3:3 + w].copy()
    if form == 1:
        s = sum(fx[k] * win[3:3 + h, k:k + w] for k in range(8))
        return np.clip(_rnd(_rnd(s, r0), 7 - r0), lo, maxv)
    if form == 2:
        s = sum(fy[k] * win[k:k + h, 3:3 + w] for k in range(8))
        return np.clip(_rnd(s, 7), lo, maxv)
    im = (1 << (bd + 6)) + sum(fx[k] * win[:, k:k + w] for k in range(8))
    im = _rnd(im, r0).astype(np.int16).astype(np.int64)
    ob = bd + 14 - r0
    s = (1 << ob) + sum(fy[k] * im[k:k + h] for k in range(8))
    res = _rnd(s, r1) - ((1 << (ob - r1)) + (1 << (ob - r1 - 1)))
    if bd == 8:
        res = res.astype(np.int16).astype(np.int64)
    return np.clip(_rnd(res, 14 - r0 - r1), lo, maxv)


def block_source(bd, w, h, content, index):
    """The drawn (h + 8) x (w + 8) source buffer of block record `index`; the block is at (3, 3)."""
    maxv = (1 << bd) - 1
    bw, bh = w + 8, h + 8
    if content == 0:
        a = draw(0x4950000000000000 + 16 * index, bw * bh, maxv + 1).reshape(bh, bw)
    elif content in (1, 2):
        a = np.full((bh, bw), 0 if content == 1 else maxv, dtype=np.int64)
    else:
        y, x = np.mgrid[0:bh, 0:bw]
        a = np.where((x + y) & 1, maxv, 0).astype(np.int64)
    return a.astype(np.uint16 if bd > 8 else np.uint8)


@functools.lru_cache(maxsize=1)
def block_cases():
    g = fixture()
    out = []
    for i in range(int(g["nblock"][0])):
        bd, w, h, phx, phy, kind, content, form, idx = (int(v) for v in g["b%d_par" % i])
        out.append(dict(name="b%d" % i, bd=bd, w=w, h=h, phx=phx, phy=phy, kind=kind, content=content, form=form, index=idx,
                        out=g["b%d_out" % i], mm=tuple(int(v) for v in g["b%d_mm" % i])))
    return out


def block_filters(c):
    t = tables()
    return t[filter_table(c["kind"], c["w"])][c["phx"]], t[filter_table(c["kind"], c["h"])][c["phy"]]


def block_expected(c):
    src = block_source(c["bd"], c["w"], c["h"], c["content"], c["index"])
    fx, fy = block_filters(c)
    return convolve(src[:c["h"] + 7, :c["w"] + 7], c["w"], c["h"], fx, fy, c["form"], c["bd"])


# ---------------------------------------------------------------------------------------------
# the motion compensation
# ---------------------------------------------------------------------------------------------
def _i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def clamp_mv(mv, org, b, dim, ss):
    """One component: MV in 1/8 luma sample of a block of luma size b at luma origin org in a picture of luma size dim ->
    (integer source position in the plane, phase)."""
    sc = 1 - ss
    q = _i16(mv * (1 << sc))
    spel = (4 + (b >> ss)) << 4
    lo = -(org * 8) * (1 << sc) - spel
    hi = ((dim - b - org) * 8) * (1 << sc) + spel - 16
    q = _i16(min(max(q, lo), hi))
    return (org >> ss) + (q >> 4), q & 15


def padded_reference(bd, w, h, seed, pad=PAD):
    """The three planes of a drawn reference picture with edge-replicated borders of `pad` luma samples."""
    sc, maxv, planes = 1 << (bd - 8), (1 << bd) - 1, []
    for p in range(3):
        pw, ph = w >> (p > 0), h >> (p > 0)
        y, x = np.mgrid[0:ph, 0:pw]
        a = np.clip((2 * x + y) * sc // 4 + draw(seed + p, pw * ph, 64 * sc).reshape(ph, pw), 0, maxv)
        planes.append(np.pad(a, pad >> (p > 0), mode="edge").astype(np.uint16 if bd > 8 else np.uint8))
    return planes


def blocks_of(m):
    """The prediction blocks of one 64x64 block's motion record: (x, y, size, mvx, mvy) relative to the block."""
    if m["use64"]:
        return [(0, 0, 64, int(m["mv64"][0]), int(m["mv64"][1]))]
    out = []
    for i in range(4):
        x32, y32 = (i & 1) * 32, (i >> 1) * 32
        if not m["split32"][i]:
            out.append((x32, y32, 32, int(m["mv32"][i][0]), int(m["mv32"][i][1])))
            continue
        for j in range(4):
            x16, y16, q = x32 + (j & 1) * 16, y32 + (j >> 1) * 16, 4 * i + j
            if not m["split16"][q]:
                out.append((x16, y16, 16, int(m["mv16"][q][0]), int(m["mv16"][q][1])))
                continue
            for k in range(4):
                out.append((x16 + (k & 1) * 8, y16 + (k >> 1) * 8, 8, int(m["mv8"][4 * q + k][0]), int(m["mv8"][4 * q + k][1])))
    return out


def predict_frame(ref, pad, motion, bd, w, h, tf_chroma, border=None, out=None):
    """The predictor picture of one reference: ref = three padded planes (pad luma samples), motion = nblk records in raster
    order.  border = (bx, by) clamps every read coordinate into [-border, size + border - 1] as the library does; None:
    unclamped (the reference's own reads).  Returns three planes over the 64-aligned area (chroma zeros without tf_chroma)."""
    t = tables()
    bc, br = (w + 63) // 64, (h + 63) // 64
    if out is None:
        out = [np.zeros((br * 64 >> (p > 0), bc * 64 >> (p > 0)), dtype=ref[0].dtype) for p in range(3)]
    for blk, m in enumerate(motion):
        bx, by = (blk % bc) * 64, (blk // bc) * 64
        for x0, y0, b, mvx, mvy in blocks_of(m):
            for p in range(3 if tf_chroma else 1):
                ss = int(p > 0)
                bp, pd, pw, ph = b >> ss, pad >> ss, w >> ss, h >> ss
                sx, phx = clamp_mv(mvx, bx + x0, b, w, ss)
                sy, phy = clamp_mv(mvy, by + y0, b, h, ss)
                xs, ys = np.arange(sx - 3, sx + bp + 4), np.arange(sy - 3, sy + bp + 4)
                if border is not None:
                    xs = np.clip(xs, -(border[0] >> ss), pw + (border[0] >> ss) - 1)
                    ys = np.clip(ys, -(border[1] >> ss), ph + (border[1] >> ss) - 1)
                assert xs.min() >= -pd and ys.min() >= -pd and xs.max() < pw + pd and ys.max() < ph + pd
                win = ref[p][np.ix_(ys + pd, xs + pd)]
                tab = filter_table(SHARP, bp)
                form = (1 if phx else 0) | (2 if phy else 0)
                res = convolve(win, bp, bp, t[tab][phx], t[tab][phy], form, bd)
                oy, ox = (by + y0) >> ss, (bx + x0) >> ss
                out[p][oy:oy + bp, ox:ox + bp] = res
    return out


def _motion_records(g, i, nr, nblk):
    return [[dict(use64=int(g["p%d_use64" % i][r][b]), mv64=g["p%d_mv64" % i][r][b], split32=g["p%d_split32" % i][r][b],
                  split16=g["p%d_split16" % i][r][b], mv32=g["p%d_mv32" % i][r][b], mv16=g["p%d_mv16" % i][r][b],
                  mv8=g["p%d_mv8" % i][r][b]) for b in range(nblk)] for r in range(nr)]


@functools.lru_cache(maxsize=1)
def pred_cases():
    g = fixture()
    out = []
    for i in range(int(g["npred"][0])):
        bd, w, h, nr, chroma, pad, idx = (int(v) for v in g["p%d_par" % i])
        nblk = ((w + 63) // 64) * ((h + 63) // 64)
        refs = [padded_reference(bd, w, h, 0x4950000000100000 + 256 * idx + 4 * r, pad) for r in range(nr)]
        pred = [[g["p%d_pred%d_%d" % (i, r, p)] for p in range(3 if chroma else 1)] for r in range(nr)]
        out.append(dict(name="p%d" % i, bd=bd, w=w, h=h, n_refs=nr, tf_chroma=chroma, pad=pad, nblk=nblk, refs=refs,
                        motion=_motion_records(g, i, nr, nblk), pred=pred, kinds=[int(v) for v in g["p%d_kinds" % i]]))
    return out


@functools.lru_cache(maxsize=1)
def chain_cases():
    g = fixture()
    out = []
    for i in range(int(g["nchain"][0])):
        rec, mv_dist_th, chroma, idx = (int(v) for v in g["c%d_par" % i])
        c = pred_cases()[rec]
        sc, maxv, centre = 1 << (c["bd"] - 8), (1 << c["bd"]) - 1, []
        for p in range(3):
            pw, ph = ((c["w"] + 63) & ~63) >> (p > 0), ((c["h"] + 63) & ~63) >> (p > 0)
            y, x = np.mgrid[0:ph, 0:pw]
            a = np.clip((2 * x + y) * sc // 4 + draw(0x4950000000200000 + 16 * idx + p, pw * ph, 64 * sc).reshape(ph, pw), 0, maxv)
            centre.append(a.astype(np.uint16 if c["bd"] > 8 else np.uint8))
        out.append(dict(name="c%d" % i, pred=c, mv_dist_th=mv_dist_th, tf_chroma=chroma, decay=[int(v) for v in g["c%d_decay" % i]],
                        err32=g["c%d_err32" % i], err16=g["c%d_err16" % i], centre=centre,
                        out=[g["c%d_out%d" % (i, p)] for p in range(3)]))
    return out


def border_case(c, border=68):
    """A frame on which the read clamp must act, from prediction record c: reference planes of noise over the whole
    allocation (picture and all `pad` samples around it, so a sample beyond the border differs from the one the clamp
    substitutes), and c's motion with four whole 64x64 blocks moved out of the picture: one far outside (the MV clamp makes
    its phase zero, so luma reaches b + 4 = 68 samples out and only chroma, at 36 + 3 > 34, meets the read clamp), and three
    whose MV is one eighth inside the MV clamp's bound (up-left, up-right, down-right: luma at 68 samples out with a
    non-zero phase, whose taps reach 71).
    Returns (refs, motion, want, free): want the restatement with the clamp at `border`, computed from planes whose samples
    beyond the border are overwritten (it cannot have read them); free the restatement without a clamp."""
    rng = np.random.default_rng(68 + c["bd"])
    dt = c["refs"][0][0].dtype
    refs = [[rng.integers(0, 1 << c["bd"], a.shape).astype(dt) for a in r] for r in c["refs"]]
    motion = [[dict(m) for m in row] for row in c["motion"]]
    bc = (c["w"] + 63) // 64
    x_hi = ((c["w"] - 64 - (bc - 1) * 64) * 16 + (68 << 4) - 16) // 2 - 1   # one eighth below the right bound, last column
    y_hi = ((c["h"] - 64 - (c["nblk"] // bc - 1) * 64) * 16 + (68 << 4) - 16) // 2 - 1
    lo = -(68 << 4) // 2 + 1                                                # one eighth above the left / top bound at 0
    for r, blk, mv in ((1, 0, (-2000, -1500)), (0, 0, (lo, lo)), (0, bc - 1, (x_hi, lo)), (1, c["nblk"] - 1, (x_hi, y_hi))):
        motion[r][blk] = dict(motion[r][blk], use64=1, mv64=np.array(mv, dtype=np.int16))
    want, free = [], []
    for r in range(c["n_refs"]):
        cut = []
        for p, a in enumerate(refs[r]):
            k = (c["pad"] - border) >> (p > 0)
            b = np.full(a.shape, 1, a.dtype)
            b[k:a.shape[0] - k, k:a.shape[1] - k] = a[k:a.shape[0] - k, k:a.shape[1] - k]
            cut.append(b)
        want.append(predict_frame(cut, c["pad"], motion[r], c["bd"], c["w"], c["h"], 1, border=(border, border)))
        free.append(predict_frame(refs[r], c["pad"], motion[r], c["bd"], c["w"], c["h"], 1))
    return refs, motion, want, free


def random_motion(rng, nblk, w):
    """nblk motion records of random partitions and MVs (small, large and far outside the picture)."""
    def mv(n):
        kind = rng.integers(0, 6, size=(n, 2))
        small, big = rng.integers(-64, 65, size=(n, 2)), rng.integers(-(w * 8 + 1200), w * 8 + 1201, size=(n, 2))
        return np.where(kind == 0, 0, np.where(kind == 5, big, small)).astype(np.int16)
    return [dict(use64=int(rng.integers(0, 4) == 0), mv64=mv(1)[0], split32=rng.integers(0, 2, 4), split16=rng.integers(0, 2, 16),
                 mv32=mv(4), mv16=mv(16), mv8=mv(64)) for _ in range(nblk)]
