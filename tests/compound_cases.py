"""AV1 compound (two-reference) prediction: reader of tests/golden/compound.bin (written by
tests/golden/gen_golden_compound.c from the reference's own C) and a numpy restatement, written from the C, of the eight
jnt_convolve functions (EbInterPrediction.c:503-677, :861-1040), the weight selection of
svt_av1_dist_wtd_comp_weight_assign (:276-318) and svt_aom_inter_prediction's compound path
(EbEncInterPrediction.c:4070; MV clamp :28-48, :3166-3177).  Shared by tests/test_compound.py (CPU) and
tests/test_compound_gpu.py."""
import functools
import os

import numpy as np

import golden_io
from interp_cases import REGULAR, SMOOTH, SHARP, BILINEAR, _i16, _rnd, filter_table, tables  # noqa: F401
from tf_cases import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compound.bin")
FORMS = ("2d_copy", "x", "y", "2d")  # by (phase_x != 0) | (phase_y != 0) << 1
SIZES = [(8, 8), (8, 16), (16, 8), (8, 32), (32, 8), (16, 16), (16, 32), (32, 16), (16, 64), (64, 16), (32, 32), (32, 64),
         (64, 32), (64, 64), (64, 128), (128, 64), (128, 128)]
CHROMA_ONLY_SIZES = [(4, 4), (4, 8), (8, 4), (4, 16), (16, 4)]
MODES = [(0, 0, 0), (1, 9, 7), (1, 11, 5), (1, 12, 4), (1, 13, 3), (1, 7, 9), (1, 5, 11), (1, 4, 12), (1, 3, 13)]
QUANT_DIST_WEIGHT = ((2, 3), (2, 5), (2, 7), (1, 31))
QUANT_DIST_LOOKUP = (((9, 7), (11, 5), (12, 4), (13, 3)), ((7, 9), (5, 11), (4, 12), (3, 13)))


@functools.lru_cache(maxsize=1)
def fixture():
    return golden_io.load(GOLDEN)


def rounds(bd):
    """get_conv_params_no_round (convolve.h:40-64) with is_compound = 1: (round_0, round_1)."""
    return 3 + max(bd + 7 - 3 + 2 - 16, 0), 7


def dist_wtd_weights(d0, d1, order_idx):
    """The table walk of svt_av1_dist_wtd_comp_weight_assign on the two frame distances."""
    d0, d1 = min(d0, 31), min(d1, 31)
    order = int(d0 <= d1)
    i = 3
    if d0 and d1:
        for i in range(3):
            a, b = d0 * QUANT_DIST_WEIGHT[i][order], d1 * QUANT_DIST_WEIGHT[i][1 - order]
            if (d0 > d1 and a < b) or (d0 <= d1 and a > b):
                break
        else:
            i = 3
    return QUANT_DIST_LOOKUP[order_idx][i][order], QUANT_DIST_LOOKUP[order_idx][i][1 - order]


def first_pass(win, w, h, fx, fy, form, bd, r0=None, r1=None):
    """The CONV_BUF_TYPE-range value of one block before it is stored or combined (int64: the x and y forms hold it in an
    int32, the copy and 2-D forms in a uint16).  `win` is the (h + 7) x (w + 7) window with the block at (3, 3)."""
    win = np.asarray(win, dtype=np.int64)
    fx, fy = np.asarray(fx, dtype=np.int64), np.asarray(fy, dtype=np.int64)
    if r0 is None:
        r0, r1 = rounds(bd)
    ob = bd + 14 - r0
    ro = (1 << (ob - r1)) + (1 << (ob - r1 - 1))
    if form == 0:
        res = ((win[3:3 + h, 3:3 + w] << (14 - r0 - r1)) & 0xFFFF) + ro
        return res & 0xFFFF
    if form == 1:
        s = sum(fx[k] * win[3:3 + h, k:k + w] for k in range(8))
        return (1 << (7 - r1)) * _rnd(s, r0) + ro
    if form == 2:
        s = sum(fy[k] * win[k:k + h, 3:3 + w] for k in range(8))
        return _rnd(s * (1 << (7 - r0)), r1) + ro
    im = (1 << (bd + 6)) + sum(fx[k] * win[:, k:k + w] for k in range(8))
    im = _rnd(im, r0).astype(np.int16).astype(np.int64)
    s = (1 << ob) + sum(fy[k] * im[k:k + h] for k in range(8))
    return _rnd(s, r1) & 0xFFFF


def combine(tmp, res, mode, bd, r0=None, r1=None):
    """The second call's tail: tmp the stored CONV_BUF_TYPE block, res the second reference's first_pass; mode (dist_wtd,
    fwd_offset, bck_offset)."""
    if r0 is None:
        r0, r1 = rounds(bd)
    ob = bd + 14 - r0
    tmp = np.asarray(tmp, dtype=np.int64)
    t = (tmp * mode[1] + res * mode[2]) >> 4 if mode[0] else (tmp + res) >> 1
    t = t - ((1 << (ob - r1)) + (1 << (ob - r1 - 1)))
    return np.clip(_rnd(t, 14 - r0 - r1), 0, (1 << bd) - 1)


def block_source(bd, w, h, content, index, which):
    """The drawn (h + 8) x (w + 8) source buffer `which` (0 or 1) of block record `index`; the block is at (3, 3)."""
    maxv = (1 << bd) - 1
    bw, bh = w + 8, h + 8
    if content == 0:
        a = draw(0x4A4E000000000000 + 16 * index + 8 * which, bw * bh, maxv + 1).reshape(bh, bw)
    elif content in (1, 2):
        a = np.full((bh, bw), 0 if content == 1 else maxv, dtype=np.int64)
    else:
        y, x = np.mgrid[0:bh, 0:bw]
        a = np.where((x + y + which) & 1, maxv, 0).astype(np.int64)
    return a.astype(np.uint16 if bd > 8 else np.uint8)


@functools.lru_cache(maxsize=1)
def block_cases():
    g = fixture()
    out = []
    for i in range(int(g["nblock"][0])):
        bd, w, h, phx, phy, kind, content, form, idx, dist, fwd, bck = (int(v) for v in g["b%d_par" % i])
        out.append(dict(name="b%d" % i, bd=bd, w=w, h=h, phx=phx, phy=phy, kind=kind, content=content, form=form, index=idx,
                        mode=(dist, fwd, bck), conv=g["b%d_conv" % i], out=g["b%d_out" % i],
                        mm=tuple(int(v) for v in g["b%d_mm" % i])))
    return out


def block_filters(c):
    t = tables()
    return t[filter_table(c["kind"], c["w"])][c["phx"]], t[filter_table(c["kind"], c["h"])][c["phy"]]


def block_expected(c):
    """(the CONV_BUF_TYPE block after the first call, the pixels after the second)."""
    fx, fy = block_filters(c)
    w, h = c["w"], c["h"]
    s0, s1 = (block_source(c["bd"], w, h, c["content"], c["index"], k)[:h + 7, :w + 7] for k in (0, 1))
    conv = first_pass(s0, w, h, fx, fy, c["form"], c["bd"]) & 0xFFFF
    return conv, combine(conv, first_pass(s1, w, h, fx, fy, c["form"], c["bd"]), c["mode"], c["bd"])


# ---------------------------------------------------------------------------------------------
# the batch predictor
# ---------------------------------------------------------------------------------------------
def clamp_mv(mv, org, b, dim, ss):
    """One component (clamp_mv_to_umv_border_sb with the block's own edges): MV in 1/8 luma sample of a block of luma size b
    at luma origin org in a picture of luma size dim -> (offset of the source from the block's origin in the plane, phase)."""
    sc = 1 - ss
    q = _i16(mv * (1 << sc))
    spel = (4 + (b >> ss)) << 4
    lo = -(org * 8) * (1 << sc) - spel
    hi = ((dim - b - org) * 8) * (1 << sc) + spel - 16
    q = _i16(min(max(q, lo), hi))
    return q >> 4, q & 15


def padded_reference(bd, w, h, seed, pad):
    """The three planes of a drawn reference picture with edge-replicated borders of `pad` luma samples."""
    sc, maxv, planes = 1 << (bd - 8), (1 << bd) - 1, []
    for p in range(3):
        pw, ph = w >> (p > 0), h >> (p > 0)
        y, x = np.mgrid[0:ph, 0:pw]
        a = np.clip((2 * x + y) * sc // 4 + draw(seed + p, pw * ph, 64 * sc).reshape(ph, pw), 0, maxv)
        planes.append(np.pad(a, pad >> (p > 0), mode="edge").astype(np.uint16 if bd > 8 else np.uint8))
    return planes


def predict_batch(refs, pad, blocks, bd, w, h, chroma, border=None, out=None, fill=0):
    """refs: per reference three padded planes (`pad` luma samples around the picture); blocks: dicts with x, y, w, h, ref0,
    ref1, mv0, mv1, fx, fy, mode.  border = (bx, by) clamps every read coordinate into [-border, size + border - 1] as the
    library does; None: unclamped, which needs the planes to hold what is read.  Returns the three predictor planes (`fill`
    where no block writes)."""
    t = tables()
    if out is None:
        out = [np.full((h >> (p > 0), w >> (p > 0)), fill, dtype=refs[0][0].dtype) for p in range(3)]
    for b in blocks:
        for p in range(3 if chroma else 1):
            ss = int(p > 0)
            bw, bh, pd, pw, ph = b["w"] >> ss, b["h"] >> ss, pad >> ss, w >> ss, h >> ss
            ox, oy = (((b["x"] >> 3) << 3) >> 1, ((b["y"] >> 3) << 3) >> 1) if ss else (b["x"], b["y"])
            fxt, fyt = filter_table(b["fx"], bw), filter_table(b["fy"], bh)
            passes = []
            for ref, mv in ((b["ref0"], b["mv0"]), (b["ref1"], b["mv1"])):
                dx, phx = clamp_mv(mv[0], b["x"], b["w"], w, ss)
                dy, phy = clamp_mv(mv[1], b["y"], b["h"], h, ss)
                xs, ys = np.arange(ox + dx - 3, ox + dx + bw + 4), np.arange(oy + dy - 3, oy + dy + bh + 4)
                if border is not None:
                    xs = np.clip(xs, -(border[0] >> ss), pw + (border[0] >> ss) - 1)
                    ys = np.clip(ys, -(border[1] >> ss), ph + (border[1] >> ss) - 1)
                form = (1 if phx else 0) | (2 if phy else 0)
                # only what the form reads has to be there
                if not form & 1:
                    xs[:3], xs[-4:] = xs[3], xs[-5]
                if not form & 2:
                    ys[:3], ys[-4:] = ys[3], ys[-5]
                assert xs.min() >= -pd and ys.min() >= -pd and xs.max() < pw + pd and ys.max() < ph + pd, (b, p)
                win = refs[ref][p][np.ix_(ys + pd, xs + pd)]
                passes.append(first_pass(win, bw, bh, t[fxt][phx], t[fyt][phy], form, bd))
            out[p][oy:oy + bh, ox:ox + bw] = combine(passes[0] & 0xFFFF, passes[1], b["mode"], bd)
    return out


def _blocks(rows):
    return [dict(x=int(v[0]), y=int(v[1]), w=int(v[2]), h=int(v[3]), ref0=int(v[4]), ref1=int(v[5]), mv0=(int(v[6]), int(v[7])),
                 mv1=(int(v[8]), int(v[9])), fx=int(v[10]), fy=int(v[11]), mode=(int(v[12]), int(v[13]), int(v[14])))
            for v in rows]


@functools.lru_cache(maxsize=1)
def batch_cases():
    g = fixture()
    out = []
    for i in range(int(g["nbatch"][0])):
        bd, w, h, nr, chroma, border, nb, idx = (int(v) for v in g["q%d_par" % i])
        refs = [padded_reference(bd, w, h, 0x4A4E000000100000 + 256 * idx + 4 * r, border) for r in range(nr)]
        out.append(dict(name="q%d" % i, bd=bd, w=w, h=h, n_refs=nr, chroma=chroma, pad=border, refs=refs,
                        blocks=_blocks(g["q%d_blocks" % i]), pred=[g["q%d_pred%d" % (i, p)] for p in range(3 if chroma else 1)],
                        kinds=[int(v) for v in g["q%d_kinds" % i]]))
    return out


def pyramid_blocks(rng, w=128, h=64):
    """The list of the cross-check picture: one 64x64, two 32x64, ... down to 8x8 (w x h = 128 x 64), every MV one eighth
    inside the MV clamp's bound or far outside it, in turn on each side."""
    shapes, x = [], 0
    for bw, bh, n in ((64, 64, 1), (32, 64, 2)):
        for _ in range(n):
            shapes.append((x, 0, bw, bh))
            x += bw
    assert x == w
    # the second 32x64 column is replaced by smaller blocks, still a tiling: 32x32, 32x16, 16x16, 16x8, 8x8, 8x8
    shapes[-1:] = [(96, 0, 32, 32), (96, 32, 32, 16), (96, 48, 16, 16), (112, 48, 16, 8), (112, 56, 8, 8), (120, 56, 8, 8)]
    blocks = []
    for k, (bx, by, bw, bh) in enumerate(shapes):
        def bound(org, b, dim, side, far):
            lo, hi = -(org * 16) - ((4 + b) << 4), (dim - b - org) * 16 + ((4 + b) << 4) - 16
            if far:
                return -(dim * 8 + 1200) if side else dim * 8 + 1200
            return (lo // 2 + 1) if side else (hi // 2 - 1)  # one eighth inside, in 1/8 luma sample
        mv0 = (bound(bx, bw, w, k & 1, False), bound(by, bh, h, (k >> 1) & 1, False))
        mv1 = (bound(bx, bw, w, (k + 1) & 1, k % 3 == 0), bound(by, bh, h, k & 1, k % 3 != 0))
        mode = (1,) + tuple(MODES[1 + k % 8][1:]) if k & 1 else (0, 0, 0)
        blocks.append(dict(x=bx, y=by, w=bw, h=bh, ref0=int(rng.integers(0, 2)), ref1=int(rng.integers(0, 2)), mv0=mv0, mv1=mv1,
                           fx=k & 3, fy=(k >> 1) & 3, mode=mode))
    return blocks
