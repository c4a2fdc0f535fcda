"""AV1 masked compound prediction (COMPOUND_WEDGE, COMPOUND_DIFFWTD): reader of tests/golden/masked_compound.bin (written by
tests/golden/gen_golden_masked_compound.c from the reference's own C) and a numpy restatement, written from the C, of the
wedge masks (svt_av1_init_wedge_masks, EbInterPrediction.c:1445-2132), the DIFFWTD mask
(svt_av1_build_compound_diffwtd_mask_d16_c), the four forms of svt_aom_(lowbd|highbd)_blend_a64_d16_mask_c and
svt_aom_inter_prediction's masked path.  The two reference passes are tests/compound_cases.py's, which tests/test_compound.py
holds to the reference.  Shared by tests/test_masked_compound.py (CPU) and tests/test_masked_compound_gpu.py."""
import functools
import os

import numpy as np

import compound_cases as cc
import golden_io
from interp_cases import _rnd, filter_table, tables
from tf_cases import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masked_compound.bin")
WEDGE_SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (8, 32), (32, 8)]  # BlockSize order
SUB_FORMS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (subw, subh) of b<i>_out<f>, f = subw + 2 * subh
WEDGE, DIFFWTD = 0, 1

# the reference's three primary rows
_ODD = [0] * 28 + [1, 2, 6, 18, 37, 53, 60, 63] + [64] * 28
_EVEN = [0] * 28 + [1, 4, 11, 27, 46, 58, 62, 63] + [64] * 28
_VERT = [0] * 28 + [0, 2, 7, 21, 43, 57, 62, 64] + [64] * 28
H, V, O27, O63, O117, O153 = range(6)
_HEAD = [(O27, 4, 4), (O63, 4, 4), (O117, 4, 4), (O153, 4, 4)]
_TAIL = [(O27, 4, 2), (O27, 4, 6), (O153, 4, 2), (O153, 4, 6), (O63, 2, 4), (O63, 6, 4), (O117, 2, 4), (O117, 6, 4)]
CODEBOOK_HGTW = _HEAD + [(H, 4, 2), (H, 4, 4), (H, 4, 6), (V, 4, 4)] + _TAIL
CODEBOOK_HLTW = _HEAD + [(V, 2, 4), (V, 4, 4), (V, 6, 4), (H, 4, 4)] + _TAIL
CODEBOOK_HEQW = _HEAD + [(H, 4, 2), (H, 4, 6), (V, 2, 4), (V, 6, 4)] + _TAIL
_FLIP_SQUARE = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1]
_FLIP_2TO1 = [1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1]
SIGNFLIP = {(8, 32): [1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1, 1, 1, 0, 1], (32, 8): [1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1]}


@functools.lru_cache(maxsize=1)
def fixture():
    return golden_io.load(GOLDEN)


@functools.lru_cache(maxsize=1)
def golden_wedges():
    """{(w, h, index, sign): uint8 [h][w]} of the fixture's 288 masks."""
    g = fixture()
    assert [tuple(int(v) for v in r) for r in g["wedge_sizes"]] == WEDGE_SIZES and g["wedge"].size == 100352
    out, o = {}, 0
    for w, h in WEDGE_SIZES:
        for i in range(16):
            for s in range(2):
                out[(w, h, i, s)] = g["wedge"][o:o + w * h].reshape(h, w)
                o += w * h
    return out


def _shift_copy(src, shift):
    src = np.asarray(src)
    if shift >= 0:
        return np.concatenate([np.full(shift, src[0]), src[:64 - shift]])
    return np.concatenate([src[-shift:], np.full(-shift, src[63])])


@functools.lru_cache(maxsize=1)
def wedge_primaries():
    """init_wedge_primary_masks: [negative][direction] 64x64."""
    m = np.zeros((2, 6, 64, 64), np.int64)
    shift = 16
    for i in range(0, 64, 2):
        m[0, O63, i] = _shift_copy(_EVEN, shift)
        shift -= 1
        m[0, O63, i + 1] = _shift_copy(_ODD, shift)
        m[0, V, i] = m[0, V, i + 1] = _VERT
    m[0, O27] = m[0, O63].T
    m[0, O117] = 64 - m[0, O63][:, ::-1]
    m[0, O153] = m[0, O117].T  # [(w - 1 - j)][i] = 64 - msk(i, j): the transpose of OBLIQUE117
    m[0, H] = m[0, V].T
    m[1] = 64 - m[0]
    return m


def wedge_mask(w, h, index, sign):
    """get_wedge_mask_inplace + the copy of init_wedge_masks."""
    book = CODEBOOK_HGTW if h > w else CODEBOOK_HLTW if h < w else CODEBOOK_HEQW
    flip = SIGNFLIP.get((w, h), _FLIP_SQUARE if w == h else _FLIP_2TO1)[index]
    d, xo, yo = book[index]
    r0, c0 = 32 - ((yo * h) >> 3), 32 - ((xo * w) >> 3)
    return wedge_primaries()[sign ^ flip, d, r0:r0 + h, c0:c0 + w].astype(np.uint8)


def diffwtd_mask(c0, c1, mask_type, bd, r0=None, r1=None):
    if r0 is None:
        r0, r1 = cc.rounds(bd)
    d = np.abs(np.asarray(c0, np.int64) - np.asarray(c1, np.int64))
    m = np.clip(38 + _rnd(d, 14 - r0 - r1 + bd - 8) // 16, 0, 64)
    return (64 - m if mask_type else m).astype(np.uint8)


def sub_mask(mask, subw, subh):
    """The mask value per output sample of the four blend forms."""
    m = np.asarray(mask, np.int64)
    if subw and subh:
        return (m[0::2, 0::2] + m[1::2, 0::2] + m[0::2, 1::2] + m[1::2, 1::2] + 2) >> 2
    if subw:
        return (m[:, 0::2] + m[:, 1::2] + 1) >> 1
    if subh:
        return (m[0::2] + m[1::2] + 1) >> 1
    return m


def blend(m, c0, c1, bd, r0=None, r1=None):
    if r0 is None:
        r0, r1 = cc.rounds(bd)
    ob = bd + 14 - r0
    res = ((m * np.asarray(c0, np.int64) + (64 - m) * np.asarray(c1, np.int64)) >> 6) - ((1 << (ob - r1)) + (1 << (ob - r1 - 1)))
    return np.clip(_rnd(res, 14 - r0 - r1), 0, (1 << bd) - 1)


def block_source(bd, w, h, content, index, which):
    """The drawn (h + 8) x (w + 8) source buffer `which` (0 or 1) of block record `index`; the block is at (3, 3)."""
    maxv, bw, bh = (1 << bd) - 1, w + 8, h + 8
    y, x = np.mgrid[0:bh, 0:bw]
    if content == 0:
        a = draw(0x4D43000000000000 + 16 * index + 8 * which, bw * bh, maxv + 1).reshape(bh, bw)
    elif content in (1, 2):
        a = np.full((bh, bw), 0 if content == 1 else maxv, dtype=np.int64)
    elif content == 3:
        a = np.where((x + y + which) & 1, maxv, 0)
    else:
        a = np.where(((0x5A >> (x & 7)) ^ which) & 1, maxv, 0)
    return a.astype(np.uint16 if bd > 8 else np.uint8)


@functools.lru_cache(maxsize=1)
def block_cases():
    """The block records with their two CONV_BUF_TYPE blocks rebuilt (c0, c1: uint16 [h][w])."""
    g, t, out = fixture(), tables(), []
    for i in range(int(g["nblock"][0])):
        bd, w, h, phx, phy, kind, content, form, idx = (int(v) for v in g["b%d_par" % i])
        fx, fy = t[filter_table(kind, w)][phx], t[filter_table(kind, h)][phy]
        conv = [(cc.first_pass(block_source(bd, w, h, content, idx, k)[:h + 7, :w + 7], w, h, fx, fy, form, bd) & 0xFFFF).astype(np.uint16)
                for k in (0, 1)]
        outs = {f: g["b%d_out%d" % (i, f)] for f in range(4) if "b%d_out%d" % (i, f) in g}
        out.append(dict(name="b%d" % i, bd=bd, w=w, h=h, content=content, form=form, kind=kind, index=idx, c0=conv[0], c1=conv[1],
                        masks=[g["b%d_mask%d" % (i, k)] for k in (0, 1)], outs=outs, mm=tuple(int(v) for v in g["b%d_mm" % i])))
    return out


# ---------------------------------------------------------------------------------------------
# the batch predictor
# ---------------------------------------------------------------------------------------------
def predict_batch(refs, pad, blocks, bd, w, h, chroma, border=None, fill=0):
    """As compound_cases.predict_batch with the masked combine: blocks carry type, widx, wsign, mtype."""
    t = tables()
    out = [np.full((h >> (p > 0), w >> (p > 0)), fill, dtype=refs[0][0].dtype) for p in range(3)]
    for b in blocks:
        luma_mask = None
        for p in range(3 if chroma else 1):
            ss = int(p > 0)
            bw, bh, pd, pw, ph = b["w"] >> ss, b["h"] >> ss, pad >> ss, w >> ss, h >> ss
            ox, oy = (((b["x"] >> 3) << 3) >> 1, ((b["y"] >> 3) << 3) >> 1) if ss else (b["x"], b["y"])
            fxt, fyt = filter_table(b["fx"], bw), filter_table(b["fy"], bh)
            passes = []
            for ref, mv in ((b["ref0"], b["mv0"]), (b["ref1"], b["mv1"])):
                dx, phx = cc.clamp_mv(mv[0], b["x"], b["w"], w, ss)
                dy, phy = cc.clamp_mv(mv[1], b["y"], b["h"], h, ss)
                xs, ys = np.arange(ox + dx - 3, ox + dx + bw + 4), np.arange(oy + dy - 3, oy + dy + bh + 4)
                if border is not None:
                    xs = np.clip(xs, -(border[0] >> ss), pw + (border[0] >> ss) - 1)
                    ys = np.clip(ys, -(border[1] >> ss), ph + (border[1] >> ss) - 1)
                form = (1 if phx else 0) | (2 if phy else 0)
                if not form & 1:
                    xs[:3], xs[-4:] = xs[3], xs[-5]
                if not form & 2:
                    ys[:3], ys[-4:] = ys[3], ys[-5]
                assert xs.min() >= -pd and ys.min() >= -pd and xs.max() < pw + pd and ys.max() < ph + pd, (b, p)
                win = refs[ref][p][np.ix_(ys + pd, xs + pd)]
                passes.append(cc.first_pass(win, bw, bh, t[fxt][phx], t[fyt][phy], form, bd) & 0xFFFF)
            if p == 0:
                luma_mask = wedge_mask(b["w"], b["h"], b["widx"], b["wsign"]) if b["type"] == WEDGE else \
                    diffwtd_mask(passes[0], passes[1], b["mtype"], bd)
            out[p][oy:oy + bh, ox:ox + bw] = blend(sub_mask(luma_mask, ss, ss), passes[0], passes[1], bd)
    return out


def _blocks(rows):
    return [dict(x=int(v[0]), y=int(v[1]), w=int(v[2]), h=int(v[3]), ref0=int(v[4]), ref1=int(v[5]), mv0=(int(v[6]), int(v[7])),
                 mv1=(int(v[8]), int(v[9])), fx=int(v[10]), fy=int(v[11]), type=int(v[12]), widx=int(v[13]), wsign=int(v[14]),
                 mtype=int(v[15])) for v in rows]


@functools.lru_cache(maxsize=1)
def batch_cases():
    g = fixture()
    out = []
    for i in range(int(g["nbatch"][0])):
        bd, w, h, nr, chroma, border, nb, idx = (int(v) for v in g["q%d_par" % i])
        # the planes hold 80 replicated samples whatever the record declares: replicated, they are what the reference read
        refs = [cc.padded_reference(bd, w, h, 0x4D43000000100000 + 256 * idx + 4 * r, 80) for r in range(nr)]
        out.append(dict(name="q%d" % i, bd=bd, w=w, h=h, n_refs=nr, chroma=chroma, pad=80, border=border, refs=refs,
                        blocks=_blocks(g["q%d_blocks" % i]), pred=[g["q%d_pred%d" % (i, p)] for p in range(3 if chroma else 1)],
                        kinds=[int(v) for v in g["q%d_kinds" % i]]))
    return out
